// Tree reuse as a workgroup's job: the sliding compaction of dev_search.h (advance_tree_scalar is its one-lane
// statement) for one tree, over (source records, destination records, hi, keep_root), with nothing in it that knows
// about slots, pages or streams. The result is advance_tree_scalar's, byte for byte.
//
// Fast path (trees of up to ADV_MAX_NODES nodes from the kept root on):
//   1. parents: all threads load h1.parent of the nodes keep_root .. hi-1, a tile of ADV_TILE at a time, into LDS
//      (independent loads, all of a tile in flight); nothing below keep_root is read -- it is all dropped, and no
//      kept node refers to it. Ids in LDS are relative to keep_root and 16 bits wide.
//   2. keep flags and new ids: one wavefront runs the recurrence keep[i] = keep[parent[i]] 64 ids at a time over the
//      tile; a parent in an earlier group reads its flag from the keep bitmap in LDS, a parent in the same group resolves
//      by the shuffle loop. The new id of a kept node is its rank among the kept ones: the group's running count plus a
//      popcount below its bit, so the bitmap and one count per 64 ids ARE the table old id -> new id -- and, read the
//      other way (a search over the counts, then the k-th set bit of a word), the list src[new id] = old id. A list of
//      its own and 16-bit new ids would take 4 bytes of LDS per node; this takes 1.25 bits plus the tile of parents, 9.5 KB
//      for any tree of the fast path, which fits beside two workgroups of the MLP evaluator (74 KB each of a CU's 160).
//   3. the caller picks the destination once the count is known (the same records, or a run of another size).
//   4. move, by 16-byte group: unit u is group u % 20 of kept node u / 20, so twenty consecutive lanes read one
//      contiguous record and the stores to dst + 16 u are contiguous across the whole block. The units that hold ids
//      (adv_id_words) are mapped through the table on the way. The move goes in chunks of ADV_CHUNK_NODES whole kept nodes:
//      the source node of each is looked up once per chunk, into a 16-bit list in LDS (two lists of a chunk: 204 bytes,
//      not the 2 bytes per node of a list of the whole tree), and the loads of the next chunks are in flight while a
//      chunk waits, passes its barrier and is stored (adv_move_lds).
// The slow path (any hi) keeps new ids in the arena's fwd[] in global memory: the recurrence as one wavefront ran it
// before, then a move by 25 old nodes per step over all threads.
#pragma once
#include "dev_search.h"

#include <cstddef>

namespace ar {

enum {
    ADV_THREADS = 512,
    ADV_TILE = 2048,             // parents in LDS at a time
    ADV_MAX_NODES = 32768,       // hi - keep_root of the fast path: bitmap + counts cover this many ids
    ADV_UNITS = 2,               // units per thread and chunk of the move
    ADV_CHUNK_NODES = ADV_THREADS * ADV_UNITS / NODE_GROUPS,  // a chunk: 51 whole kept nodes (1020 units, 16 KB)
    ADV_CHUNK_UNITS = ADV_CHUNK_NODES * NODE_GROUPS,
    ADV_DEPTH = 3,               // chunks in flight: the loads of chunk c + ADV_DEPTH - 1 are issued before chunk c's barrier
    ADV_PARENT_GROUP = 11,       // h1: {scale, r1, r2, parent}
    ADV_SLOW_NODES = ADV_THREADS / NODE_GROUPS,  // old nodes per step of the slow path's move
};
static_assert(offsetof(NodeStats, h1) + offsetof(NodeH1, parent) == ADV_PARENT_GROUP * 16 + 12, "parent: word 3 of group 11");
static_assert(offsetof(NodeStats, c) == NODE_KID_GROUP * 16 && offsetof(NodeStats, pad) == 19 * 16 + 4, "child ids: groups 13..19");
static_assert(ADV_MAX_NODES < 0xFFFF && ADV_TILE % 64 == 0 && ADV_TILE % ADV_THREADS == 0, "16-bit relative ids");

// ---- index logic of the move (runs on the CPU too: tests/hostsim_advance) ---------------------------------------------
AR_HD uint32_t adv_unit_node(uint32_t u) { return u / NODE_GROUPS; }
AR_HD uint32_t adv_unit_group(uint32_t u) { return u % NODE_GROUPS; }
// bit w set: word w of group g holds a node id (the parent; 25 child ids, the last three words of group 19 are pad)
AR_HD uint32_t adv_id_words(uint32_t g) {
    return g == ADV_PARENT_GROUP ? 8u : g < NODE_KID_GROUP ? 0u : g < NODE_GROUPS - 1 ? 15u : 1u;
}
// new id of the kept node `rel` ids above keep_root: kept nodes below it. bits: keep flags, 64 ids a word;
// before[w]: kept nodes in the words below w
AR_HD uint32_t adv_new_id(const unsigned long long* bits, const uint16_t* before, uint32_t rel) {
    const unsigned long long below = bits[rel >> 6] & ((1ULL << (rel & 63u)) - 1ULL);
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)before[rel >> 6] + (uint32_t)__popcll(below);
#else
    return (uint32_t)before[rel >> 6] + (uint32_t)__builtin_popcountll(below);
#endif
}
// old id (relative to keep_root) of the kept node with new id k < the kept count: the word that holds it is the largest
// w with before[w] <= k (before[w + 1] = before[w] + the word's bits > k), then the (k - before[w])-th set bit of it.
// words: 64-id words the tree has. from_word: a word at or below the one that holds it (a thread's units go up through
// the kept nodes, 1/20 of a chunk at a time, so the word of its last unit is a few words short at most: a few steps
// forward, and a binary search over the rest only when those were not enough). The move no longer searches (adv_fill_list
// below); this stays as the statement of what a list entry is, and tests/hostsim_advance runs it.
AR_HD uint32_t adv_src_node(const unsigned long long* bits, const uint16_t* before, uint32_t words, uint32_t k, uint32_t from_word) {
    uint32_t lo = from_word, hi = words - 1;
    for (int step = 0; step < 4 && lo < hi && (uint32_t)before[lo + 1] <= k; ++step) ++lo;
    if (lo < hi && (uint32_t)before[lo + 1] > k) hi = lo;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if ((uint32_t)before[mid] <= k) lo = mid;
        else hi = mid - 1;
    }
    uint32_t r = k - (uint32_t)before[lo];
    const unsigned long long w = bits[lo];
    uint32_t pos = 0;
    for (uint32_t s = 32; s; s >>= 1) {
        const unsigned long long part = (w >> pos) & ((1ULL << s) - 1ULL);
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t c = (uint32_t)__popcll(part);
#else
        const uint32_t c = (uint32_t)__builtin_popcountll(part);
#endif
        if (r >= c) {
            r -= c;
            pos += s;
        }
    }
    return lo * 64u + pos;
}
// The source list of a chunk, src[n0 + k] = old id (relative to keep_root) for the chunk's kept nodes k = 0 .. nodes - 1,
// without a search: where the id `rel` goes in it (ADV_NOT_LISTED: dropped, or a node of another chunk).
static const uint32_t ADV_NOT_LISTED = 0xFFFFFFFFu;
AR_HD uint32_t adv_list_slot(const unsigned long long* bits, const uint16_t* before, uint32_t rel, uint32_t n0, uint32_t nodes) {
    if (!((bits[rel >> 6] >> (rel & 63u)) & 1ULL)) return ADV_NOT_LISTED;
    const uint32_t k = adv_new_id(bits, before, rel) - n0;  // (below n0: wraps to a large number)
    return k < nodes ? k : ADV_NOT_LISTED;
}
// Thread `tid` of `threads` (a multiple of 64) fills its part of the list: the threads take one id each of a window of
// `threads` ids that starts at word from_word, and the window moves up until the words below it hold the whole chunk.
// from_word: a word at or below the one that holds kept node n0 (the word of the last node of the chunk before).
// cnt: the tree's kept count; nothing is written for n0 >= cnt. No two threads write the same entry, and a thread needs
// nothing another one writes: one barrier after the call publishes the list.
AR_HD void adv_fill_list(const unsigned long long* bits, const uint16_t* before, uint32_t words, uint32_t cnt, uint32_t n0,
                         uint32_t from_word, uint32_t tid, uint32_t threads, uint16_t* list) {
    if (n0 >= cnt) return;
    const uint32_t nodes = cnt - n0 < (uint32_t)ADV_CHUNK_NODES ? cnt - n0 : (uint32_t)ADV_CHUNK_NODES;
    for (uint32_t w0 = from_word; w0 < words; w0 += threads / 64u) {
        const uint32_t rel = w0 * 64u + tid;
        if ((rel >> 6) < words) {
            const uint32_t k = adv_list_slot(bits, before, rel, n0, nodes);
            if (k != ADV_NOT_LISTED) list[k] = (uint16_t)rel;
        }
        const uint32_t next = w0 + threads / 64u;
        if (next < words && (uint32_t)before[next] >= n0 + nodes) break;  // (the words from `next` on hold later nodes only)
    }
}
// The k-th unit of thread `tid` in chunk c of a tree of `units` units. Local unit j (< ADV_CHUNK_UNITS) is group j % 20 of
// the chunk's kept node j / 20 and unit c * ADV_CHUNK_UNITS + j of the tree. Every thread has ADV_UNITS units in every
// chunk, on no condition (adv_move_lds says why): the few threads whose k-th local unit would lie past the chunk's last
// repeat that last unit (the same load, the same store of the same bytes), and a unit past the tree's last loads the kept
// root's first group and is not stored.
struct AdvUnit {
    uint32_t j, u;  // local unit (clamped), the tree's unit
    bool in_tree;   // u < units
};
AR_HD AdvUnit adv_chunk_unit(uint32_t c, uint32_t k, uint32_t tid, uint32_t units) {
    AdvUnit x;
    x.j = k * ADV_THREADS + tid;
    if (x.j >= (uint32_t)ADV_CHUNK_UNITS) x.j = ADV_CHUNK_UNITS - 1u;
    x.u = c * ADV_CHUNK_UNITS + x.j;
    x.in_tree = x.u < units;
    return x;
}
// where the unit is loaded from, in 16-byte groups from the kept root's record on; entry: the chunk's source list entry of
// the unit's node (anything, if the unit is past the tree)
AR_HD uint32_t adv_unit_source(const AdvUnit& x, uint32_t entry) { return x.in_tree ? entry * NODE_GROUPS + adv_unit_group(x.j) : 0u; }
// whole: the chunk is one of the cnt / ADV_CHUNK_NODES whole ones (every unit of it is in the tree)
AR_HD bool adv_unit_stored(const AdvUnit& x, bool whole) { return whole || x.in_tree; }
// the register buffer a chunk's units wait in
AR_HD uint32_t adv_chunk_buffer(uint32_t c) { return c % ADV_DEPTH; }
static_assert(ADV_DEPTH >= 2, "the rest of a tree is loaded ADV_DEPTH - 1 steps ahead like any chunk: something must be ahead");

// one unit on its way from the source to the destination: w = the four words of group g of a kept node
// (is_root: of the kept root, whose parent becomes NIL); new_id maps an old id of a kept node
template <class NewId>
AR_HD void adv_remap_unit(uint32_t w[4], uint32_t g, bool is_root, NewId new_id) {
    const uint32_t ids = adv_id_words(g);
    if (ids == 0) return;
    for (int k = 0; k < 4; ++k) {
        if (!((ids >> k) & 1u)) continue;
        if (g == ADV_PARENT_GROUP) w[k] = is_root ? NIL : new_id(w[k]);
        else if (w[k] != NIL) w[k] = new_id(w[k]);
    }
}

#if defined(__HIPCC__)
struct AdvLds {
    unsigned long long bits[ADV_MAX_NODES / 64];  // keep flags by id relative to keep_root
    uint16_t before[ADV_MAX_NODES / 64];          // kept nodes in the words below
    uint16_t par[ADV_TILE];                       // parents of the tile, relative to keep_root (ADV_NONE: dropped for sure)
    uint16_t list[2][ADV_CHUNK_NODES];            // source lists of the move: chunk c's in list[c & 1]
    uint32_t cnt;
    uint32_t pick;                                // the caller's word (which destination was picked)
    uint32_t ticket;                              // the caller's word (which entry of the launch's list comes next)
};
static const uint32_t ADV_NONE = 0xFFFFu;

// all loaded values are in their registers when this returns (a use the compiler cannot move or drop)
__device__ inline void adv_arrived(uint4& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }

// steps 1 and 2. All ADV_THREADS threads call it; returns the number of kept nodes (to all).
__device__ inline uint32_t adv_mark_lds(const NodeStats* src, uint32_t hi, uint32_t keep_root, AdvLds& L) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, n = hi - keep_root;
    const uint32_t* parent = &src[keep_root].h1.parent;
    constexpr uint32_t STRIDE = sizeof(NodeStats) / 4, PER = ADV_TILE / ADV_THREADS;
    uint32_t cnt = 0;  // (first wavefront)
    for (uint32_t t0 = 0; t0 < n; t0 += ADV_TILE) {
        const uint32_t tn = n - t0 < (uint32_t)ADV_TILE ? n - t0 : (uint32_t)ADV_TILE;
        uint32_t p[PER];
#pragma unroll
        for (uint32_t k = 0; k < PER; ++k) {
            const uint32_t j = tid + k * ADV_THREADS;
            p[k] = j < tn ? parent[(size_t)(t0 + j) * STRIDE] : NIL;
        }
#pragma unroll
        for (uint32_t k = 0; k < PER; ++k) {
            const uint32_t j = tid + k * ADV_THREADS;
            if (j < tn) L.par[j] = (p[k] != NIL && p[k] >= keep_root) ? (uint16_t)(p[k] - keep_root) : (uint16_t)ADV_NONE;
        }
        __syncthreads();
        if (tid < 64) {
            uint32_t pr_next = lane < tn ? (uint32_t)L.par[lane] : (uint32_t)ADV_NONE;
            for (uint32_t g0 = 0; g0 < tn; g0 += 64) {
                const uint32_t base = t0 + g0, j = base + lane;
                uint32_t st = 2, pr = ADV_NONE;  // 0 unknown, 1 keep, 2 drop
                const uint32_t pr_here = pr_next;  // (the next group's parents are on their way during this group's rounds)
                pr_next = g0 + 64 + lane < tn ? (uint32_t)L.par[g0 + 64 + lane] : (uint32_t)ADV_NONE;
                if (g0 + lane < tn) {
                    if (j == 0) st = 1;
                    else {
                        pr = pr_here;
                        if (pr == ADV_NONE) st = 2;
                        else if (pr < base) st = ((L.bits[pr >> 6] >> (pr & 63u)) & 1ULL) ? 1u : 2u;
                        else st = 0;
                    }
                }
                // parents inside this group of 64: propagate along the id order (parent lane < child lane)
                for (int round = 0; round < 64; ++round) {
                    const uint32_t from = (st == 0) ? (pr - base) : lane;
                    const uint32_t pst = (uint32_t)__shfl((int)st, (int)from, 64);
                    if (st == 0 && pst != 0) st = pst;
                    if (!__any(st == 0)) break;
                }
                const bool keep = st == 1;
                const unsigned long long bal = __ballot(keep);
                if (lane == 0) {
                    L.bits[base >> 6] = bal;
                    L.before[base >> 6] = (uint16_t)cnt;
                }
                cnt += (uint32_t)__popcll(bal);
                // the next group's lanes read this group's flags (one wavefront, LDS: an ordering, no cache traffic)
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
        }
        __syncthreads();  // (the next tile's parents overwrite this one's)
    }
    if (tid == 0) L.cnt = cnt;
    __syncthreads();
    return L.cnt;
}

// step 4. A chunk is ADV_CHUNK_NODES whole kept nodes, so a thread's units are the same groups of the same nodes of every
// chunk. The chunk's source list (adv_fill_list) is in LDS before its loads are issued: one lookup per kept node, and a
// unit's lanes read their node's entry. In place, units go in increasing order in chunks, and every load of a chunk has
// RETURNED before any store of the chunk is issued (registers filled, then a barrier). No other ordering is needed:
// src[n] >= n, so the source of unit u lies at or above dst + 16 u. A chunk's stores therefore land at or below its own
// sources, which it has read already, and below the sources of every later chunk, which lie above everything written so
// far -- so the loads of the next ADV_DEPTH - 1 chunks are issued BEFORE this chunk's wait, barrier and stores and stay
// in flight across them. A tree that moves to other records waits for no load at the barrier, which is then only what
// publishes the next list. Step c: loads of chunk c + ADV_DEPTH - 1, list of chunk c + ADV_DEPTH (into the buffer whose
// readers all passed the barrier before), wait for chunk c, barrier, ids mapped, stores of chunk c.
// Forced inline: as a called function its record pointers are generic, and flat loads also count on the counter that the
// waits for LDS reads use (profiles/r08_resource_usage.txt).
__device__ __forceinline__ void adv_move_lds(const NodeStats* src, NodeStats* dst, uint32_t hi, uint32_t cnt, uint32_t keep_root,
                                             bool in_place, AdvLds& L) {
    const uint4* s4 = (const uint4*)(src + keep_root);  // (a uniform base and 32-bit offsets: ids relative to keep_root)
    uint4* d4 = (uint4*)dst;
    const uint32_t tid = threadIdx.x, units = cnt * NODE_GROUPS, words = (hi - keep_root + 63u) / 64u;
    const uint32_t full = cnt / ADV_CHUNK_NODES;  // whole chunks; the rest, if any, is chunk `full`
    auto fill = [&](uint32_t c) {
        const uint32_t from_word = c == 0 ? 0u : (uint32_t)L.list[(c - 1u) & 1u][ADV_CHUNK_NODES - 1] >> 6;
        adv_fill_list(L.bits, L.before, words, cnt, c * ADV_CHUNK_NODES, from_word, tid, ADV_THREADS, L.list[c & 1u]);
    };
    // Every thread issues ADV_UNITS loads per chunk, and ADV_UNITS stores per whole chunk, on no condition (adv_chunk_unit):
    // the compiler then knows how many are outstanding and waits for a chunk with a counted vmcnt that leaves the later
    // ones in flight (behind a branch it would have to wait for all).
    auto load = [&](uint32_t c, uint4* v) {
#pragma unroll
        for (uint32_t k = 0; k < ADV_UNITS; ++k) {
            const AdvUnit x = adv_chunk_unit(c, k, tid, units);
            v[k] = s4[adv_unit_source(x, L.list[c & 1u][adv_unit_node(x.j)])];
        }
    };
    auto store = [&](uint32_t c, uint4* v, bool whole) {
#pragma unroll
        for (uint32_t k = 0; k < ADV_UNITS; ++k) {
            const AdvUnit x = adv_chunk_unit(c, k, tid, units);
            if (adv_id_words(adv_unit_group(x.j)) != 0) {
                uint32_t w[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
                adv_remap_unit(w, adv_unit_group(x.j), x.u < NODE_GROUPS,
                               [&](uint32_t old) { return adv_new_id(L.bits, L.before, old - keep_root); });
                v[k] = make_uint4(w[0], w[1], w[2], w[3]);
            }
            if (adv_unit_stored(x, whole)) (d4 + (size_t)c * ADV_CHUNK_UNITS)[x.j] = v[k];
        }
    };
    auto arrived = [&](uint4* v) {
        if (in_place) {
#pragma unroll
            for (uint32_t k = 0; k < ADV_UNITS; ++k) adv_arrived(v[k]);
        }
    };
    uint4 v[ADV_DEPTH][ADV_UNITS];
    fill(0);
    __syncthreads();
#pragma unroll
    for (uint32_t s = 1; s < ADV_DEPTH; ++s) {
        load(s - 1, v[s - 1]);
        fill(s);
        __syncthreads();
    }
    for (uint32_t c0 = 0; c0 < full; c0 += ADV_DEPTH) {
#pragma unroll
        for (uint32_t s = 0; s < ADV_DEPTH; ++s) {
            const uint32_t c = c0 + s;  // (adv_chunk_buffer(c) = s: c0 is a multiple of ADV_DEPTH)
            if (c >= full) break;
            load(c + ADV_DEPTH - 1, v[(s + ADV_DEPTH - 1) % ADV_DEPTH]);
            fill(c + ADV_DEPTH);
            arrived(v[s]);
            __syncthreads();
            store(c, v[s], true);
        }
    }
    if (cnt % ADV_CHUNK_NODES != 0) {  // the rest: its loads were issued ADV_DEPTH - 1 steps ago, like any chunk's
#pragma unroll
        for (uint32_t s = 0; s < ADV_DEPTH; ++s)
            if (adv_chunk_buffer(full) == s) {
                arrived(v[s]);
                __syncthreads();
                store(full, v[s], false);
            }
    }
}

// ---- slow path: new ids in fwd[] (global memory), any hi ----------------------------------------------------------------
// the recurrence by the first wavefront; fwd[i] for i >= keep_root is written (nothing reads the entries below).
// All threads call it; returns the number of kept nodes (to all), with fwd[] visible to the whole block.
__device__ inline uint32_t adv_mark_fwd(const NodeStats* src, uint32_t* fwd, uint32_t hi, uint32_t keep_root, AdvLds& L) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (tid < 64) {
        uint32_t cnt = 0;
        for (uint32_t base = keep_root & ~63u; base < hi; base += 64) {
            const uint32_t i = base + lane;
            uint32_t st = 2, p = NIL;  // 0 unknown, 1 keep, 2 drop
            if (i < hi) {
                if (i == keep_root) st = 1;
                else if (i > keep_root) {
                    p = src[i].h1.parent;
                    if (p == NIL || p < keep_root) st = 2;
                    else if (p < base)
                        st = __hip_atomic_load(&fwd[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != NIL ? 1u : 2u;
                    else st = 0;
                }
            }
            for (int round = 0; round < 64; ++round) {
                const uint32_t from = (st == 0) ? (p - base) : lane;
                const uint32_t pst = (uint32_t)__shfl((int)st, (int)from, 64);
                if (st == 0 && pst != 0) st = pst;
                if (!__any(st == 0)) break;
            }
            const bool keep = st == 1;
            const unsigned long long bal = __ballot(keep);
            const uint32_t before = (uint32_t)__popcll(bal & ((1ULL << lane) - 1ULL));
            if (i >= keep_root && i < hi)
                __hip_atomic_store(&fwd[i], keep ? cnt + before : NIL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            cnt += (uint32_t)__popcll(bal);
            // the next group's lanes read this group's new ids: the stores must have left the wavefront (one CU:
            // workgroup scope is enough, and an agent-scope fence would write back the XCD's whole L2)
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        }
        if (tid == 0) L.cnt = cnt;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    return L.cnt;
}
// the move: 25 old nodes per step, twenty lanes a node; a dropped node's lanes idle. Steps go in old-id order with
// every load of a step returned before its stores (both ways, as the destination may be the source): new id <= old id,
// so a step's stores land at or below the nodes it has read, and below every node a later step reads.
__device__ inline void adv_move_fwd(const NodeStats* src, NodeStats* dst, const uint32_t* fwd, uint32_t hi, uint32_t keep_root) {
    const uint4* s4 = (const uint4*)src;
    uint4* d4 = (uint4*)dst;
    const uint32_t tid = threadIdx.x, sub = tid / NODE_GROUPS, g = tid % NODE_GROUPS;
    for (uint32_t i0 = keep_root; i0 < hi; i0 += ADV_SLOW_NODES) {
        const uint32_t i = i0 + sub;
        uint32_t ni = NIL;
        if (sub < (uint32_t)ADV_SLOW_NODES && i < hi) ni = __hip_atomic_load(&fwd[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        uint4 v = make_uint4(0, 0, 0, 0);
        if (ni != NIL) {
            v = s4[(size_t)i * NODE_GROUPS + g];
            if (adv_id_words(g) != 0) {
                uint32_t w[4] = {v.x, v.y, v.z, v.w};
                adv_remap_unit(w, g, i == keep_root, [&](uint32_t old) {
                    return __hip_atomic_load(&fwd[old], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                });
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        adv_arrived(v);
        __syncthreads();
        if (ni != NIL) d4[(size_t)ni * NODE_GROUPS + g] = v;
    }
}

// The compaction of one tree by a block of ADV_THREADS threads. fast_nodes: the largest hi - keep_root that takes the
// fast path (at most ADV_MAX_NODES; 0: always the slow path). pick_dst(cnt) is called by every thread once the kept
// nodes are counted and returns the destination records (uniform over the block; `src` itself: in place).
// Returns the number of kept nodes. 0 < keep_root < hi or keep_root == 0 (nothing to drop) are both fine.
#if defined(AR_STATS)
// wall clock (100 MHz) of the compaction's phases, summed over trees by each block's first thread: [0] trees, [1] mark,
// [2] pick (the caller's claim of a destination), [3] move, [4] sum of hi - keep_root, [5] sum of kept, [6] slow-path trees,
// [8..16) trees by total time / 100 us, [16..22) the same sums as [0..6) over the trees that took more than 300 us
__device__ unsigned long long g_adv_clk[32];
#define ADV_STAT(...) __VA_ARGS__
#else
#define ADV_STAT(...)
#endif

template <class PickDst>
__device__ inline uint32_t advance_compact(const NodeStats* src, uint32_t* fwd, uint32_t hi, uint32_t keep_root,
                                           uint32_t fast_nodes, AdvLds& L, PickDst pick_dst) {
    const uint32_t n = hi - keep_root;
    const bool fast = n <= fast_nodes && n <= (uint32_t)ADV_MAX_NODES;
    ADV_STAT(const unsigned long long c0 = wall_clock64();)
    const uint32_t cnt = (uint32_t)__builtin_amdgcn_readfirstlane(  // (the same in every lane: a scalar register)
        (int)(fast ? adv_mark_lds(src, hi, keep_root, L) : adv_mark_fwd(src, fwd, hi, keep_root, L)));
    ADV_STAT(const unsigned long long c1 = wall_clock64();)
    NodeStats* dst = pick_dst(cnt);
    ADV_STAT(const unsigned long long c2 = wall_clock64();)
    if (fast) adv_move_lds(src, dst, hi, cnt, keep_root, dst == src, L);
    else adv_move_fwd(src, dst, fwd, hi, keep_root);
    ADV_STAT(__syncthreads(); if (threadIdx.x == 0) {
        const unsigned long long c3 = wall_clock64();
        const unsigned long long v[7] = {1ULL, c1 - c0, c2 - c1, c3 - c2, n, cnt, fast ? 0ULL : 1ULL};
        for (int k = 0; k < 7; ++k) atomicAdd(&g_adv_clk[k], v[k]);
        const unsigned long long b = (c3 - c0) / 10000ULL;
        atomicAdd(&g_adv_clk[8 + (b < 7 ? b : 7)], 1ULL);
        if (c3 - c0 > 30000ULL)
            for (int k = 0; k < 7; ++k) atomicAdd(&g_adv_clk[16 + k], v[k]);
    })
    return cnt;
}
#endif  // __HIPCC__

}  // namespace ar
