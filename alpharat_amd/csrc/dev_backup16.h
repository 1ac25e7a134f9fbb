// The backup (search.rs:1027-1066: populate / finalize the gathered leaves, walk the values up, cancel the
// collisions) with SIXTEEN LANES PER GAME: lane w of a group takes batch entry w, a wavefront holds four games.
//
// The lane-per-game backup (backup_round, dev_search.h) is one dependent memory trip per tree level per entry:
// ~16 entries x ~10 levels = ~170 trips per batch in sequence, and nothing else to run meanwhile. Entries cannot
// simply be walked at the same time: paths share their upper part, and a shared node's running means must take the
// entries' values in batch order (f32 Welford updates do not commute). But the value an entry delivers to a node does
// not depend on any node's statistics: it is q = r + q', q' what the entry delivered one level below and r the static
// edge reward of the node below (NodeH1::r1/r2); at the leaf it is the evaluator's output, or 0 for a terminal. So
// every q of every (entry, level) is known once the path is, the nodes are independent of each other, and a node is
// read once, given all its entries' updates in batch order in registers, and written once:
//   1. every lane follows the parent links of its own entry from the leaf to the root and notes per level, in LDS,
//      the step (node, which outcome pair of it leads down) and the pair (q1, q2) the entry delivers there -- reads
//      only, all entries at once: depth trips. Level 0 is the leaf (populate_node + first finalize), so a terminal
//      node that was claimed twice in one batch is served in order like any shared node;
//   2. a node belongs to the lowest lane whose path has it. Two paths that share a node have it at the same depth
//      from the root and share everything above it, so a lane's own nodes are the levels of its path below the longest
//      prefix it shares with a lower lane (bk16_claim: LDS reads only). The own levels of lane 0, 1, ... in turn are
//      the list of the game's distinct nodes; item t of it is served by lane t % 16 -- the shared upper part of the
//      paths, which all belongs to lane 0, is spread over the group, and a lane has two or three items, not a whole
//      path. Serving a node: find the entries that have it (sixteen LDS reads at its depth), load the header and the
//      edges, apply finalize_score_update / update_multivisit of every such entry in entry order, exactly as
//      backup_round does, store what changed. There is no fence inside the phase;
//   3. collisions only subtract integers from in-flight counters (search.rs:860-889: a record's count comes off every
//      ancestor of its node and off the two edges that lead down to it), and a record is only ever written for a node
//      that is the leaf of an entry of the same batch (claimed at that moment, or claimed earlier in the batch and not
//      yet visited: gw_visit, emit_coll's callers). So the record's way up is a path phase 1 has noted, and the three
//      counters it meets at an ancestor are the header and the two edges phase 2 updates there for that entry. Between
//      1 and 2 the lanes take the records sixteen at a time (the first two of a lane are loaded before the walk), find
//      the lowest lane of the chunk whose leaf the record's node is (sixteen LDS compares) and add the count to that
//      lane's total cm (bk16_fold); bk16_settle takes cm off after that entry's update of an ancestor, the leaf itself
//      left alone. In-flight counts feed no float, so the subtraction commutes with everything else done to the node:
//      the same bytes as the walk, no memory trip, no atomic, no barrier of its own. A record is folded in the first
//      chunk that has its leaf and never again (a bit per record and lane); what no chunk takes -- a record without a
//      node, on the leaf of an entry dropped with error 6, on a node that is no noted leaf, or beyond the 512th of a
//      batch -- is walked up with atomic subtractions behind the last chunk (bk16_cancel_left), by the wavefronts that
//      have one: in a regular batch none.
// Levels are numbered from the leaf, so of a path longer than PATH_LDS_STEPS it is the root side that lives in scratch:
// the lanes' scans at those depths are global loads (cached: sixteen lanes read the same few words). Searches with the
// shipped constants stay near ten levels; tests/test_gpu_backup_merge.py has paths of forty.
// A path longer than path_cap (never met: the cap is beyond the turn limit) flags the game with error 6 and drops that
// entry alone; the other entries and later chunks are served (the pipeline this replaces stopped the lane for good).
// Same arithmetic, same order per node as backup_round: trees are bit-identical. 1, 2 and 3 are host-callable per lane
// (bk16_walk, bk16_fold, bk16_claim, bk16_apply, bk16_cancel_left: lanes meet only through the notes), and
// tests/hostsim_backup runs them on the CPU with the lanes in ascending and in descending order against the
// entry-by-entry walk and the plain cancel walk. End-of-batch bookkeeping (batch_end)
// is done by lane 0; the end of a move (extraction, sampling, record, step: finish_move) is left to k_finish.
#pragma once
#include "dev_search.h"

namespace ar {

// one step of a path: node id (26 bits) | outcome pair of THIS node that leads to the level below (p1 3 bits, p2 3 bits)
typedef uint32_t PathStep;
// levels kept in LDS per lane; deeper ones go to the game's (idle) level-stack scratch. Twelve levels are 9.5 KB a
// wavefront (9.75 KB with the heads, cuts and collision totals; LDS is dealt in 1.25 KB steps, so 10 KB either way):
// sixteen wavefronts a CU, which the 128 registers of the kernel allow too (twenty would be ten)
enum { PATH_LDS_STEPS = 12 };
enum { PATH_NODE_MASK = 0x3FFFFFF, PATH_LANES = 16 };
AR_HD PathStep path_pack(uint32_t node, uint32_t o1, uint32_t o2) { return node | (o1 << 26) | (o2 << 29); }

// a level beyond PATH_LDS_STEPS, in scratch
struct PathNote {
    PathStep step;
    float q1, q2;
};
// bytes of level-stack scratch the deep levels of a game's sixteen paths take (path_cap = max_depth + 2 levels each)
AR_HD size_t backup16_deep_bytes(uint32_t max_depth) {
    const uint32_t cap = max_depth + 2;
    return cap > PATH_LDS_STEPS ? (size_t)PATH_LANES * (cap - PATH_LDS_STEPS) * sizeof(PathNote) : 0;
}

// what a lane says about its entry: path length (0: no entry) | the leaf is evaluated << 18 | where the evaluator put
// its outputs << 19
enum { HEAD_LEN_BITS = 18 };
AR_HD uint32_t head_pack(uint32_t len, uint32_t entry_word) {
    return len | (proc_kind(entry_word) == PROC_EVAL ? (1u << HEAD_LEN_BITS) | (proc_eval_index(entry_word) << (HEAD_LEN_BITS + 1)) : 0u);
}
AR_HD uint32_t head_len(uint32_t h) { return h & ((1u << HEAD_LEN_BITS) - 1u); }
AR_HD bool head_is_eval(uint32_t h) { return (h >> HEAD_LEN_BITS) & 1u; }
AR_HD uint32_t head_eval_index(uint32_t h) { return h >> (HEAD_LEN_BITS + 1); }
static_assert(HEAD_LEN_BITS + 1 + PROC_INDEX_BITS <= 32, "a head word is length | evaluated | evaluation index");

// The notes of one game's sixteen paths. Level l of lane j is step[l * stride + j] (likewise q1, q2) below
// PATH_LDS_STEPS and deep[j * deep_cap + l - PATH_LDS_STEPS] from there on; level 0 is the leaf.
struct PathNotes {
    PathStep* step;
    float* q1;
    float* q2;
    uint32_t* head;  // [16]
    uint32_t* cut;   // [16] first level (from the root) no lower lane has: bk16_claim
    PathNote* deep;
    uint32_t stride, deep_cap;
    uint32_t* cm = nullptr;  // [16] collision total to cancel along the lane's path: bk16_fold (null: no totals)
};
AR_HD PathStep note_step(const PathNotes& P, uint32_t j, uint32_t l) {
    return l < PATH_LDS_STEPS ? P.step[l * P.stride + j] : P.deep[(size_t)j * P.deep_cap + (l - PATH_LDS_STEPS)].step;
}
AR_HD void note_get(const PathNotes& P, uint32_t j, uint32_t l, PathStep& s, float& q1, float& q2) {
    if (l < PATH_LDS_STEPS) {
        s = P.step[l * P.stride + j];
        q1 = P.q1[l * P.stride + j];
        q2 = P.q2[l * P.stride + j];
    } else {
        const PathNote n = P.deep[(size_t)j * P.deep_cap + (l - PATH_LDS_STEPS)];
        s = n.step;
        q1 = n.q1;
        q2 = n.q2;
    }
}
AR_HD void note_put(const PathNotes& P, uint32_t j, uint32_t l, PathStep s, float q1, float q2) {
    if (l < PATH_LDS_STEPS) {
        P.step[l * P.stride + j] = s;
        P.q1[l * P.stride + j] = q1;
        P.q2[l * P.stride + j] = q2;
    } else {
        PathNote n;
        n.step = s;
        n.q1 = q1;
        n.q2 = q2;
        P.deep[(size_t)j * P.deep_cap + (l - PATH_LDS_STEPS)] = n;
    }
}

// ---- 1. lane w notes the path of its entry (leaf `leaf`, entry word `entry_word`; `mine` = the lane has an entry).
// Returns the error code (6: the path is longer than path_cap; the entry then takes no part in the backup).
AR_HD uint32_t bk16_walk(const PathNotes& P, uint32_t w, bool mine, uint32_t leaf, uint32_t entry_word,
                         const NodeStats* stats, const EvalOut* ev, uint32_t path_cap) {
    uint32_t D = 0, err = 0;
    if (mine) {
        // what the leaf takes: the evaluator's values, or zeros (its read does not wait for the walk)
        float q1 = 0.0f, q2 = 0.0f;
        if (proc_kind(entry_word) == PROC_EVAL) {
            const EvalOut& o = ev[proc_eval_index(entry_word)];
            q1 = o.v1;
            q2 = o.v2;
        }
        uint32_t cur = leaf, po = 0;
        while (true) {
            if (D >= path_cap) {
                err = 6;
                D = 0;
                break;
            }
            const NodeH1 h = stats[cur].h1;
            const uint32_t meta = stats[cur].h2.meta;
            note_put(P, w, D, path_pack(cur, po & 7u, po >> 3), q1, q2);
            D += 1;
            // one level up (backup_round B_LEVEL): the edge rewards of the level below plus the value carried up
            q1 = h.r1 + q1;
            q2 = h.r2 + q2;
            po = meta_po(meta, 0) | (meta_po(meta, 1) << 3);
            cur = h.parent;
            if (cur == NIL) break;
        }
    }
    P.head[w] = head_pack(D, entry_word);
    return err;
}

// ---- 2. a node in the registers of the lane that serves it
struct OwnedNode {
    uint32_t same;  // lanes whose path has the node (at the same depth from the root, all of them)
    uint32_t node;
    NodeH0 h0;
    Edge e[2][5];  // loaded where an entry changes them (not for a node that is only a terminal leaf here)
};
// what populate_node needs of an evaluated leaf
struct LeafEval {
    uint32_t omap[2];
    float p1[5], p2[5];
};
AR_HD LeafEval leaf_eval(const NodeStats& N, const EvalOut& o) {
    LeafEval r;
    const NodeH2 c = N.h2;
    r.omap[0] = c.omap[0];
    r.omap[1] = c.omap[1];
    for (int i = 0; i < 5; ++i) {
        r.p1[i] = o.p1[i];
        r.p2[i] = o.p2[i];
    }
    return r;
}

// the three fields of edge `a` an update changes, as ORs over masked elements (sel5u, dev_search.h)
AR_HD Edge edge_pick(const Edge* e, uint32_t a) {
    uint32_t q = 0, v = 0, n = 0;
#pragma unroll
    for (uint32_t i = 0; i < 5; ++i) {
        q |= (a == i) ? f32_to_bits(e[i].q) : 0u;
        v |= (a == i) ? e[i].visits : 0u;
        n |= (a == i) ? e[i].nif : 0u;
    }
    Edge r;
    r.prior = 0.0f;
    r.q = bits_to_f32(q);
    r.visits = v;
    r.nif = n;
    return r;
}
AR_HD void edge_place(Edge* e, uint32_t a, const Edge& r) {
#pragma unroll
    for (uint32_t i = 0; i < 5; ++i) {
        e[i].q = (a == i) ? r.q : e[i].q;
        e[i].visits = (a == i) ? r.visits : e[i].visits;
        e[i].nif = (a == i) ? r.nif : e[i].nif;
    }
}

// The node gets the update of every entry that has it, in entry order, and is stored. Returns the number of updates.
// `k` = the node's depth from the root, `le` = what lane `first_eval`'s evaluated leaf needs, if the node is one.
AR_HD uint32_t bk16_settle(const PathNotes& P, uint32_t first_eval, uint32_t k, NodeStats* stats, const EvalOut* ev,
                           const LeafEval& le0, OwnedNode& n) {
    NodeStats& N = stats[n.node];
    uint32_t nv = 0, dirty = 0;  // bit pl * 5 + i: edge record to store
    for (uint32_t left = n.same; left; left &= left - 1u) {
        const uint32_t j = (uint32_t)lowest_bit(left), hj = P.head[j], l = head_len(hj) - 1 - k;
        PathStep ps;
        float q1, q2;
        note_get(P, j, l, ps, q1, q2);
        if (l == 0) {
            // the gathered leaf: populate_node (tree.rs:156-173) + first finalize (backup_round B_ENTRY)
            if (head_is_eval(hj)) {
                LeafEval le = le0;
                if (j != first_eval) le = leaf_eval(N, ev[head_eval_index(hj)]);  // (an evaluated leaf has one entry: not met)
                float red1[5], red2[5];
                reduce_prior(le.omap[0], le.p1, red1);
                reduce_prior(le.omap[1], le.p2, red2);
                for (int i = 0; i < 5; ++i) {
                    n.e[0][i].prior = red1[i];
                    n.e[1][i].prior = red2[i];
                }
                dirty = 0x3FFu;
            }
            finalize_h0(n.h0, q1, q2, 1);
        } else {
            // one ancestor (backup_round B_LEVEL, search.rs:834-851)
            const uint32_t a1 = (ps >> 26) & 7u, a2 = ps >> 29;
            Edge e1 = edge_pick(n.e[0], a1), e2 = edge_pick(n.e[1], a2);
            finalize_h0(n.h0, q1, q2, 1);
            edge_update(e1, q1, 1);
            edge_update(e2, q2, 1);
            // the collisions on this entry's leaf (search.rs:860-889): the three counters their walk would meet here
            const uint32_t cmj = P.cm ? P.cm[j] : 0u;
            n.h0.nif -= cmj;
            e1.nif -= cmj;
            e2.nif -= cmj;
            edge_place(n.e[0], a1, e1);
            edge_place(n.e[1], a2, e2);
            dirty |= (1u << a1) | (32u << a2);
        }
        nv += 1;
    }
    N.h0 = n.h0;
    for (int pl = 0; pl < 2; ++pl)
        for (int i = 0; i < 5; ++i)
            if ((dirty >> (pl * 5 + i)) & 1u) N.e[pl][i] = n.e[pl][i];
    return nv;
}

// ---- 2a. lane w finds the levels of its path that are its own: those no lower lane has. Two paths that share a node
// share everything above it, so these are the depths from `cut` on, cut = the longest prefix shared with a lower lane.
AR_HD void bk16_claim(const PathNotes& P, uint32_t w) {
    const uint32_t D = head_len(P.head[w]);
    uint32_t c = 0;
    for (uint32_t j = 0; j < w && c < D;) {
        const uint32_t Dj = head_len(P.head[j]);
        if (Dj > c && ((note_step(P, j, Dj - 1 - c) ^ note_step(P, w, D - 1 - c)) & PATH_NODE_MASK) == 0)
            c += 1;  // lane j has the node at depth c too
        else
            j += 1;
    }
    P.cut[w] = c;
}

// ---- 2b. The game's distinct nodes are lane 0's own levels, then lane 1's, ...: item t of that list is served by
// lane t % 16, whoever's path it is on, so the long shared prefix of lane 0 is spread over the group. A lane takes its
// items one after the other: who has the node (sixteen LDS reads), load, every entry's update in entry order, store.
// Every lane's notes and cuts must be complete. Returns the number of (entry, level) updates the lane applied.
AR_HD uint32_t bk16_apply(const PathNotes& P, uint32_t x, NodeStats* stats, const EvalOut* ev) {
    uint32_t nv = 0;
    for (uint32_t t = x;; t += PATH_LANES) {
        // item t: level k (from the root) of lane w's path
        uint32_t off = 0, w = PATH_LANES, k = 0, Dw = 0;
#pragma unroll 4
        for (uint32_t j = 0; j < PATH_LANES; ++j) {
            const uint32_t Dj = head_len(P.head[j]), cj = P.cut[j];
            if (w == PATH_LANES && t < off + (Dj - cj)) {
                w = j;
                k = cj + (t - off);
                Dw = Dj;
            }
            off += Dj - cj;
        }
        if (w == PATH_LANES) break;
        OwnedNode n;
        n.node = note_step(P, w, Dw - 1 - k) & PATH_NODE_MASK;
        uint32_t same = 0, terminal_leaves = 0, first_eval = PATH_LANES;
#pragma unroll 4
        for (uint32_t j = 0; j < PATH_LANES; ++j) {
            const uint32_t hj = P.head[j], Dj = head_len(hj);
            if (Dj > k && (note_step(P, j, Dj - 1 - k) & PATH_NODE_MASK) == n.node) {
                same |= 1u << j;
                if (Dj - 1 == k) {
                    if (!head_is_eval(hj)) terminal_leaves |= 1u << j;
                    else if (first_eval == PATH_LANES) first_eval = j;
                }
            }
        }
        n.same = same;
        NodeStats& N = stats[n.node];
        n.h0 = N.h0;
        if (same != terminal_leaves)
            for (int pl = 0; pl < 2; ++pl)
                for (int i = 0; i < 5; ++i) n.e[pl][i] = N.e[pl][i];
        LeafEval le = {};
        if (first_eval != PATH_LANES) le = leaf_eval(N, ev[head_eval_index(P.head[first_eval])]);
        nv += bk16_settle(P, first_eval, k, stats, ev, le, n);
    }
    return nv;
}

// ---- 3. collisions. A record (node, mv) asks for mv to be taken off the in-flight counters of every ancestor of `node`
// and of the edges that lead down to it. The node of a record is the leaf of an entry of the same batch, so that path
// is in the notes: the record's count goes to the lowest lane of the chunk whose leaf it is (cm, an LDS add), and
// bk16_settle takes cm off while it has each ancestor in registers. Lane w has records w, 16 + w, ...; bit g of
// `left` = record 16 g + w is still to be cancelled (the first 512 records of a batch: later ones are walked).
AR_HD uint32_t bk16_coll_mask(uint32_t n_coll, uint32_t w) {
    const uint32_t mine = n_coll > w ? (n_coll - w + PATH_LANES - 1) / PATH_LANES : 0u;
    return mine >= 32u ? ~0u : (1u << mine) - 1u;
}
AR_HD bool bk16_fold_one(const PathNotes& P, CollEntry ce) {
    uint32_t j = PATH_LANES;
#pragma unroll 4
    for (uint32_t i = PATH_LANES; i-- > 0;)  // (an entry dropped with error 6 has no length and notes no leaf)
        if (head_len(P.head[i]) != 0 && (note_step(P, i, 0) & PATH_NODE_MASK) == ce.node) j = i;
    if (j == PATH_LANES) return false;
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(&P.cm[j], ce.mv);
#else
    P.cm[j] += ce.mv;
#endif
    return true;
}
// Lane w folds what it can of its records into this chunk's totals and returns what is left. Every lane's notes must be
// complete and cm zeroed before the first lane folds; `c0`, `c1` = the lane's first two records (read before the walk).
AR_HD uint32_t bk16_fold(const PathNotes& P, uint32_t w, const CollEntry* coll, uint32_t left, CollEntry c0, CollEntry c1) {
    if (P.cm == nullptr) return left;
    if ((left & 1u) && bk16_fold_one(P, c0)) left &= ~1u;
    if ((left & 2u) && bk16_fold_one(P, c1)) left &= ~2u;
    for (uint32_t g = 2; g < 32u && (left >> g) != 0; ++g)
        if (((left >> g) & 1u) && bk16_fold_one(P, coll[g * PATH_LANES + w])) left &= ~(1u << g);
    return left;
}
// What no chunk folded (a record without a node, on the leaf of a dropped entry, on a node that is no entry's leaf, or
// past the 512th) is walked up with subtractions, atomic on the device, after all the updates are stored. Returns the
// number of records walked (`steps`, if given, takes the number of levels).
AR_HD uint32_t bk16_cancel_left(uint32_t w, const CollEntry* coll, uint32_t n_coll, uint32_t left, NodeStats* stats,
                                uint32_t* steps = nullptr) {
    uint32_t walked = 0;
    for (uint32_t g = 0; g * PATH_LANES + w < n_coll; ++g) {
        if (g < 32u && !((left >> g) & 1u)) continue;
        const CollEntry ce = coll[g * PATH_LANES + w];
        if (ce.node == NIL) continue;
        walked += 1;
        for (uint32_t cur = ce.node;;) {
            const NodeH1 h = stats[cur].h1;
            const NodeH2 c = stats[cur].h2;
            if (h.parent == NIL) break;
            NodeStats& Q = stats[h.parent];
#if defined(__HIP_DEVICE_COMPILE__)
            atomicSub(&Q.h0.nif, ce.mv);
            atomicSub(&Q.e[0][meta_po(c.meta, 0)].nif, ce.mv);
            atomicSub(&Q.e[1][meta_po(c.meta, 1)].nif, ce.mv);
#else
            Q.h0.nif -= ce.mv;
            Q.e[0][meta_po(c.meta, 0)].nif -= ce.mv;
            Q.e[1][meta_po(c.meta, 1)].nif -= ce.mv;
#endif
            cur = h.parent;
            if (steps) *steps += 1;
        }
    }
    return walked;
}

}  // namespace ar

#if defined(__HIPCC__)
namespace ar {

__device__ inline uint32_t grp_pick(uint32_t v, uint32_t w) {  // value of group lane `w` (16 lanes per game)
    return (uint32_t)__shfl((int)v, (int)((threadIdx.x & 48u) | w), 64);
}
// LDS of a wavefront: step, q1, q2 [PATH_LDS_STEPS][64], one head word, one cut and one collision total per lane
enum { BACKUP16_LDS_BYTES = (3 * PATH_LDS_STEPS + 3) * 64 * 4 };

#if defined(AR_STATS)
// tools/bk16_stats.py. [0] wavefronts; 100 MHz clocks of a wavefront in [1] entries and sort, [2] walk, [3] claim + apply,
// [4] collisions, [5] all of backup16(); [6] batches, [7] collision records, [8] chunks, [9] records whose node is the
// leaf of an entry of a chunk, [10] records with node NIL, [11] (record, level) steps of the atomic walks (three
// atomics each), [12] rounds of the walk loop (a wavefront's trips in sequence), [13] deepest path of a wavefront's
// chunk, summed over [14] chunks of wavefronts, [15] wavefronts that walked at all
__device__ unsigned long long g_bk16_clk[32];
#define BK_STAT(...) __VA_ARGS__
#else
#define BK_STAT(...)
#endif
// the clock since the last mark goes to phase k
#define BK_MARK(k) BK_STAT({ const unsigned long long bs_now = wall_clock64(); bs_clk[k] += bs_now - bs_t; bs_t = bs_now; })

// A batch that evaluates the ROOT (a fresh tree's first batch: one entry) draws Dirichlet noise (search.rs:1036-1050,
// the Gamma sampler is a hundred registers of code): such games are left to the lane-per-game kernel, which the host
// launches behind this one for whatever still has a batch to back up.
template <int NW>
__device__ inline bool backup16_wants(const Slot<NW>& S, const Mem<NW>& m, const SearchCfg& cfg) {
    if (!(cfg.noise_epsilon > 0.0f)) return true;
    const ProcEntry pe = m.proc[0];
    return !(S.n_proc >= 1 && pe.node == S.root && proc_kind(pe.kind) == PROC_EVAL);
}

// One game's batch. `lds` = the wavefront's BACKUP16_LDS_BYTES; all 16 lanes of the group call this together (idle
// groups call it with active = false and only take part in the wave-wide loops' votes and barriers).
template <int NW>
__device__ inline void backup16(bool active, Slot<NW>& S, const Mem<NW>& m, const SearchCfg& cfg, const EvalOut* ev,
                                uint32_t* lds, uint32_t path_cap, uint32_t w) {
    (void)cfg;
    const uint32_t n_proc = active ? S.n_proc : 0u, n_coll = active ? S.n_coll : 0u;
    PathNotes P;
    {
        const uint32_t g0 = threadIdx.x & 48u;  // the game's first lane
        P.step = lds + g0;
        P.q1 = (float*)(lds + PATH_LDS_STEPS * 64 + g0);
        P.q2 = (float*)(lds + 2 * PATH_LDS_STEPS * 64 + g0);
        P.head = lds + 3 * PATH_LDS_STEPS * 64 + g0;
        P.cut = lds + (3 * PATH_LDS_STEPS + 1) * 64 + g0;
        P.cm = lds + (3 * PATH_LDS_STEPS + 2) * 64 + g0;
        P.deep = (PathNote*)m.levels;  // (not in use between gather and gather)
        P.stride = 64;
        P.deep_cap = path_cap > PATH_LDS_STEPS ? path_cap - PATH_LDS_STEPS : 0u;
    }
    uint32_t err = 0;
    uint32_t nv = 0;  // node records updated (the lane kernel's nv_backup)
    BK_STAT(unsigned long long bs_clk[4] = {0, 0, 0, 0}, bs_cnt[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, bs_t = wall_clock64();
            const unsigned long long bs_t0 = bs_t;
            if (active && w == 0) { bs_cnt[0] = 1; bs_cnt[1] = n_coll; })
    uint32_t left = bk16_coll_mask(n_coll, w);  // the lane's collision records no chunk has folded yet
    for (uint32_t base = 0; __any(base < n_proc); base += 16) {
        BK_STAT(if (w == 0 && base < n_proc) bs_cnt[2] += 1;)
        const uint32_t e = base + w;
        const bool mine = e < n_proc;
        // the lane's first two collision records: nothing in the walk waits for them, they arrive under it
        CollEntry c0, c1;
        c0.node = c1.node = NIL;
        c0.mv = c1.mv = 0;
        if (left & 1u) c0 = m.coll[w];
        if (left & 2u) c1 = m.coll[PATH_LANES + w];
        P.cm[w] = 0;
        ProcEntry pe;
        pe.node = NIL;
        pe.kind = proc_none();
        {
            // lane w takes the w-th entry in backup order: rank by key among the chunk's entries (a chunk of the
            // depth-first gathers' entries is in order already; the work-queue gather writes at most 16, in arrival order)
            if (mine) pe = m.proc[e];
            uint32_t rank = 0;
            for (uint32_t j = 0; j < 16; ++j) {
                const uint32_t kj = proc_key(grp_pick(pe.kind, j));
                rank += (kj < proc_key(pe.kind) || (kj == proc_key(pe.kind) && j < w)) ? 1u : 0u;
            }
            uint32_t src = 0;
            for (uint32_t j = 0; j < 16; ++j) src = grp_pick(rank, j) == w ? j : src;
            pe.node = grp_pick(pe.node, src);
            pe.kind = grp_pick(pe.kind, src);
            // (entries without a batch entry sort last: lanes >= n_proc - base get those)
        }
        BK_MARK(0)
        // ---- 1. the path of entry e, noted for all
        err |= bk16_walk(P, w, mine, pe.node, pe.kind, m.stats, ev, path_cap);
        __syncthreads();  // (one wavefront: a wait for the notes, those in scratch included)
        BK_MARK(1)
        BK_STAT({
            uint32_t d = head_len(P.head[w]);
            for (int off = 32; off > 0; off >>= 1) d = max(d, (uint32_t)__shfl_xor((int)d, off, 64));
            if ((threadIdx.x & 63u) == 0) { bs_cnt[7] += d; bs_cnt[8] += 1; }
            bs_t = wall_clock64();
        })
        // ---- 3. a collision record on a leaf of this chunk goes to that lane's total (LDS only; the barrier below
        // orders the adds before phase 2 reads them, the one that ends the chunk orders the reads before the next zero)
        {
            const uint32_t was = left;
            left = bk16_fold(P, w, m.coll, was, c0, c1);
            BK_STAT(bs_cnt[3] += (unsigned long long)__popc(was ^ left);)
        }
        BK_MARK(3)
        // ---- 2. every node once: the lowest lane that has it lists it, the list is dealt round the group
        bk16_claim(P, w);
        __syncthreads();
        nv += bk16_apply(P, w, m.stats, ev);
        // a later chunk reads what this one stored, and phase 3's atomics hit words the stores wrote
        __syncthreads();
        BK_MARK(2)
    }
    // ---- 3, the rest: what no chunk folded is walked up, atomics where paths meet (none at all in a regular batch)
    if (__any(left != 0 || n_coll > 32u * PATH_LANES)) {
        BK_STAT(uint32_t steps = 0;)
        bk16_cancel_left(w, m.coll, n_coll, left, m.stats BK_STAT(, &steps));
        BK_STAT(bs_cnt[5] += steps; if ((threadIdx.x & 63u) == 0) bs_cnt[9] |= 1;
                {
                    uint32_t d = steps;  // (the slowest lane's levels: the wavefront's trips in sequence)
                    for (int off = 32; off > 0; off >>= 1) d = max(d, (uint32_t)__shfl_xor((int)d, off, 64));
                    if ((threadIdx.x & 63u) == 0) bs_cnt[6] += d;
                })
    }
    BK_MARK(3)
    BK_STAT(for (uint32_t g = 0; g * PATH_LANES + w < n_coll; ++g) if (m.coll[g * PATH_LANES + w].node == NIL) bs_cnt[4] += 1;)
    BK_STAT({
        for (int k = 0; k < 10; ++k)
            for (int off = 32; off > 0; off >>= 1) bs_cnt[k] += (unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)bs_cnt[k], off, 64);
        if ((threadIdx.x & 63u) == 0) {
            atomicAdd(&g_bk16_clk[0], 1ULL);
            for (int k = 0; k < 4; ++k) atomicAdd(&g_bk16_clk[1 + k], bs_clk[k]);
            atomicAdd(&g_bk16_clk[5], bs_t - bs_t0);
            for (int k = 0; k < 10; ++k) atomicAdd(&g_bk16_clk[6 + k], bs_cnt[k]);
        }
    })
    // counters: sum over the group's lanes, written by lane 0
    for (int off = 8; off > 0; off >>= 1) {
        nv += (uint32_t)__shfl_xor((int)nv, off, 64);
        err |= (uint32_t)__shfl_xor((int)err, off, 64);
    }
    if (active && w == 0) {
        S.nv_backup += nv;
        if (err) S.error = err;
    }
}

}  // namespace ar
#endif
