// TEST HARNESS -- the pipelined move of alpharat_amd/csrc/dev_advance.h on the CPU: the per-chunk source lists as the
// kernel's threads fill them (adv_fill_list, every thread of the block, in any order), and the move of a re-rooted tree
// with several chunks in flight under random schedules of the single loads and stores of all threads that keep only the
// two rules the kernel keeps (ap_move). It is NOT a CPU fallback: nothing in alpharat_amd/ loads this file.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>

#include "../../alpharat_amd/csrc/dev_advance.h"

using namespace ar;

namespace {

struct Tables {
    std::vector<unsigned long long> bits;
    std::vector<uint16_t> before;
    uint32_t words = 0, cnt = 0;
};
// what the mark phase leaves in LDS: keep flags by id relative to keep_root, kept nodes in the words below
Tables mark(const uint32_t* src, uint32_t hi, uint32_t keep_root) {
    Tables T;
    const uint32_t n = hi - keep_root;
    T.words = (n + 63) / 64;
    T.bits.assign(T.words, 0ULL);
    T.before.assign(T.words, 0);
    for (uint32_t j = 0; j < n; ++j) {
        if ((j & 63u) == 0) T.before[j >> 6] = (uint16_t)T.cnt;
        bool keep = j == 0;
        if (!keep) {
            const uint32_t p = src[(size_t)(keep_root + j) * 80 + ADV_PARENT_GROUP * 4 + 3];
            keep = p != NIL && p >= keep_root && ((T.bits[(p - keep_root) >> 6] >> ((p - keep_root) & 63u)) & 1ULL);
        }
        if (keep) {
            T.bits[j >> 6] |= 1ULL << (j & 63u);
            T.cnt += 1;
        }
    }
    return T;
}
// chunk by chunk as adv_move_lds does it: chunk c's list in buffer c & 1, started from the word of the last entry of the
// list before; the threads in a shuffled order. Entries no thread wrote stay 0xFFFF.
std::vector<uint16_t> lists(const Tables& T, std::mt19937_64& rng) {
    const uint32_t chunks = (T.cnt + ADV_CHUNK_NODES - 1) / ADV_CHUNK_NODES;
    std::vector<uint16_t> all((size_t)chunks * ADV_CHUNK_NODES, 0xFFFF);
    uint16_t buf[2][ADV_CHUNK_NODES];
    std::vector<uint32_t> tids(ADV_THREADS);
    for (uint32_t t = 0; t < ADV_THREADS; ++t) tids[t] = t;
    for (uint32_t c = 0; c < chunks + 1; ++c) {  // (one past the end: the kernel asks for it, and nothing may be written)
        const uint32_t from_word = c == 0 ? 0u : (uint32_t)buf[(c - 1) & 1][ADV_CHUNK_NODES - 1] >> 6;
        for (uint32_t k = 0; k < ADV_CHUNK_NODES; ++k) buf[c & 1][k] = 0xFFFF;
        std::shuffle(tids.begin(), tids.end(), rng);
        for (uint32_t t : tids)
            adv_fill_list(T.bits.data(), T.before.data(), T.words, T.cnt, c * ADV_CHUNK_NODES, from_word, t, ADV_THREADS, buf[c & 1]);
        if (c < chunks) memcpy(&all[(size_t)c * ADV_CHUNK_NODES], buf[c & 1], sizeof buf[0]);
        else
            for (uint32_t k = 0; k < ADV_CHUNK_NODES; ++k)
                if (buf[c & 1][k] != 0xFFFF) all.clear();  // (reported as a failure)
    }
    return all;
}

}  // namespace

extern "C" {

uint32_t ap_chunk_nodes() { return ADV_CHUNK_NODES; }
uint32_t ap_depth() { return ADV_DEPTH; }

// The source lists of every chunk, concatenated: out[c * ADV_CHUNK_NODES + k], room for chunks * ADV_CHUNK_NODES entries
// (entries past a short last chunk's nodes: 0xFFFF). Returns the kept count, 0xFFFFFFFF if a list past the end was written.
uint32_t ap_lists(const void* src_records, uint32_t hi, uint32_t keep_root, uint16_t* out, uint64_t seed) {
    const Tables T = mark((const uint32_t*)src_records, hi, keep_root);
    std::mt19937_64 rng(seed);
    const std::vector<uint16_t> all = lists(T, rng);
    if (all.empty()) return 0xFFFFFFFFu;
    memcpy(out, all.data(), all.size() * sizeof(uint16_t));
    return T.cnt;
}

// The move with `depth` chunks in flight. Every thread's every unit of every chunk, as adv_chunk_unit hands them out (the
// repeated last units of a chunk and the units past the tree included), is a load event, and a store event where
// adv_unit_stored says so; where a unit is loaded from is adv_unit_source's word. The events of all threads and chunks
// happen in a random order under two rules only:
//   1. every load of chunk c (of every thread) comes before every store of chunk c (the barrier) -- and of every later
//      chunk, as a block passes its barriers in order: chunk c + 1's first kept node may be the source of chunk c's last,
//   2. a thread's loads of chunk c + depth do not start before its stores of chunk c have finished (it needs the registers:
//      buffer adv_chunk_buffer(c) when depth is the header's; held per thread, this allows every order the same rule over
//      the whole block allows, and more).
// A load reads the records as they are at that moment. mode 0: any enabled event; 1: loads whenever one is enabled (as much
// in flight as the rules allow); 2: stores whenever one is enabled. src == dst: in place. Returns the kept count.
uint32_t ap_move(void* src_records, void* dst_records, uint32_t hi, uint32_t keep_root, uint32_t depth, int mode, uint64_t seed) {
    const uint32_t* src = (const uint32_t*)src_records;
    uint32_t* dst = (uint32_t*)dst_records;
    const Tables T = mark(src, hi, keep_root);
    std::mt19937_64 rng(seed);
    const std::vector<uint16_t> all = lists(T, rng);
    if (all.empty() || depth == 0) return 0xFFFFFFFFu;
    const uint32_t units = T.cnt * NODE_GROUPS, chunks = (T.cnt + ADV_CHUNK_NODES - 1) / ADV_CHUNK_NODES;
    const uint32_t full = T.cnt / ADV_CHUNK_NODES;  // whole chunks, as adv_move_lds counts them
    struct Ev {
        uint32_t tid, c, k;  // thread, chunk, which of the thread's units
    };
    const size_t per_chunk = (size_t)ADV_THREADS * ADV_UNITS;
    auto slot_of = [&](const Ev& e) { return ((size_t)e.c * per_chunk + (size_t)e.k * ADV_THREADS + e.tid) * 4; };
    std::vector<Ev> loads, stores;  // the enabled ones
    std::vector<uint32_t> chunk_loads_left(chunks, (uint32_t)per_chunk);
    std::vector<uint32_t> held((size_t)chunks * per_chunk * 4);  // a thread's registers, by (chunk, unit, thread)
    if (depth == (uint32_t)ADV_DEPTH)  // (the header's rotation: chunks c and c + depth share a buffer, no two in between do)
        for (uint32_t c = 0; c + 1 < chunks; ++c)
            if ((adv_chunk_buffer(c + depth) != adv_chunk_buffer(c)) || (depth > 1 && adv_chunk_buffer(c + 1) == adv_chunk_buffer(c)))
                return 0xFFFFFFFDu;
    // a thread may load chunk c once its stores of chunk c - depth are done
    std::vector<std::vector<uint32_t>> stores_left(ADV_THREADS, std::vector<uint32_t>(chunks, 0));
    for (uint32_t c = 0; c < chunks; ++c)
        for (uint32_t k = 0; k < ADV_UNITS; ++k)
            for (uint32_t tid = 0; tid < ADV_THREADS; ++tid)
                if (adv_unit_stored(adv_chunk_unit(c, k, tid, units), c < full)) stores_left[tid][c] += 1;
    std::vector<uint32_t> next_load(ADV_THREADS, 0);  // first chunk whose loads are not enabled yet
    auto advance_thread = [&](uint32_t tid) {
        while (next_load[tid] < chunks) {
            const uint32_t c = next_load[tid];
            if (c >= depth && stores_left[tid][c - depth] != 0) break;
            for (uint32_t k = 0; k < ADV_UNITS; ++k) loads.push_back(Ev{tid, c, k});
            next_load[tid] += 1;
        }
    };
    for (uint32_t tid = 0; tid < ADV_THREADS; ++tid) advance_thread(tid);
    auto take = [&](std::vector<Ev>& v) {
        const size_t i = (size_t)(rng() % v.size());
        const Ev e = v[i];
        v[i] = v.back();
        v.pop_back();
        return e;
    };
    uint32_t barriers = 0;  // chunks whose barrier the block has passed
    while (!loads.empty() || !stores.empty()) {
        bool do_load;
        if (loads.empty()) do_load = false;
        else if (stores.empty()) do_load = true;
        else if (mode == 1) do_load = true;
        else if (mode == 2) do_load = false;
        else do_load = rng() % (loads.size() + stores.size()) < loads.size();
        if (do_load) {
            const Ev e = take(loads);
            const AdvUnit x = adv_chunk_unit(e.c, e.k, e.tid, units);
            const uint32_t entry = all[(size_t)e.c * ADV_CHUNK_NODES + adv_unit_node(x.j)];  // (0xFFFF past the tree)
            const size_t from = (size_t)keep_root * NODE_GROUPS + adv_unit_source(x, entry);
            if (from >= (size_t)hi * NODE_GROUPS) return 0xFFFFFFFCu;  // (a load outside the tree's records)
            memcpy(&held[slot_of(e)], src + from * 4, 16);
            chunk_loads_left[e.c] -= 1;
            for (; barriers < chunks && chunk_loads_left[barriers] == 0; ++barriers)
                for (uint32_t k = 0; k < ADV_UNITS; ++k)
                    for (uint32_t tid = 0; tid < ADV_THREADS; ++tid)
                        if (adv_unit_stored(adv_chunk_unit(barriers, k, tid, units), barriers < full)) stores.push_back(Ev{tid, barriers, k});
        } else {
            const Ev e = take(stores);
            const AdvUnit x = adv_chunk_unit(e.c, e.k, e.tid, units);
            if (x.u >= units) return 0xFFFFFFFBu;  // (a store past the kept records)
            uint32_t* w = &held[slot_of(e)];
            adv_remap_unit(w, adv_unit_group(x.j), x.u < NODE_GROUPS,
                           [&](uint32_t old) { return adv_new_id(T.bits.data(), T.before.data(), old - keep_root); });
            memcpy(dst + (size_t)x.u * 4, w, 16);
            if (--stores_left[e.tid][e.c] == 0) advance_thread(e.tid);
        }
    }
    for (uint32_t c = 0; c < chunks; ++c)
        if (chunk_loads_left[c] != 0) return 0xFFFFFFFEu;  // (the schedule got stuck: a bug of the harness)
    return T.cnt;
}

}  // extern "C"
