// TEST HARNESS -- runs the index logic of alpharat_amd/csrc/dev_advance.h on the CPU: the move of a re-rooted tree unit
// by unit (adv_unit_node / adv_unit_group / adv_id_words / adv_remap_unit / adv_new_id, exactly what a thread of k_advance
// does with one 16-byte group), in chunks whose loads all happen before their stores, in any order within a chunk; and
// advance_tree_scalar of dev_search.h, the statement it has to agree with. It is NOT a CPU fallback: nothing in
// alpharat_amd/ loads this file.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>

#include "../../alpharat_amd/csrc/dev_advance.h"

using namespace ar;

extern "C" {

// advance_tree_scalar in place on `records` ([hi] node records); returns the kept count
uint32_t av_scalar(void* records, uint32_t hi, uint32_t keep_root) {
    std::vector<uint32_t> fwd(hi ? hi : 1);
    Slot<1> s;
    memset(&s, 0, sizeof s);
    s.hi = hi;
    s.pending_root = keep_root;
    Mem<1> m;
    memset(&m, 0, sizeof m);
    m.stats = (NodeStats*)records;
    m.fwd = fwd.data();
    advance_tree_scalar(s, m);
    return s.node_count;
}

// The kernel's steps: keep flags and counts (what its first wavefront leaves in LDS), then the move in units.
// src == dst: in place. order: 0 forward, 1 reversed, 2 shuffled within each chunk of `chunk_units`. Returns the kept count.
uint32_t av_units(void* src_records, void* dst_records, uint32_t hi, uint32_t keep_root, uint32_t chunk_units, int order,
                  uint64_t seed) {
    const uint32_t* src = (const uint32_t*)src_records;
    uint32_t* dst = (uint32_t*)dst_records;
    const uint32_t n = hi - keep_root, words = (n + 63) / 64;
    std::vector<unsigned long long> bits(words, 0ULL);
    std::vector<uint16_t> before(words, 0);
    std::vector<uint32_t> from;  // src[new id] = old id - keep_root (what adv_src_node has to find)
    for (uint32_t j = 0; j < n; ++j) {
        if ((j & 63u) == 0) before[j >> 6] = (uint16_t)from.size();
        bool keep = j == 0;
        if (!keep) {
            const uint32_t p = src[(size_t)(keep_root + j) * 80 + ADV_PARENT_GROUP * 4 + 3];
            keep = p != NIL && p >= keep_root && ((bits[(p - keep_root) >> 6] >> ((p - keep_root) & 63u)) & 1ULL);
        }
        if (keep) {
            bits[j >> 6] |= 1ULL << (j & 63u);
            from.push_back(j);
        }
    }
    const uint32_t cnt = (uint32_t)from.size(), units = cnt * NODE_GROUPS;
    std::mt19937_64 rng(seed);
    struct Held {
        uint32_t u, w[4];
    };
    for (uint32_t c0 = 0; c0 < units; c0 += chunk_units) {
        std::vector<uint32_t> us;
        for (uint32_t u = c0; u < units && u < c0 + chunk_units; ++u) us.push_back(u);
        if (order == 1) std::reverse(us.begin(), us.end());
        if (order == 2) std::shuffle(us.begin(), us.end(), rng);
        std::vector<Held> held;
        for (uint32_t u : us) {  // every load of the chunk
            Held h;
            h.u = u;
            const uint32_t node = adv_unit_node(u), g = adv_unit_group(u);
            // (any word at or below the node's own is a valid place to start from: the first, the right one, one in between)
            const uint32_t right = from[node] >> 6, start = (u % 3 == 0) ? 0u : (u % 3 == 1) ? right : right / 2;
            const uint32_t old = adv_src_node(bits.data(), before.data(), words, node, start);
            if (old != from[node]) return 0xFFFFFFFFu;
            memcpy(h.w, src + (size_t)(keep_root + old) * 80 + g * 4, 16);
            adv_remap_unit(h.w, g, u < NODE_GROUPS,
                           [&](uint32_t old) { return adv_new_id(bits.data(), before.data(), old - keep_root); });
            held.push_back(h);
        }
        if (order == 2) std::shuffle(held.begin(), held.end(), rng);
        for (const Held& h : held) memcpy(dst + (size_t)h.u * 4, h.w, 16);  // then every store
    }
    return cnt;
}

}  // extern "C"
