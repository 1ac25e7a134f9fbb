// TEST HARNESS -- the sixteen-lane backup's per-lane logic (alpharat_amd/csrc/dev_backup16.h: bk16_walk, bk16_claim, bk16_apply)
// on the CPU, as a program of its own (tests/test_backup_merge_cpu.py runs it, once plain and once built with
// -fsanitize=address,undefined). Random small trees built here, depths 1 to 24 (so some paths pass PATH_LDS_STEPS),
// batches of 1, 2, 15, 16, 17 and 33 entries in chunks of sixteen as the kernel takes them: shared prefixes of every
// length, the same terminal leaf twice, an entry whose leaf is the root. The lanes of a chunk run one after the other,
// in ascending and in descending order; the yardstick is the entry-by-entry walk of backup_round (dev_search.h),
// restated below, in batch order. Every node record must come out equal byte for byte, and the update counts equal.
// Exit status 0 and a line "ok: N batches" when that holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../alpharat_amd/csrc/dev_backup16.h"

using namespace ar;

namespace {

struct Rand {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        return (uint32_t)(s >> 33);
    }
    uint32_t below(uint32_t n) { return next() % n; }
    float unit() { return (float)(next() & 0xFFFFFF) / 16777216.0f; }
};

enum { MAX_NODES_DEEP = 24, PATH_CAP = MAX_NODES_DEEP + 2 };

struct Tree {
    std::vector<NodeStats> stats;
    std::vector<uint32_t> depth;  // nodes on the path to the root, the node included
};

uint32_t add_node(Tree& t, Rand& r, uint32_t parent) {
    NodeStats nd;
    memset(&nd, 0, sizeof nd);
    uint32_t eff[2];
    for (int pl = 0; pl < 2; ++pl) {
        eff[pl] = 0;
        for (int a = 0; a < 5; ++a) eff[pl] |= (r.below(3) ? (uint32_t)a : r.below(5)) << (3 * a);
    }
    init_shell(nd, eff[0], eff[1], (uint16_t)(1 + r.below(9)), parent, r.below(5), r.below(5), r.unit() * 2.0f - 0.5f,
               r.below(4) ? 0.0f : 1.0f);
    // a tree in the middle of a search: statistics and in-flight counts everywhere
    for (int pl = 0; pl < 2; ++pl)
        for (int i = 0; i < 5; ++i) {
            Edge& e = nd.e[pl][i];
            e.prior = r.unit();
            e.q = r.unit() * 6.0f - 1.0f;
            e.visits = r.below(4) ? r.below(300) : 0u;
            e.nif = 40 + r.below(40);
        }
    nd.h0.v1 = r.unit() * 5.0f;
    nd.h0.v2 = r.unit() * 5.0f - 2.0f;
    nd.h0.visits = r.below(5) ? r.below(2000) : 0u;
    nd.h0.nif = 40 + r.below(40);
    t.stats.push_back(nd);
    t.depth.push_back(parent == NIL ? 1u : t.depth[parent] + 1u);
    return (uint32_t)t.stats.size() - 1u;
}

// a spine of `deep` nodes from the root, a side child at every spine node, then random growth
Tree make_tree(Rand& r, uint32_t deep, uint32_t extra) {
    Tree t;
    uint32_t cur = add_node(t, r, NIL);
    for (uint32_t d = 1; d < deep; ++d) cur = add_node(t, r, cur);
    for (uint32_t d = 0; d + 1 < deep; ++d) add_node(t, r, d);
    for (uint32_t i = 0; i < extra; ++i) {
        uint32_t p = r.below((uint32_t)t.stats.size());
        while (t.depth[p] >= MAX_NODES_DEEP) p = t.stats[p].h1.parent;
        add_node(t, r, p);
    }
    return t;
}

struct Batch {
    std::vector<ProcEntry> proc;
    std::vector<EvalOut> ev;
};

void add_entry(Batch& b, Rand& r, uint32_t node, uint32_t kind) {
    ProcEntry pe;
    pe.node = node;
    pe.kind = proc_pack(kind, (uint32_t)b.ev.size(), (uint32_t)b.proc.size());
    if (kind == PROC_EVAL) {
        EvalOut o;
        for (int i = 0; i < 5; ++i) {
            o.p1[i] = r.unit();
            o.p2[i] = r.unit();
        }
        o.v1 = r.unit() * 4.0f;
        o.v2 = r.unit() * 4.0f - 1.0f;
        b.ev.push_back(o);
    }
    b.proc.push_back(pe);
}

// `mode` 0: random leaves; 1: the side children of the spine, deepest first (shared prefixes of every length), the
// spine's end twice as a terminal, the root as a leaf
Batch make_batch(Rand& r, const Tree& t, uint32_t n, uint32_t deep, int mode) {
    Batch b;
    const uint32_t nodes = (uint32_t)t.stats.size();
    std::vector<uint8_t> evaluated(nodes, 0);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t node = r.below(nodes), kind = r.below(2) ? PROC_EVAL : PROC_TERMINAL;
        if (mode == 1) {
            if (i == 0 || i == 3) node = deep - 1, kind = PROC_TERMINAL;
            else if (i == 1) node = 0, kind = r.below(2) ? PROC_EVAL : PROC_TERMINAL;
            else if (deep > 1) node = deep + (deep - 2 - (i * 7u) % (deep - 1));
        } else if (r.below(4) == 0 && i > 0) {
            node = b.proc[r.below(i)].node;  // a leaf claimed again
            kind = PROC_TERMINAL;
        }
        // (the gather evaluates a leaf once; a second claim of it in the same batch would be a collision)
        if (kind == PROC_EVAL && evaluated[node]) kind = PROC_TERMINAL;
        if (kind == PROC_EVAL) evaluated[node] = 1;
        add_entry(b, r, node, kind);
    }
    return b;
}

// backup_round's B_ENTRY / B_LEVEL states for one entry after the other (dev_search.h; no Dirichlet noise here)
uint32_t plain_backup(std::vector<NodeStats>& stats, const Batch& b) {
    uint32_t nv = 0;
    for (const ProcEntry& pe : b.proc) {
        NodeStats& N = stats[pe.node];
        float g1 = 0.0f, g2 = 0.0f;
        if (proc_kind(pe.kind) == PROC_EVAL) {
            const EvalOut o = b.ev[proc_eval_index(pe.kind)];
            float red1[5], red2[5];
            reduce_prior(N.h2.omap[0], o.p1, red1);
            reduce_prior(N.h2.omap[1], o.p2, red2);
            for (int k = 0; k < 5; ++k) {
                N.e[0][k].prior = red1[k];
                N.e[1][k].prior = red2[k];
            }
            g1 = o.v1;
            g2 = o.v2;
        }
        finalize_h0(N.h0, g1, g2, 1);
        nv += 1;
        float v1 = g1, v2 = g2, cr1 = N.h1.r1, cr2 = N.h1.r2;
        uint32_t a1 = meta_po(N.h2.meta, 0), a2 = meta_po(N.h2.meta, 1), parent = N.h1.parent;
        while (parent != NIL) {
            NodeStats& Q = stats[parent];
            const float q1 = cr1 + v1, q2 = cr2 + v2;
            finalize_h0(Q.h0, q1, q2, 1);
            edge_update(Q.e[0][a1], q1, 1);
            edge_update(Q.e[1][a2], q2, 1);
            nv += 1;
            v1 = q1;
            v2 = q2;
            cr1 = Q.h1.r1;
            cr2 = Q.h1.r2;
            a1 = meta_po(Q.h2.meta, 0);
            a2 = meta_po(Q.h2.meta, 1);
            parent = Q.h1.parent;
        }
    }
    return nv;
}

// the kernel's chunk loop, the sixteen lanes one after the other (each phase complete before the next, as the
// kernel's barriers have it)
uint32_t merged_backup(std::vector<NodeStats>& stats, const Batch& b, bool descending, uint32_t path_cap, uint32_t& err) {
    const uint32_t deep_cap = path_cap > PATH_LDS_STEPS ? path_cap - PATH_LDS_STEPS : 0u;
    std::vector<PathStep> step(PATH_LDS_STEPS * PATH_LANES);
    std::vector<float> q1(PATH_LDS_STEPS * PATH_LANES), q2(PATH_LDS_STEPS * PATH_LANES);
    std::vector<uint32_t> head(PATH_LANES), cut(PATH_LANES);
    std::vector<PathNote> deep((size_t)PATH_LANES * deep_cap);
    PathNotes P;
    P.step = step.data();
    P.q1 = q1.data();
    P.q2 = q2.data();
    P.head = head.data();
    P.cut = cut.data();
    P.deep = deep.data();
    P.stride = PATH_LANES;
    P.deep_cap = deep_cap;
    const uint32_t n_proc = (uint32_t)b.proc.size();
    uint32_t nv = 0;
    err = 0;
    for (uint32_t base = 0; base < n_proc; base += PATH_LANES) {
        for (uint32_t i = 0; i < PATH_LANES; ++i) {
            const uint32_t w = descending ? PATH_LANES - 1 - i : i;
            const bool mine = base + w < n_proc;
            err |= bk16_walk(P, w, mine, mine ? b.proc[base + w].node : NIL, mine ? b.proc[base + w].kind : proc_none(),
                             stats.data(), b.ev.data(), path_cap);
        }
        for (uint32_t i = 0; i < PATH_LANES; ++i) bk16_claim(P, descending ? PATH_LANES - 1 - i : i);
        for (uint32_t i = 0; i < PATH_LANES; ++i)
            nv += bk16_apply(P, descending ? PATH_LANES - 1 - i : i, stats.data(), b.ev.data());
    }
    return nv;
}

bool same_bytes(const std::vector<NodeStats>& a, const std::vector<NodeStats>& b, const char* what, unsigned long id) {
    for (size_t i = 0; i < a.size(); ++i)
        if (memcmp(&a[i], &b[i], sizeof(NodeStats)) != 0) {
            fprintf(stderr, "backup_sim: batch %lu, %s lanes: node %zu differs (h0 %s)\n", id, what, i,
                    memcmp(&a[i].h0, &b[i].h0, sizeof(NodeH0)) ? "differs" : "equal");
            return false;
        }
    return true;
}

}  // namespace

int main() {
    static const uint32_t sizes[6] = {1, 2, 15, 16, 17, 33};
    Rand r = {0x5EEDBAC0ULL};
    unsigned long batches = 0;
    for (uint32_t deep = 1; deep <= MAX_NODES_DEEP; ++deep)
        for (int mode = 0; mode < 2; ++mode)
            for (uint32_t n : sizes) {
                const Tree t = make_tree(r, deep, mode ? 6 : 40);
                const Batch b = make_batch(r, t, n, deep, mode);
                std::vector<NodeStats> want = t.stats;
                const uint32_t nv_want = plain_backup(want, b);
                for (int descending = 0; descending < 2; ++descending) {
                    std::vector<NodeStats> got = t.stats;
                    uint32_t err = 0;
                    const uint32_t nv = merged_backup(got, b, descending != 0, PATH_CAP, err);
                    if (err) {
                        fprintf(stderr, "backup_sim: batch %lu: error %u\n", batches, err);
                        return 1;
                    }
                    if (nv != nv_want) {
                        fprintf(stderr, "backup_sim: batch %lu: %u updates, want %u\n", batches, nv, nv_want);
                        return 1;
                    }
                    if (!same_bytes(got, want, descending ? "descending" : "ascending", batches)) return 1;
                }
                batches += 1;
            }
    // a path longer than the cap: error 6, the entry takes no part, the others are served as ever
    {
        const Tree t = make_tree(r, 12, 0);
        Batch b, rest;
        add_entry(b, r, 11, PROC_TERMINAL);  // 12 levels
        add_entry(b, r, 12 + 3, PROC_TERMINAL);  // side child of spine node 3: 5 levels
        add_entry(rest, r, 12 + 3, PROC_TERMINAL);
        std::vector<NodeStats> want = t.stats, got = t.stats;
        const uint32_t nv_want = plain_backup(want, rest);
        uint32_t err = 0;
        const uint32_t nv = merged_backup(got, b, false, 8, err);
        if (err != 6 || nv != nv_want || !same_bytes(got, want, "capped", batches)) {
            fprintf(stderr, "backup_sim: path cap: error %u, %u updates, want 6, %u\n", err, nv, nv_want);
            return 1;
        }
        batches += 1;
    }
    printf("ok: %lu batches\n", batches);
    return 0;
}
