// TEST HARNESS -- the sixteen-lane backup's collision cancel (alpharat_amd/csrc/dev_backup16.h: bk16_fold adds a record's
// count to the lane whose entry has the record's node as its leaf, bk16_settle subtracts that total from every ancestor
// while it has the node in registers, bk16_cancel_left walks what was not folded) on the CPU, as a program of its own
// (tests/test_backup_collide_cpu.py runs it, once plain and once built with -fsanitize=address,undefined).
// Random small trees with in-flight counts everywhere, as in backup_sim.cpp; batches of 1, 2, 15, 16, 17 and 33 entries
// in chunks of sixteen, collision lists of 0, 1, 16, 17 and 40 records (and one of 530, past the 512 a lane's mask
// holds): several records on one leaf, records whose leaf is in another chunk than their own index, the same terminal
// leaf claimed twice with records on it, records on an entry whose leaf is the root, paths past PATH_LDS_STEPS, records
// with node NIL, records on a node that is no entry's leaf, and an entry past path_cap (error 6) with a record on its
// leaf. The lanes of a chunk run one after the other, ascending and descending. The yardstick is the entry-by-entry
// backup followed by the plain cancel walk (backup_machine, dev_search.h), restated below. Every node record must come
// out equal byte for byte, the update counts equal, and every record must be folded exactly when its node is a noted
// leaf and walked otherwise: never both, never neither. Exit status 0 and a line "ok: N batches ..." when that holds.
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

// in-flight counts hold every subtraction of a batch (33 entries + 530 records of at most 3), so nothing wraps
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
    for (int pl = 0; pl < 2; ++pl)
        for (int i = 0; i < 5; ++i) {
            Edge& e = nd.e[pl][i];
            e.prior = r.unit();
            e.q = r.unit() * 6.0f - 1.0f;
            e.visits = r.below(4) ? r.below(300) : 0u;
            e.nif = 2000 + r.below(1000);
        }
    nd.h0.v1 = r.unit() * 5.0f;
    nd.h0.v2 = r.unit() * 5.0f - 2.0f;
    nd.h0.visits = r.below(5) ? r.below(2000) : 0u;
    nd.h0.nif = 2000 + r.below(1000);
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
    std::vector<CollEntry> coll;
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
// spine's end twice as a terminal (entries 0 and 3), the root as a leaf (entry 1)
void make_entries(Batch& b, Rand& r, const Tree& t, uint32_t n, uint32_t deep, int mode) {
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
        if (kind == PROC_EVAL && evaluated[node]) kind = PROC_TERMINAL;
        if (kind == PROC_EVAL) evaluated[node] = 1;
        add_entry(b, r, node, kind);
    }
}

uint32_t other_node(Rand& r, const Tree& t, const Batch& b) {  // a node that is no entry's leaf (NIL if there is none)
    const uint32_t nodes = (uint32_t)t.stats.size(), start = r.below(nodes);
    for (uint32_t k = 0; k < nodes; ++k) {
        const uint32_t x = (start + k) % nodes;
        bool leaf = false;
        for (const ProcEntry& pe : b.proc) leaf = leaf || pe.node == x;
        if (!leaf) return x;
    }
    return NIL;
}

// `c` records: mostly on the leaves of random entries (so on entries of any chunk, whatever the record's own index),
// some on the node of the record before (several on one leaf), some NIL, some on a node that is no leaf. Fixed ones:
// record 0 on the last entry (the last chunk), record 1 on the same leaf, record 2 on entry 0 (in mode 1 the terminal
// claimed twice), record 3 on entry 1 (in mode 1 the root), record 16 on entry 0 (the first chunk), 5 NIL, 6 no leaf.
void make_records(Batch& b, Rand& r, const Tree& t, uint32_t c) {
    const uint32_t n = (uint32_t)b.proc.size();
    for (uint32_t i = 0; i < c; ++i) {
        CollEntry ce;
        ce.mv = 1 + r.below(3);
        const uint32_t what = r.below(10);
        ce.node = b.proc[r.below(n)].node;
        if (what == 7 && i > 0) ce.node = b.coll[i - 1].node;
        if (what == 8) ce.node = NIL;
        if (what == 9) ce.node = other_node(r, t, b);
        if (i == 0) ce.node = b.proc[n - 1].node;
        if (i == 1) ce.node = b.coll[0].node;
        if (i == 2) ce.node = b.proc[0].node;
        if (i == 3 && n > 1) ce.node = b.proc[1].node;
        if (i == 16) ce.node = b.proc[0].node;
        if (i == 5) ce.node = NIL;
        if (i == 6) ce.node = other_node(r, t, b);
        b.coll.push_back(ce);
    }
}

// backup_round's B_ENTRY / B_LEVEL states for one entry after the other, then backup_machine's cancel walk of every
// record (dev_search.h; mcts.hpp:598), a record without a node skipped
uint32_t plain_backup(std::vector<NodeStats>& stats, const std::vector<ProcEntry>& proc, const Batch& b) {
    uint32_t nv = 0;
    for (const ProcEntry& pe : proc) {
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
    for (const CollEntry& ce : b.coll) {
        if (ce.node == NIL) continue;
        uint32_t cur = ce.node;
        for (;;) {
            const uint32_t parent = stats[cur].h1.parent;
            if (parent == NIL) break;
            const uint32_t meta = stats[cur].h2.meta;
            NodeStats& Q = stats[parent];
            Q.h0.nif -= ce.mv;
            Q.e[0][meta_po(meta, 0)].nif -= ce.mv;
            Q.e[1][meta_po(meta, 1)].nif -= ce.mv;
            cur = parent;
        }
    }
    return nv;
}

struct Counts {
    uint32_t nv, err, folded, walked;
};

// the kernel's chunk loop and its tail, the sixteen lanes one after the other (each phase complete before the next, as
// the kernel's barriers have it)
Counts merged_backup(std::vector<NodeStats>& stats, const Batch& b, bool descending, uint32_t path_cap) {
    const uint32_t deep_cap = path_cap > PATH_LDS_STEPS ? path_cap - PATH_LDS_STEPS : 0u;
    std::vector<PathStep> step(PATH_LDS_STEPS * PATH_LANES);
    std::vector<float> q1(PATH_LDS_STEPS * PATH_LANES), q2(PATH_LDS_STEPS * PATH_LANES);
    std::vector<uint32_t> head(PATH_LANES), cut(PATH_LANES), cm(PATH_LANES);
    std::vector<PathNote> deep((size_t)PATH_LANES * deep_cap);
    PathNotes P;
    P.step = step.data();
    P.q1 = q1.data();
    P.q2 = q2.data();
    P.head = head.data();
    P.cut = cut.data();
    P.cm = cm.data();
    P.deep = deep.data();
    P.stride = PATH_LANES;
    P.deep_cap = deep_cap;
    const uint32_t n_proc = (uint32_t)b.proc.size(), n_coll = (uint32_t)b.coll.size();
    Counts c = {0, 0, 0, 0};
    uint32_t left[PATH_LANES];
    for (uint32_t w = 0; w < PATH_LANES; ++w) left[w] = bk16_coll_mask(n_coll, w);
    auto lane = [&](uint32_t i) { return descending ? PATH_LANES - 1 - i : i; };
    for (uint32_t base = 0; base < n_proc; base += PATH_LANES) {
        for (uint32_t i = 0; i < PATH_LANES; ++i) {
            const uint32_t w = lane(i);
            const bool mine = base + w < n_proc;
            P.cm[w] = 0;
            c.err |= bk16_walk(P, w, mine, mine ? b.proc[base + w].node : NIL, mine ? b.proc[base + w].kind : proc_none(),
                               stats.data(), b.ev.data(), path_cap);
        }
        for (uint32_t i = 0; i < PATH_LANES; ++i) {
            const uint32_t w = lane(i), was = left[w];
            // (the kernel has a lane's first two records in registers before the walk)
            CollEntry c0 = {NIL, 0}, c1 = {NIL, 0};
            if (was & 1u) c0 = b.coll[w];
            if (was & 2u) c1 = b.coll[PATH_LANES + w];
            left[w] = bk16_fold(P, w, b.coll.data(), was, c0, c1);
            if (left[w] & ~was) {
                fprintf(stderr, "collide_sim: a folded record came back\n");
                exit(1);
            }
            c.folded += (uint32_t)__builtin_popcount(was ^ left[w]);
        }
        for (uint32_t i = 0; i < PATH_LANES; ++i) bk16_claim(P, lane(i));
        for (uint32_t i = 0; i < PATH_LANES; ++i) c.nv += bk16_apply(P, lane(i), stats.data(), b.ev.data());
    }
    for (uint32_t i = 0; i < PATH_LANES; ++i) c.walked += bk16_cancel_left(lane(i), b.coll.data(), n_coll, left[lane(i)], stats.data());
    return c;
}

bool same_bytes(const std::vector<NodeStats>& a, const std::vector<NodeStats>& b, const char* what, unsigned long id) {
    for (size_t i = 0; i < a.size(); ++i)
        if (memcmp(&a[i], &b[i], sizeof(NodeStats)) != 0) {
            fprintf(stderr, "collide_sim: batch %lu, %s lanes: node %zu differs (h0 %s; nif %u, want %u)\n", id, what, i,
                    memcmp(&a[i].h0, &b[i].h0, sizeof(NodeH0)) ? "differs" : "equal", a[i].h0.nif, b[i].h0.nif);
            return false;
        }
    return true;
}

// one batch both ways; `served` = the entries that take part (all but those dropped with error 6)
bool check(const Tree& t, const Batch& b, const std::vector<ProcEntry>& served, uint32_t path_cap, uint32_t want_err,
           unsigned long id, unsigned long& folded, unsigned long& walked) {
    std::vector<NodeStats> want = t.stats;
    const uint32_t nv_want = plain_backup(want, served, b);
    // a record folds exactly when its node is the leaf of a served entry; every other record with a node is walked
    uint32_t fold_want = 0, walk_want = 0;
    for (const CollEntry& ce : b.coll) {
        bool leaf = false;
        for (const ProcEntry& pe : served) leaf = leaf || pe.node == ce.node;
        fold_want += leaf ? 1u : 0u;
        walk_want += !leaf && ce.node != NIL ? 1u : 0u;
    }
    for (int descending = 0; descending < 2; ++descending) {
        std::vector<NodeStats> got = t.stats;
        const Counts c = merged_backup(got, b, descending != 0, path_cap);
        if (c.err != want_err || c.nv != nv_want || c.folded != fold_want || c.walked != walk_want) {
            fprintf(stderr, "collide_sim: batch %lu: error %u (want %u), %u updates (want %u), %u folded (want %u), %u walked (want %u)\n",
                    id, c.err, want_err, c.nv, nv_want, c.folded, fold_want, c.walked, walk_want);
            return false;
        }
        if (!same_bytes(got, want, descending ? "descending" : "ascending", id)) return false;
    }
    folded += fold_want;
    walked += walk_want;
    return true;
}

}  // namespace

int main() {
    static const uint32_t sizes[6] = {1, 2, 15, 16, 17, 33}, lists[5] = {0, 1, 16, 17, 40};
    Rand r = {0xC0111DE5ULL};
    unsigned long batches = 0, folded = 0, walked = 0;
    for (uint32_t deep = 1; deep <= MAX_NODES_DEEP; ++deep)
        for (int mode = 0; mode < 2; ++mode)
            for (uint32_t n : sizes)
                for (uint32_t c : lists) {
                    const Tree t = make_tree(r, deep, mode ? 6 : 40);
                    Batch b;
                    make_entries(b, r, t, n, deep, mode);
                    make_records(b, r, t, c);
                    if (!check(t, b, b.proc, PATH_CAP, 0, batches, folded, walked)) return 1;
                    batches += 1;
                }
    // more records than the 32 a lane keeps a bit for: the rest is walked, whatever its node
    {
        const Tree t = make_tree(r, 14, 40);
        Batch b;
        make_entries(b, r, t, 33, 14, 1);
        make_records(b, r, t, 530);
        std::vector<NodeStats> want = t.stats, got = t.stats;
        const uint32_t nv_want = plain_backup(want, b.proc, b);
        const Counts c = merged_backup(got, b, false, PATH_CAP);
        uint32_t with_node = 0;
        for (const CollEntry& ce : b.coll) with_node += ce.node != NIL ? 1u : 0u;
        if (c.err || c.nv != nv_want || c.folded + c.walked != with_node || c.folded == 0 || !same_bytes(got, want, "530 records", batches)) {
            fprintf(stderr, "collide_sim: 530 records: error %u, %u updates (want %u), %u folded + %u walked (want %u)\n", c.err, c.nv,
                    nv_want, c.folded, c.walked, with_node);
            return 1;
        }
        batches += 1;
    }
    // a path longer than the cap: error 6, the entry takes no part and notes no leaf, so the records on its leaf are walked
    {
        const Tree t = make_tree(r, 12, 0);
        Batch b;
        add_entry(b, r, 11, PROC_TERMINAL);      // 12 levels
        add_entry(b, r, 12 + 3, PROC_TERMINAL);  // side child of spine node 3: 5 levels
        const std::vector<ProcEntry> served(b.proc.begin() + 1, b.proc.end());
        const CollEntry recs[4] = {{11, 2}, {12 + 3, 1}, {NIL, 3}, {11, 1}};
        b.coll.assign(recs, recs + 4);
        const unsigned long walked_before = walked;
        if (!check(t, b, served, 8, 6, batches, folded, walked)) return 1;
        if (walked - walked_before != 2) {
            fprintf(stderr, "collide_sim: path cap: the dropped entry's records were not walked\n");
            return 1;
        }
        batches += 1;
    }
    if (folded == 0 || walked == 0) {
        fprintf(stderr, "collide_sim: %lu folded, %lu walked: one of the two ways was never taken\n", folded, walked);
        return 1;
    }
    printf("ok: %lu batches, %lu records folded, %lu walked\n", batches, folded, walked);
    return 0;
}
