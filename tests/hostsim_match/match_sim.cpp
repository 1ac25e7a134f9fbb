// TEST HARNESS -- plays whole head-to-head matches on the CPU with the product's device-side code: the search headers
// (alpharat_amd/csrc/dev_search.h, written __host__ __device__) for both agents' searches and dev_match.h match_move for
// the pairing, scheduled the way the device runs them: two slot sets of `resident` slots, one batch step of every slot
// per tick, then the moves of the games whose two searches are complete, then the fresh roots, and every few ticks the
// finished games are drained and their slot pairs refilled. It is NOT a CPU fallback: nothing in alpharat_amd/ loads
// this file. (tests/hostsim is the harness of single searches and self-play games; its evaluator stand-ins are restated.)
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../alpharat_amd/csrc/slot_layout.h"
#include "../../alpharat_amd/csrc/dev_match.h"
#include "../../alpharat_amd/csrc/zig_norm_tables.inc"

using namespace ar;

static const ZigTables g_zig = {AR_ZIG_NORM_X_INIT, AR_ZIG_NORM_F_INIT};

extern "C" {

struct MsAgent {
    float c_puct, fpu_reduction, force_k, noise_epsilon, noise_concentration;
    uint32_t coll_min, coll_max, coll_start, coll_end;
    float coll_power;
    uint32_t n_sims, batch;
    uint32_t evaluator;      // 0 SmartUniform inside the gather, 1 hashed_eval on stored leaves
    uint32_t gather_rounds;  // 0: a gather runs to its end; else rounds per tick (the gather is parked and resumed)
    uint32_t arena_nodes;    // 0: the product's fresh arena; else a small one (trees stall and grow mid-search)
    uint64_t seed_base;
};
struct MsGame {
    uint8_t width, height;
    uint16_t max_turns;
    uint8_t p1_x, p1_y, p2_x, p2_y;
    uint32_t game_index;
    const uint8_t* cost;    // [hw*4]
    const uint8_t* cheese;  // [hw]
};

}  // extern "C"

namespace {

// tests/hostsim/hostsim.cpp hashed_eval, restated: priors and values that are a fixed hash of the position
void hashed_eval(const State<4>& lf, EvalOut& o) {
    uint32_t x = (uint32_t)lf.p1 * 7919u + (uint32_t)lf.p2 * 104729u + (uint32_t)lf.turn * 1299709u;
    for (int c = 0; c < 256; ++c)
        if (st_has_cheese(lf, c)) x += (uint32_t)(c + 1) * 15485863u;
    for (int pl = 0; pl < 2; ++pl) {
        float w[5], tot = 0.0f;
        for (uint32_t a = 0; a < 5; ++a) {
            const uint32_t h = (x + a * 40503u + (uint32_t)pl * 7u) * 2654435761u;
            w[a] = (float)(1u + ((h >> 8) % 1000u));
            tot += w[a];
        }
        for (int a = 0; a < 5; ++a) (pl == 0 ? o.p1 : o.p2)[a] = w[a] / tot;
    }
    o.v1 = (float)((x * 2246822519u >> 10) % 64u) / 16.0f;
    o.v2 = (float)((x * 3266489917u >> 10) % 64u) / 16.0f;
}

SearchCfg to_cfg(const MsAgent& c) {
    SearchCfg s;
    s.c_puct = c.c_puct;
    s.fpu_reduction = c.fpu_reduction;
    s.force_k = c.force_k;
    s.noise_epsilon = c.noise_epsilon;
    s.noise_concentration = c.noise_concentration;
    s.coll_min = c.coll_min;
    s.coll_max = c.coll_max;
    s.coll_start = c.coll_start;
    s.coll_end = c.coll_end;
    s.coll_power = c.coll_power;
    s.n_sims = c.n_sims;
    s.batch_size = c.batch;
    s.alloc_per_round = 2;
    return s;
}

struct SlotRun {
    Slot<4> slot;
    std::vector<unsigned char> scratch, arena;
    std::vector<uint8_t> cost;
};

// one agent's slot set
struct Side {
    MsAgent agent;
    SearchCfg cfg;
    SlotLayout L;
    std::vector<SlotRun> slots;
    std::vector<EvalOut> ev;
    uint32_t grows = 0;

    Mem<4> mem(SlotRun& r) { return resolve_mem<4>(r.slot, r.arena.data(), r.scratch.data(), 0, L, r.cost.data()); }
    void set_arena(SlotRun& r, uint32_t cap) {
        r.slot.cap = cap;
        r.slot.stats_off = 0;
        r.slot.fwd_off = (long long)((size_t)cap * sizeof(NodeStats));
    }
    void start(SlotRun& r, const MsGame& g) {
        const int hw = g.width * g.height;
        r.cost.assign(g.cost, g.cost + hw * 4);
        r.scratch.assign(L.total, 0);
        const uint32_t cap = agent.arena_nodes ? agent.arena_nodes : initial_arena_nodes(cfg);
        r.arena.assign(arena_bytes(cap) + 256, 0);
        Slot<4>& s = r.slot;
        std::memset(&s, 0, sizeof s);
        set_arena(r, cap);
        s.board.width = g.width;
        s.board.height = g.height;
        s.board.max_turns = g.max_turns;
        s.board.maze_off = 0;
        uint16_t rem = 0;
        for (int i = 0; i < hw; ++i)
            if (g.cheese[i]) {
                s.st.cheese[i >> 6] |= 1ULL << (i & 63);
                ++rem;
            }
        s.st.remaining = rem;
        s.board.total_cheese = rem;
        s.st.p1 = (uint8_t)(g.p1_y * g.width + g.p1_x);
        s.st.p2 = (uint8_t)(g.p2_y * g.width + g.p2_x);
        rng_seed(s.rng, agent.seed_base + g.game_index);
        s.game_index = g.game_index;
        s.single_search = 1;
        start_game(s, mem(r), cfg);
    }
    // what the runtime does for a stalled slot: a doubled arena, live nodes copied across unchanged
    void grow(SlotRun& r) {
        uint32_t ncap = r.slot.cap * 2;
        while (ncap < r.slot.need_nodes) ncap *= 2;
        std::vector<unsigned char> na(arena_bytes(ncap) + 256);
        std::memcpy(na.data(), r.arena.data(), (size_t)r.slot.hi * sizeof(NodeStats));
        r.arena.swap(na);
        set_arena(r, ncap);
        r.slot.status = SLOT_ACTIVE;
        grows += 1;
    }
    // one batch step of one slot: what the gather / evaluator / backup kernels do for it in one launch set
    void step(SlotRun& r) {
        Slot<4>& s = r.slot;
        if (s.status == SLOT_STALL) {
            grow(r);
            return;
        }
        if (s.status != SLOT_ACTIVE) return;  // (SLOT_DONE: waits for its partner, untouched)
        Mem<4> m = mem(r);
        const int mode = agent.evaluator == 0 ? EVAL_UNIFORM : EVAL_STORE;
        if (agent.gather_rounds) {
            if (gather_machine_limited(s, m, cfg, mode, agent.gather_rounds) != GATHER_COMPLETE) return;
        } else if (!gather_machine(s, m, cfg, mode)) {
            return;
        }
        const EvalOut* evp = m.ev_local;
        if (agent.evaluator != 0) {
            for (uint32_t j = 0; j < s.b_nn; ++j) hashed_eval(m.leaf_local[j], ev[j]);
            evp = ev.data();
        }
        if (backup_machine(s, m, cfg, evp, &g_zig)) finish_move(s, m, cfg);
    }
    void advance(SlotRun& r) {
        if (r.slot.status == SLOT_ADVANCE) advance_tree_scalar(r.slot, mem(r));
    }
};

struct GameOut {
    MatchGame<4> hdr;
    std::vector<MatchPos<4>> pos;
};

struct MatchSim {
    Side a, b;
    std::vector<MatchGame<4>> games;            // per slot
    std::vector<std::vector<MatchPos<4>>> recs;  // per slot, max_turns entries
    std::vector<GameOut> out;                    // finished games in game order
    uint64_t ticks = 0;
};

}  // namespace

extern "C" {

// `visit_every`: ticks between two drains / refills (how the run is cut into launches)
void* ms_run(const MsGame* gs, uint32_t n_games, const MsAgent* aa, const MsAgent* ab, int swap_sides, uint32_t resident,
             uint32_t visit_every) {
    MatchSim* M = new MatchSim();
    uint16_t max_turns = 1;
    for (uint32_t i = 0; i < n_games; ++i)
        if (gs[i].max_turns > max_turns) max_turns = gs[i].max_turns;
    for (Side* sd : {&M->a, &M->b}) {
        sd->agent = sd == &M->a ? *aa : *ab;
        sd->cfg = to_cfg(sd->agent);
        sd->L = make_layout<4>(sd->cfg, max_turns);
        sd->slots.resize(resident);
        sd->ev.resize(sd->cfg.batch_size);
        for (SlotRun& r : sd->slots) std::memset(&r.slot, 0, sizeof r.slot);
    }
    M->games.resize(resident);
    for (auto& g : M->games) std::memset(&g, 0, sizeof g);
    M->recs.assign(resident, std::vector<MatchPos<4>>(max_turns));
    M->out.resize(n_games);
    std::vector<uint32_t> slot_game(resident, 0);
    uint32_t next = 0, finished = 0;
    auto refill = [&](uint32_t sl) {
        if (next >= n_games) return;
        const MsGame& g = gs[next];
        M->a.start(M->a.slots[sl], g);
        M->b.start(M->b.slots[sl], g);
        MatchGame<4>& mg = M->games[sl];
        std::memset(&mg, 0, sizeof mg);
        mg.status = MATCH_PLAYING;
        mg.game_index = g.game_index;
        mg.a_is_p1 = (swap_sides && (g.game_index & 1u)) ? 0u : 1u;
        slot_game[sl] = next++;
    };
    for (uint32_t sl = 0; sl < resident; ++sl) refill(sl);
    while (finished < n_games) {
        for (uint32_t k = 0; k < visit_every; ++k) {
            for (SlotRun& r : M->a.slots) M->a.step(r);
            for (SlotRun& r : M->b.slots) M->b.step(r);
            for (uint32_t sl = 0; sl < resident; ++sl) {
                Slot<4>&sa = M->a.slots[sl].slot, &sb = M->b.slots[sl].slot;
                if (!match_ready(M->games[sl], sa, sb)) continue;
                match_move(M->games[sl], sa, sb, M->a.slots[sl].cost.data(), M->recs[sl].data(), M->a.cfg.n_sims,
                           M->b.cfg.n_sims, (uint32_t)SLOT_ADVANCE);
            }
            for (SlotRun& r : M->a.slots) M->a.advance(r);
            for (SlotRun& r : M->b.slots) M->b.advance(r);
            M->ticks += 1;
        }
        for (uint32_t sl = 0; sl < resident; ++sl) {
            MatchGame<4>& mg = M->games[sl];
            if (mg.status != MATCH_FINISHED) continue;
            GameOut& o = M->out[slot_game[sl]];
            o.hdr = mg;
            o.pos.assign(M->recs[sl].begin(), M->recs[sl].begin() + (mg.n_pos < max_turns ? mg.n_pos : max_turns));
            mg.status = MATCH_EMPTY;
            M->a.slots[sl].slot.status = SLOT_EMPTY;
            M->b.slots[sl].slot.status = SLOT_EMPTY;
            finished += 1;
            refill(sl);
        }
    }
    return M;
}
void ms_free(void* p) { delete (MatchSim*)p; }

// [n_positions, a_is_p1, error, game_index], final scores; totals: [ticks, grows of A, grows of B]
void ms_header(const void* p, uint32_t game, uint32_t out[4], float fs[2], uint64_t totals[3]) {
    const MatchSim* M = (const MatchSim*)p;
    const GameOut& o = M->out[game];
    out[0] = o.hdr.n_pos;
    out[1] = o.hdr.a_is_p1;
    out[2] = o.hdr.error;
    out[3] = o.hdr.game_index;
    fs[0] = o.hdr.final_st.s1;
    fs[1] = o.hdr.final_st.s2;
    totals[0] = M->ticks;
    totals[1] = M->a.grows;
    totals[2] = M->b.grows;
}
static void fill_floats(const State<4>& st, const MoveResult& m, float* F) {
    F[0] = st.s1;
    F[1] = st.s2;
    F[2] = m.value[0];
    F[3] = m.value[1];
    std::memcpy(F + 4, m.visit_counts[0], 20);
    std::memcpy(F + 9, m.visit_counts[1], 20);
    std::memcpy(F + 14, m.prior[0], 20);
    std::memcpy(F + 19, m.prior[1], 20);
    std::memcpy(F + 24, m.policy[0], 20);
    std::memcpy(F + 29, m.policy[1], 20);
}
// per position: ints[9] = p1x p1y p2x p2y mud1 mud2 turn a1 a2; per agent floats[34] (the layout of the oracle driver's
// position rows) and counts[4] = total_visits nn_evals terminals collisions; the cheese mask
void ms_positions(const void* p, uint32_t game, uint32_t width, uint32_t hw, int32_t* ints, float* fa, float* fb,
                  uint32_t* ca, uint32_t* cb, uint8_t* masks) {
    const MatchSim* M = (const MatchSim*)p;
    const GameOut& o = M->out[game];
    for (size_t i = 0; i < o.pos.size(); ++i) {
        const MatchPos<4>& q = o.pos[i];
        int32_t* I = ints + i * 9;
        I[0] = q.st.p1 % width;
        I[1] = q.st.p1 / width;
        I[2] = q.st.p2 % width;
        I[3] = q.st.p2 / width;
        I[4] = q.st.m1;
        I[5] = q.st.m2;
        I[6] = q.st.turn;
        I[7] = q.a1;
        I[8] = q.a2;
        fill_floats(q.st, q.a, fa + i * 34);
        fill_floats(q.st, q.b, fb + i * 34);
        const MoveResult* rs[2] = {&q.a, &q.b};
        for (int k = 0; k < 2; ++k) {
            uint32_t* c = (k ? cb : ca) + i * 4;
            c[0] = rs[k]->total_visits;
            c[1] = rs[k]->nn_evals;
            c[2] = rs[k]->terminals;
            c[3] = rs[k]->collisions;
        }
        for (uint32_t c = 0; c < hw; ++c) masks[i * hw + c] = st_has_cheese(q.st, (int)c);
    }
}

}  // extern "C"
