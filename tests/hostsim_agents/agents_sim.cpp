// TEST HARNESS -- runs alpharat_amd/csrc/dev_agents.h on the CPU: the greedy move through the lane phases the kernel
// k_match_greedy runs (greedy_load / greedy_tent / greedy_key / greedy_rank), with a loop over the 64 lanes where the
// device has a wavefront, a plain minimum or sum where it has a wave reduction, and the end of a loop where it has a
// barrier; the temperature sample; and whole matches between any two agent kinds, scheduled like tests/hostsim_match
// (whose slot sets, evaluator stand-in and record readers this file includes and reuses). It is NOT a CPU fallback:
// nothing in alpharat_amd/ loads this file.
#include "../hostsim_match/match_sim.cpp"

#include "../../alpharat_amd/csrc/dev_agents.h"

extern "C" {

struct AsAgent {
    MsAgent search;  // read for a search agent; seed_base for every kind
    uint32_t kind;   // AGENT_*
    float temperature;
};

}  // extern "C"

namespace {

// k_match_greedy's driver. `reverse`: the lanes of every phase run in descending order (no phase may depend on it).
uint32_t greedy_lanes(const uint8_t* cost, int w, int h, const State<4>& st, uint32_t start, int reverse, bool& bound_hit,
                      uint32_t* rounds_out) {
    static GreedyShared sh;
    const uint32_t hw = (uint32_t)(w * h);
    auto lane_of = [&](uint32_t i) { return reverse ? GREEDY_LANES - 1 - i : i; };
    bound_hit = false;
    if (rounds_out) *rounds_out = 0;
    for (uint32_t i = 0; i < GREEDY_LANES; ++i) greedy_load(sh, lane_of(i), cost, st, hw, start);
    if (sh.cheese[start]) return DIR_STAY;
    uint32_t settled = 1;
    for (uint32_t round = 0; round < hw; ++round) {
        if (rounds_out) *rounds_out = round + 1;
        uint32_t level = GREEDY_NONE;
        for (uint32_t i = 0; i < GREEDY_LANES; ++i) {
            const uint32_t t = greedy_tent(sh, lane_of(i), hw, w, h);
            if (t < level) level = t;
        }
        if (level == GREEDY_NONE) return DIR_STAY;
        for (uint32_t i = 0; i < GREEDY_LANES; ++i) greedy_key(sh, lane_of(i), level, hw, w, h);
        uint32_t n = 0, cheese = GREEDY_NO_CHEESE;
        for (uint32_t i = 0; i < GREEDY_LANES; ++i) {
            uint32_t c;
            n += greedy_rank(sh, lane_of(i), level, settled, hw, c);
            if (c < cheese) cheese = c;
        }
        if (cheese != GREEDY_NO_CHEESE) return cheese & 0xffu;
        settled += n;
    }
    bound_hit = true;
    return DIR_STAY;
}

void set_cheese(State<4>& st, const uint8_t* cheese, int hw) {
    std::memset(&st, 0, sizeof st);
    for (int i = 0; i < hw; ++i)
        if (cheese[i]) {
            st.cheese[i >> 6] |= 1ULL << (i & 63);
            st.remaining += 1;
        }
}

}  // namespace

extern "C" {

// the greedy move of a player on cell `start`; out[0] = bound hit, out[1] = levels run
uint32_t as_greedy(uint32_t width, uint32_t height, const uint8_t* cost, const uint8_t* cheese, uint32_t start, int reverse,
                   uint32_t out[2]) {
    State<4> st;
    set_cheese(st, cheese, (int)(width * height));
    bool hit;
    const uint32_t mv = greedy_lanes(cost, (int)width, (int)height, st, start, reverse, hit, &out[1]);
    out[0] = hit ? 1u : 0u;
    return mv;
}

// agent_sample on the stream `state` (advanced in place)
uint32_t as_sample(uint64_t state[4], const float policy[5], float temperature) {
    Rng r = {state[0], state[1], state[2], state[3]};
    const uint32_t a = agent_sample(r, policy, temperature);
    state[0] = r.a, state[1] = r.b, state[2] = r.c, state[3] = r.d;
    return a;
}
// dev_match.h match_sample of a slot whose last search returned `policy` for `player`
uint32_t as_match_sample(uint64_t state[4], const float policy[5], int player) {
    static Slot<1> s;
    std::memset(&s, 0, sizeof s);
    s.rng = Rng{state[0], state[1], state[2], state[3]};
    std::memcpy(s.last.policy[player], policy, 20);
    const uint32_t a = match_sample(s, player);
    state[0] = s.rng.a, state[1] = s.rng.b, state[2] = s.rng.c, state[3] = s.rng.d;
    return a;
}
uint32_t as_random_move(uint64_t state[4]) {
    Rng r = {state[0], state[1], state[2], state[3]};
    const uint32_t a = agent_random_move(r);
    state[0] = r.a, state[1] = r.b, state[2] = r.c, state[3] = r.d;
    return a;
}

// ms_run for any pair of agent kinds: an agent that does not search has no slot set. The result is read with ms_header /
// ms_positions and freed with ms_free.
void* as_run(const MsGame* gs, uint32_t n_games, const AsAgent* aa, const AsAgent* ab, int swap_sides, uint32_t resident,
             uint32_t visit_every) {
    MatchSim* M = new MatchSim();
    uint16_t max_turns = 1;
    for (uint32_t i = 0; i < n_games; ++i)
        if (gs[i].max_turns > max_turns) max_turns = gs[i].max_turns;
    const AsAgent* ag[2] = {aa, ab};
    Side* sides[2] = {&M->a, &M->b};
    bool has[2];
    AgentDesc desc[2];
    for (int k = 0; k < 2; ++k) {
        Side* sd = sides[k];
        has[k] = ag[k]->kind == AGENT_SEARCH;
        sd->agent = ag[k]->search;
        sd->cfg = to_cfg(sd->agent);
        desc[k] = AgentDesc{ag[k]->kind, ag[k]->temperature, has[k] ? sd->cfg.n_sims : 0u, 0u};
        if (!has[k]) continue;
        sd->L = make_layout<4>(sd->cfg, max_turns);
        sd->slots.resize(resident);
        sd->ev.resize(sd->cfg.batch_size);
        for (SlotRun& r : sd->slots) std::memset(&r.slot, 0, sizeof r.slot);
    }
    M->games.resize(resident);
    for (auto& g : M->games) std::memset(&g, 0, sizeof g);
    M->recs.assign(resident, std::vector<MatchPos<4>>(max_turns));
    M->out.resize(n_games);
    std::vector<MatchAux<4>> aux(resident);
    std::vector<std::vector<uint8_t>> cost(resident);
    std::vector<uint32_t> slot_game(resident, 0);
    uint32_t next = 0, finished = 0;
    auto refill = [&](uint32_t sl) {
        if (next >= n_games) return;
        const MsGame& g = gs[next];
        for (int k = 0; k < 2; ++k)
            if (has[k]) sides[k]->start(sides[k]->slots[sl], g);
        const int hw = g.width * g.height;
        cost[sl].assign(g.cost, g.cost + hw * 4);
        MatchAux<4>& x = aux[sl];
        std::memset(&x, 0, sizeof x);
        x.board.width = g.width;
        x.board.height = g.height;
        x.board.max_turns = g.max_turns;
        x.board.maze_off = 0;
        set_cheese(x.st, g.cheese, hw);
        x.board.total_cheese = x.st.remaining;
        x.st.p1 = (uint8_t)(g.p1_y * g.width + g.p1_x);
        x.st.p2 = (uint8_t)(g.p2_y * g.width + g.p2_x);
        rng_seed(x.rng[0], aa->search.seed_base + g.game_index);
        rng_seed(x.rng[1], ab->search.seed_base + g.game_index);
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
            for (int s = 0; s < 2; ++s)
                if (has[s])
                    for (SlotRun& r : sides[s]->slots) sides[s]->step(r);
            for (uint32_t sl = 0; sl < resident; ++sl) {
                Slot<4>* sa = has[0] ? &M->a.slots[sl].slot : nullptr;
                Slot<4>* sb = has[1] ? &M->b.slots[sl].slot : nullptr;
                MatchGame<4>& mg = M->games[sl];
                if (!match_ready_agents(mg, sa, sb)) continue;
                MatchAux<4>& x = aux[sl];
                const int side_a = mg.a_is_p1 ? 0 : 1;
                for (int which = 0; which < 2; ++which) {  // k_match_greedy
                    if (desc[which].kind != AGENT_GREEDY) continue;
                    const int side = which == 0 ? side_a : 1 - side_a;
                    bool hit;
                    x.greedy_act[which] = greedy_lanes(cost[sl].data(), x.board.width, x.board.height, x.st,
                                                       side == 0 ? x.st.p1 : x.st.p2, (int)(sl & 1u), hit, nullptr);
                    if (hit) mg.error = 8;
                }
                match_move_agents(mg, x, sa, sb, desc[0], desc[1], cost[sl].data(), M->recs[sl].data(), (uint32_t)SLOT_ADVANCE);
            }
            for (int s = 0; s < 2; ++s)
                if (has[s])
                    for (SlotRun& r : sides[s]->slots) sides[s]->advance(r);
            M->ticks += 1;
        }
        for (uint32_t sl = 0; sl < resident; ++sl) {
            MatchGame<4>& mg = M->games[sl];
            if (mg.status != MATCH_FINISHED) continue;
            GameOut& o = M->out[slot_game[sl]];
            o.hdr = mg;
            o.pos.assign(M->recs[sl].begin(), M->recs[sl].begin() + (mg.n_pos < max_turns ? mg.n_pos : max_turns));
            mg.status = MATCH_EMPTY;
            if (has[0]) M->a.slots[sl].slot.status = SLOT_EMPTY;
            if (has[1]) M->b.slots[sl].slot.status = SLOT_EMPTY;
            finished += 1;
            refill(sl);
        }
    }
    return M;
}

}  // extern "C"
