// Match agents that do not search, and the temperature of those that do: the per-move logic of the reference's
// benchmark set (alpharat/eval/benchmark.py:78-125 build_standard_agents),
//   alpharat/ai/random_agent.py:17-19   RandomAgent.get_move: one uniform draw over the five actions,
//   alpharat/ai/greedy_agent.py:23-84   GreedyAgent.get_move: Dijkstra to the nearest cheese, its first step,
//   alpharat/ai/utils.py:8-40           select_action_from_strategy: argmax / sample / tempered sample.
// (The pure-network agent, ai/config.py:88-106, is a one-simulation search plus a temperature: no code of its own.)
//
// A match game whose agents do not both search keeps its position, the streams of its random agents and the moves of
// its greedy agents in a match-owned record (MatchAux); an agent that searches keeps its engine slot as before.
// match_move_agents is dev_match.h match_move for any pair of agent kinds; for two search agents at temperature 1.0 it
// makes the same draws in the same order and writes the same records.
//
// The greedy move is computed by one wavefront per game (k_match_greedy), the board's cells spread over its 64 lanes.
// The reference's heap, ordered by (cost, push counter), is reproduced without a heap: cells settle level by level in
// increasing distance, and inside a level in the order of the key (settle rank of the winning parent, direction), which
// is the order of the push counters ("Matches"). The level is written as three lane phases over a
// shared block (greedy_tent / greedy_key / greedy_rank), with a barrier and a wave reduction between them, so that the
// CPU harness under tests/ runs the same phases with a loop over the lanes.
#pragma once
#include "dev_match.h"

namespace ar {

enum { AGENT_SEARCH = 0, AGENT_RANDOM = 1, AGENT_GREEDY = 2 };  // ArMatchAgent::kind

struct AgentDesc {
    uint32_t kind;      // AGENT_*
    float temperature;  // search agents: utils.py:26-40
    uint32_t n_sims;    // search agents: the budget a slot is re-armed with
    uint32_t pad;
};

// Match-owned state of one resident game (slot k of the match, beside MatchGame)
template <int NW>
struct MatchAux {
    Board board;
    State<NW> st;            // the game's position (a searching agent's slot holds the same one)
    Rng rng[2];              // streams of agent A / B when they are random agents (seeded once per game)
    uint32_t greedy_act[2];  // k_match_greedy's answer for agent A / B at `st`
    uint32_t pad[2];
};

// ---- random ----------------------------------------------------------------------------------------------------
// random_agent.py:19 random.randint(0, 4): one draw per move, in mud or not
AR_HD uint32_t agent_random_move(Rng& r) { return rng_below(r, 5u); }

// ---- temperature -----------------------------------------------------------------------------------------------
// utils.py:26-40 on the f32 policy of the side played. T == 1: today's match_sample. T == 0: first index of the largest
// entry, no draw. Otherwise q_i = exp(log(p_i + 1e-10) / T) in f64, summed in index order, w_i = (float)(q_i / sum), one
// rng_weighted5 draw. An all-zero policy is STAY at every temperature and takes no draw.
AR_HD uint32_t agent_sample(Rng& r, const float* policy, float temperature) {
    if (temperature == 1.0f) {
        const int a = rng_weighted5(r, policy);
        return a < 0 ? 4u : (uint32_t)a;
    }
    bool all_zero = true;
    for (int i = 0; i < 5; ++i) all_zero = all_zero && policy[i] == 0.0f;
    if (all_zero) return 4u;
    if (temperature == 0.0f) {
        uint32_t best = 0;
        float top = policy[0];
        for (uint32_t i = 1; i < 5u; ++i) {
            const float v = sel5f(policy, i);
            if (v > top) {
                top = v;
                best = i;
            }
        }
        return best;
    }
    double q[5], sum = 0.0;
    for (int i = 0; i < 5; ++i) {
        q[i] = exp(log((double)policy[i] + 1e-10) / (double)temperature);
        sum += q[i];
    }
    float w[5];
    for (int i = 0; i < 5; ++i) w[i] = (float)(q[i] / sum);
    const int a = rng_weighted5(r, w);
    return a < 0 ? 4u : (uint32_t)a;
}

// ---- greedy ----------------------------------------------------------------------------------------------------
enum { GREEDY_LANES = 64, GREEDY_CELLS = 256, GREEDY_NONE = 0xFFFFu, GREEDY_NO_CHEESE = 0xFFFFFFFFu };

// One game's working set (LDS on the device): 3.5 KB
struct GreedyShared {
    uint32_t cost[GREEDY_CELLS];  // the four direction costs of a cell, cell_costs()
    uint16_t dist[GREEDY_CELLS];  // distance of a settled cell
    uint16_t rank[GREEDY_CELLS];  // settle rank = position in the heap's pop order; GREEDY_NONE: not settled
    uint16_t tent[GREEDY_CELLS];  // tentative distance of an unsettled cell in the current level; GREEDY_NONE: none
    uint16_t key[GREEDY_CELLS];   // cells of the current level: rank of the winning parent * 4 + direction; else NONE
    uint8_t first[GREEDY_CELLS];  // first move of the path that settled the cell
    uint8_t cheese[GREEDY_CELLS];
};

// the cell one step from `cell` in direction d (st_step's geometry), -1 outside the board
AR_HD int greedy_neighbour(int cell, uint32_t d, int w, int h) {
    const int x = cell % w, y = cell / w;
    if (d == DIR_UP) return y + 1 < h ? cell + w : -1;
    if (d == DIR_RIGHT) return x + 1 < w ? cell + 1 : -1;
    if (d == DIR_DOWN) return y > 0 ? cell - w : -1;
    return x > 0 ? cell - 1 : -1;
}

// lane phase 0: the maze, the cheese and the start cell (rank 0, distance 0)
template <int NW>
AR_HD void greedy_load(GreedyShared& sh, uint32_t lane, const uint8_t* cost, const State<NW>& st, uint32_t hw, uint32_t start) {
    for (uint32_t c = lane; c < hw; c += GREEDY_LANES) {
        sh.cost[c] = cell_costs(cost, c);
        sh.dist[c] = c == start ? 0u : (uint16_t)GREEDY_NONE;
        sh.rank[c] = c == start ? 0u : (uint16_t)GREEDY_NONE;
        sh.tent[c] = (uint16_t)GREEDY_NONE;
        sh.key[c] = (uint16_t)GREEDY_NONE;
        sh.first[c] = (uint8_t)DIR_STAY;
        sh.cheese[c] = st_has_cheese(st, (int)c) ? 1 : 0;
    }
}

// lane phase 1: the tentative distance of every unsettled cell of this lane, min over the settled cells u with an edge
// u -> v of dist[u] + w(u -> v). Returns the lane's minimum (GREEDY_NONE: nothing on the frontier).
AR_HD uint32_t greedy_tent(GreedyShared& sh, uint32_t lane, uint32_t hw, int w, int h) {
    uint32_t lane_min = GREEDY_NONE;
    for (uint32_t v = lane; v < hw; v += GREEDY_LANES) {
        uint32_t t = GREEDY_NONE;
        if (sh.rank[v] == GREEDY_NONE) {
            for (uint32_t dv = 0; dv < 4u; ++dv) {
                const int u = greedy_neighbour((int)v, dv, w, h);
                if (u < 0 || sh.rank[u] == GREEDY_NONE) continue;
                const uint32_t d = (dv + 2u) & 3u;  // the direction that leads from u to v
                const uint32_t wt = (sh.cost[u] >> (8u * d)) & 0xffu;
                if (wt == 0) continue;
                const uint32_t nc = (uint32_t)sh.dist[u] + wt;
                if (nc < t) t = nc;
            }
        }
        sh.tent[v] = (uint16_t)t;
        if (t < lane_min) lane_min = t;
    }
    return lane_min;
}

// lane phase 2: the cells of this lane that settle at distance `level` take the key and the first move of their
// winning parent: the lowest-ranked settled u with dist[u] + w(u -> v) == level (each (u, d) reaches one cell: keys are
// unique). The heap pushed v with this cost when it popped u and tried direction d, and never again.
AR_HD void greedy_key(GreedyShared& sh, uint32_t lane, uint32_t level, uint32_t hw, int w, int h) {
    for (uint32_t v = lane; v < hw; v += GREEDY_LANES) {
        uint32_t key = GREEDY_NONE, first = DIR_STAY;
        if (sh.tent[v] == level && level != GREEDY_NONE) {
            for (uint32_t dv = 0; dv < 4u; ++dv) {
                const int u = greedy_neighbour((int)v, dv, w, h);
                if (u < 0 || sh.rank[u] == GREEDY_NONE) continue;
                const uint32_t d = (dv + 2u) & 3u;
                const uint32_t wt = (sh.cost[u] >> (8u * d)) & 0xffu;
                if (wt == 0 || (uint32_t)sh.dist[u] + wt != level) continue;
                const uint32_t k = (uint32_t)sh.rank[u] * 4u + d;
                if (k < key) {
                    key = k;
                    first = sh.rank[u] == 0 ? d : sh.first[u];  // (rank 0 is the start cell)
                }
            }
            sh.first[v] = (uint8_t)first;
        }
        sh.key[v] = (uint16_t)key;
    }
}

// lane phase 3 (after a barrier): the cells of the level settle; a cell's rank is `base` + the number of smaller keys in
// the level. Returns the number of cells this lane settled; `cheese` becomes min over this lane's settled cheese cells of
// rank << 8 | first move (GREEDY_NO_CHEESE: none).
AR_HD uint32_t greedy_rank(GreedyShared& sh, uint32_t lane, uint32_t level, uint32_t base, uint32_t hw, uint32_t& cheese) {
    uint32_t mine[GREEDY_CELLS / GREEDY_LANES], below[GREEDY_CELLS / GREEDY_LANES];
    bool any = false;
#pragma unroll
    for (uint32_t k = 0; k < GREEDY_CELLS / GREEDY_LANES; ++k) {
        const uint32_t v = lane + k * GREEDY_LANES;
        mine[k] = v < hw ? (uint32_t)sh.key[v] : (uint32_t)GREEDY_NONE;
        below[k] = 0;
        any = any || mine[k] != GREEDY_NONE;
    }
    cheese = GREEDY_NO_CHEESE;
    if (!any) return 0;
    for (uint32_t j = 0; j < hw; ++j) {
        const uint32_t kj = sh.key[j];
#pragma unroll
        for (uint32_t k = 0; k < GREEDY_CELLS / GREEDY_LANES; ++k) below[k] += kj < mine[k] ? 1u : 0u;
    }
    uint32_t n = 0;
#pragma unroll
    for (uint32_t k = 0; k < GREEDY_CELLS / GREEDY_LANES; ++k) {
        if (mine[k] == GREEDY_NONE) continue;
        const uint32_t v = lane + k * GREEDY_LANES;
        // (a key of NONE is never below a member's key, so `below` counts members only)
        const uint32_t r = base + below[k];
        sh.rank[v] = (uint16_t)r;
        sh.dist[v] = (uint16_t)level;
        if (sh.cheese[v]) {
            const uint32_t c = (r << 8) | sh.first[v];
            if (c < cheese) cheese = c;
        }
        n += 1;
    }
    return n;
}

// ---- the move of one game, any pair of agent kinds ---------------------------------------------------------------
// every searching agent's search of the current position is complete (`a` / `b`: null for an agent without a slot)
template <int NW>
AR_HD bool match_ready_agents(const MatchGame<NW>& g, const Slot<NW>* a, const Slot<NW>* b) {
    return g.status == MATCH_PLAYING && (!a || a->status == SLOT_DONE) && (!b || b->status == SLOT_DONE);
}

template <int NW>
AR_HD uint32_t agent_action(const AgentDesc& d, Slot<NW>* s, MatchAux<NW>& x, int which, int side) {
    if (d.kind == AGENT_RANDOM) return agent_random_move(x.rng[which]);
    if (d.kind == AGENT_GREEDY) return x.greedy_act[which];
    return agent_sample(s->rng, s->last.policy[side], d.temperature);
}

// dev_match.h match_move with the position in `x`: match_ready_agents holds, and the greedy agents' moves for x.st are in
// x.greedy_act. The record of an agent that does not search is all zero.
template <int NW>
AR_HD void match_move_agents(MatchGame<NW>& g, MatchAux<NW>& x, Slot<NW>* a, Slot<NW>* b, const AgentDesc& da,
                             const AgentDesc& db, const uint8_t* cost, MatchPos<NW>* pos, uint32_t advance_status) {
    const int side_a = g.a_is_p1 ? 0 : 1;
    const uint32_t act_a = agent_action(da, a, x, 0, side_a);
    const uint32_t act_b = agent_action(db, b, x, 1, 1 - side_a);
    const uint32_t a1 = g.a_is_p1 ? act_a : act_b, a2 = g.a_is_p1 ? act_b : act_a;
    State<NW> st = x.st;
    if (g.n_pos < x.board.max_turns) {
        MatchPos<NW>& p = pos[g.n_pos];
        const MoveResult none = {};
        p.st = st;
        p.a = a ? a->last : none;
        p.b = b ? b->last : none;
        p.a1 = (uint8_t)a1;
        p.a2 = (uint8_t)a2;
        for (int i = 0; i < 6; ++i) p.pad[i] = 0;
    } else {
        g.error = 7;
    }
    g.n_pos += 1;
    float r1, r2;
    st_step(x.board, cost, st, a1, a2, r1, r2);
    x.st = st;
    if (st_over(x.board, st) || g.error) {
        if (a) a->st = st;
        if (b) b->st = st;
        g.final_st = st;
        g.status = MATCH_FINISHED;  // the slots stay in SLOT_DONE until the game is drained
        return;
    }
    if (a) match_rearm(*a, st, da.n_sims, advance_status);
    if (b) match_rearm(*b, st, db.n_sims, advance_status);
}

}  // namespace ar
