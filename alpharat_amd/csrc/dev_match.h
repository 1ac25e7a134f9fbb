// A head-to-head match between two search agents, one move of one game: the device-side counterpart of the reference's
// evaluation-time loop,
//   alpharat/eval/game.py:47-87        play_game: both agents move from the same position until the game is over,
//   alpharat/ai/searcher_agent.py:40-56 SearcherAgent.get_move: a search on a fresh tree, then one sample of the policy of
//                                      the side the agent plays (temperature 1.0, :53-54),
//   alpharat/eval/tournament.py:329-373 the per-game worker (who plays which side, the result from the final scores).
//
// A game of a match sits in slot k of two slot sets, one per agent. Each set is a self-play engine of its own
// (configuration, gather kernel, leaf queue, evaluator) whose slots are `single_search` slots: a finished search stops in
// SLOT_DONE with Slot::last filled and the slot's random stream where the search left it (finish_move). match_move runs
// when BOTH slots of a game are there: it draws the two actions, records the position, steps it once and hands both
// slots to the fresh-root path of the tree re-rooting kernel (pending_root == NIL) -- or marks the game finished.
// A slot whose partner is still searching stays in SLOT_DONE, which no search kernel touches.
//
// Streams: agent X's search and its action sample draw from X's own stream of this game, seeded once per game and never
// re-seeded; nothing X computes depends on the other agent's stream, on the slot the game sits in, or on when the
// move happens.
//
// Like the rest of dev_search.h the function is __host__ __device__, so the CPU harness under tests/ runs it unchanged.
#pragma once
#include "dev_search.h"

namespace ar {

enum { MATCH_EMPTY = 0, MATCH_PLAYING = 1, MATCH_FINISHED = 2 };

// One position of a match game (eval/game.py keeps no record; this is selfplay.rs:80-102 PositionRecord with the search
// output of both agents).
template <int NW>
struct MatchPos {
    State<NW> st;
    MoveResult a, b;  // what agent A's / agent B's search returned at `st`
    uint8_t a1, a2;   // the actions played by P1 and P2
    uint8_t pad[6];
};

// Per-game header of the match-owned buffer.
template <int NW>
struct MatchGame {
    uint32_t status;   // MATCH_*
    uint32_t game_index;
    uint32_t n_pos;
    uint32_t a_is_p1;  // tournament.py:397 swap_sides: 0 when agent B plays P1
    uint32_t error;    // non-zero: more positions than max_turns (bug guard)
    uint32_t pad[3];
    State<NW> final_st;
};

// both searches of the game's current position are complete
template <int NW>
AR_HD bool match_ready(const MatchGame<NW>& g, const Slot<NW>& a, const Slot<NW>& b) {
    return g.status == MATCH_PLAYING && a.status == SLOT_DONE && b.status == SLOT_DONE;
}

// searcher_agent.py:53-56: one draw from the agent's stream after its search; a negative result (all-zero policy) maps to
// STAY as in finish_move
template <int NW>
AR_HD uint32_t match_sample(Slot<NW>& s, int player) {
    const int a = rng_weighted5(s.rng, s.last.policy[player]);
    return a < 0 ? 4u : (uint32_t)a;
}

// a slot goes back to searching from the new position on a fresh tree, its stream kept
template <int NW>
AR_HD void match_rearm(Slot<NW>& s, const State<NW>& st, uint32_t n_sims, uint32_t advance_status) {
    s.st = st;
    s.remaining = n_sims;
    s.s_nn = 0;
    s.s_term = 0;
    s.s_coll = 0;
    s.pending_root = NIL;
    s.status = advance_status;
}

// One move of one game (match_ready holds). `pos` is the game's record buffer of board.max_turns entries, `cost` its maze.
// `advance_status` is the status the re-rooting kernel of this launch order accepts (SLOT_ADVANCE, parity-tagged by the
// caller where a side stream is in use).
template <int NW>
AR_HD void match_move(MatchGame<NW>& g, Slot<NW>& a, Slot<NW>& b, const uint8_t* cost, MatchPos<NW>* pos, uint32_t sims_a,
                      uint32_t sims_b, uint32_t advance_status) {
    const int side_a = g.a_is_p1 ? 0 : 1;
    const uint32_t act_a = match_sample(a, side_a);
    const uint32_t act_b = match_sample(b, 1 - side_a);
    const uint32_t a1 = g.a_is_p1 ? act_a : act_b, a2 = g.a_is_p1 ? act_b : act_a;
    State<NW> st = a.st;  // (both slots hold the same position)
    if (g.n_pos < a.board.max_turns) {
        MatchPos<NW>& p = pos[g.n_pos];
        p.st = st;
        p.a = a.last;
        p.b = b.last;
        p.a1 = (uint8_t)a1;
        p.a2 = (uint8_t)a2;
    } else {
        g.error = 7;
    }
    g.n_pos += 1;
    float r1, r2;
    st_step(a.board, cost, st, a1, a2, r1, r2);
    if (st_over(a.board, st) || g.error) {
        a.st = st;
        b.st = st;
        g.final_st = st;
        g.status = MATCH_FINISHED;  // both slots stay in SLOT_DONE until the game is drained
        return;
    }
    match_rearm(a, st, sims_a, advance_status);
    match_rearm(b, st, sims_b, advance_status);
}

}  // namespace ar
