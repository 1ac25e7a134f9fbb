// Training rows from self-play records: what the reference's sharding step computes once per position in Python
// (alpharat/data/sharding.py:513-595 _process_games_to_arrays), as per-row logic that runs on the device.
//   alpharat/nn/builders/flat.py:142-197   FlatObservationBuilder.build   -> flat_observation (k_encode runs the same text)
//   alpharat/nn/targets.py:19-70           build_targets                  -> rows_build_row
//   crates/alpharat-sampling/src/selfplay.rs:415-471 compute_cheese_outcomes -> rows_game_outcomes
//   alpharat/nn/augmentation.py:86-184     swap_player_perspective_batch  -> rows_build_row_as (the row as P2 sees it)
//
// A row is built by one wavefront (k_rows_build, k_rows_batch); a game's cheese outcomes by one block (k_rows_append). Every
// function is written as loops over `lane, lane + lanes, ...`, so that the CPU harnesses under tests/hostsim_rows and
// tests/hostsim_batches run the same text with a loop over the lanes. No lane reads what another lane wrote: there is no
// barrier and no reduction in this file.
#pragma once
#include "dev_search.h"

namespace ar {

enum { ROWS_LANES = 64 };

// One stored game (32 bytes). Its maze (hw * 4 cost bytes) and its cheese outcomes (hw bytes) sit in two arrays indexed by
// the game's number in the store.
struct RowGame {
    uint16_t width, height, max_turns, pad;
    float final1, final2;  // final scores
    uint32_t game_index;
    uint32_t n_rows;       // positions of this game
    uint64_t first_row;    // its first position in the store
};

// The eight arrays of a shard (alpharat/nn/training/keys.py:52-62 BatchKey), each contiguous over rows
struct RowOut {
    float* observation;       // [n][hw * 7 + 6]
    float* policy_p1;         // [n][5]
    float* policy_p2;         // [n][5]
    float* value_p1;          // [n]
    float* value_p2;          // [n]
    int8_t* action_p1;        // [n]
    int8_t* action_p2;        // [n]
    int8_t* cheese_outcomes;  // [n][h][w]
};

AR_HD uint32_t rows_obs_dim(uint32_t hw) { return hw * 7u + 6u; }

// flat.py:142-197 / flat_encoder.rs:52-125: maze cost / 10 (wall or edge: -1), P1 one-hot, P2 one-hot, cheese, six scalars.
// Every value is one f32 operation on values that are exact in f32.
template <int NW>
AR_HD void flat_observation(uint32_t lane, uint32_t lanes, const State<NW>& st, int hw, uint16_t max_turns, const uint8_t* cost,
                            float* o) {
    for (int k = (int)lane; k < hw * 4; k += (int)lanes) o[k] = cost[k] ? (float)cost[k] / 10.0f : -1.0f;
    for (int k = (int)lane; k < hw; k += (int)lanes) {
        o[hw * 4 + k] = k == st.p1 ? 1.0f : 0.0f;
        o[hw * 5 + k] = k == st.p2 ? 1.0f : 0.0f;
        o[hw * 6 + k] = st_has_cheese(st, k) ? 1.0f : 0.0f;
    }
    if (lane == 0) {
        float* s = o + hw * 7;
        s[0] = st.s1 - st.s2;
        s[1] = max_turns > 0 ? (float)st.turn / (float)max_turns : 0.0f;
        s[2] = (float)st.m1 / 10.0f;
        s[3] = (float)st.m2 / 10.0f;
        s[4] = st.s1 / 10.0f;
        s[5] = st.s2 / 10.0f;
    }
}

// Output row `r` from one position record of game `g`; `cost` is the game's maze, `outcomes` its cheese outcomes.
// targets.py:46-50: the policies are copied, the values are final score - score at the position (scores are multiples of 0.5:
// the f32 subtraction is exact); targets.py:58-60: the game's outcome where the position still has the cheese, else -1.
template <int NW>
AR_HD void rows_build_row(uint32_t lane, const PosRec<NW>& rec, const RowGame& g, const uint8_t* cost, const uint8_t* outcomes,
                          const RowOut& out, uint64_t r) {
    const int hw = (int)g.width * (int)g.height;
    flat_observation<NW>(lane, ROWS_LANES, rec.st, hw, g.max_turns, cost, out.observation + r * rows_obs_dim((uint32_t)hw));
    for (uint32_t k = lane; k < 5u; k += ROWS_LANES) {
        out.policy_p1[r * 5u + k] = rec.res.policy[0][k];
        out.policy_p2[r * 5u + k] = rec.res.policy[1][k];
    }
    if (lane == 0) {
        out.value_p1[r] = g.final1 - rec.st.s1;
        out.value_p2[r] = g.final2 - rec.st.s2;
        out.action_p1[r] = (int8_t)rec.a1;
        out.action_p2[r] = (int8_t)rec.a2;
    }
    int8_t* co = out.cheese_outcomes + r * (uint64_t)hw;
    for (int c = (int)lane; c < hw; c += ROWS_LANES) co[c] = st_has_cheese(rec.st, c) ? (int8_t)outcomes[c] : (int8_t)-1;
}

// The same row seen by either player (k_rows_batch): with `swap` clear, what rows_build_row writes; with it set, what
// alpharat/nn/augmentation.py:86-184 swap_player_perspective_batch makes of that row -- the one-hot planes of the two players
// exchanged, scalars 2 <-> 3 (mud) and 4 <-> 5 (scores) exchanged, the policies, actions and values exchanged, and cheese
// outcome 0 (P1 took it) <-> 3 (P2 took it); the maze, the cheese plane, scalar 1 and outcomes -1, 1 and 2 stay. Scalar 0 is
// the negation of the unswapped difference, not s2 - s1: equal scores give -0.0, as `-obs` does in the reference. `swap` is
// per row, so uniform over the wavefront: every use of it is a select between two values of the same record.
template <int NW>
AR_HD void rows_build_row_as(uint32_t lane, const PosRec<NW>& rec, const RowGame& g, const uint8_t* cost, const uint8_t* outcomes,
                             const RowOut& out, uint64_t r, bool swap) {
    const int hw = (int)g.width * (int)g.height;
    const State<NW>& st = rec.st;
    const int pa = swap ? st.p2 : st.p1, pb = swap ? st.p1 : st.p2;  // the players in the row's order
    float* o = out.observation + r * rows_obs_dim((uint32_t)hw);
    for (int k = (int)lane; k < hw * 4; k += ROWS_LANES) o[k] = cost[k] ? (float)cost[k] / 10.0f : -1.0f;
    for (int k = (int)lane; k < hw; k += ROWS_LANES) {
        o[hw * 4 + k] = k == pa ? 1.0f : 0.0f;
        o[hw * 5 + k] = k == pb ? 1.0f : 0.0f;
        o[hw * 6 + k] = st_has_cheese(st, k) ? 1.0f : 0.0f;
    }
    const int a = swap ? 1 : 0, b = a ^ 1;
    for (uint32_t k = lane; k < 5u; k += ROWS_LANES) {
        out.policy_p1[r * 5u + k] = rec.res.policy[a][k];
        out.policy_p2[r * 5u + k] = rec.res.policy[b][k];
    }
    if (lane == 0) {
        const float diff = st.s1 - st.s2;
        const float sa = swap ? st.s2 : st.s1, sb = swap ? st.s1 : st.s2;
        float* s = o + hw * 7;
        s[0] = swap ? -diff : diff;
        s[1] = g.max_turns > 0 ? (float)st.turn / (float)g.max_turns : 0.0f;
        s[2] = (float)(swap ? st.m2 : st.m1) / 10.0f;
        s[3] = (float)(swap ? st.m1 : st.m2) / 10.0f;
        s[4] = sa / 10.0f;
        s[5] = sb / 10.0f;
        out.value_p1[r] = (swap ? g.final2 : g.final1) - sa;
        out.value_p2[r] = (swap ? g.final1 : g.final2) - sb;
        out.action_p1[r] = (int8_t)(swap ? rec.a2 : rec.a1);
        out.action_p2[r] = (int8_t)(swap ? rec.a1 : rec.a2);
    }
    int8_t* co = out.cheese_outcomes + r * (uint64_t)hw;
    for (int c = (int)lane; c < hw; c += ROWS_LANES) {
        const uint8_t v = outcomes[c];
        co[c] = !st_has_cheese(st, c) ? (int8_t)-1 : (int8_t)(swap && (v == 0 || v == 3) ? 3 - v : v);
    }
}

// selfplay.rs:415-471 for one cell: the first position after which the cell has lost its cheese decides, by who stands on the
// cell in the next position (the final state after the last one): 0 P1, 1 both, 3 P2; 2 when nobody does or it never goes.
template <int NW>
AR_HD uint8_t rows_cell_outcome(const PosRec<NW>* pos, uint32_t n, const State<NW>& final_st, int c) {
    for (uint32_t i = 0; i < n; ++i) {
        if (!st_has_cheese(pos[i].st, c)) continue;
        const State<NW>& next = i + 1 < n ? pos[i + 1].st : final_st;
        if (st_has_cheese(next, c)) continue;
        return (next.p1 == c && next.p2 == c) ? 1 : next.p1 == c ? 0 : next.p2 == c ? 3 : 2;
    }
    return 2;
}
template <int NW>
AR_HD void rows_game_outcomes(uint32_t lane, uint32_t lanes, const PosRec<NW>* pos, uint32_t n, const State<NW>& final_st, int hw,
                              uint8_t* out) {
    for (int c = (int)lane; c < hw; c += (int)lanes) out[c] = rows_cell_outcome<NW>(pos, n, final_st, c);
}

}  // namespace ar
