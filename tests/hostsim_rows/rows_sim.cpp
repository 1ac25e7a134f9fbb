// TEST HARNESS -- runs alpharat_amd/csrc/dev_rows.h on the CPU: the row of a position (rows_build_row, one wavefront per row
// in k_rows_build) and the cheese outcomes of a game (rows_game_outcomes, one block per game in k_rows_append), with a loop
// over the lanes where the device has a wavefront or a block. Boards of up to 64 cells run the NW = 1 instantiation, larger
// ones NW = 4, as the library chooses. It is NOT a CPU fallback: nothing in alpharat_amd/ loads this file.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../alpharat_amd/csrc/dev_rows.h"

using namespace ar;

extern "C" {

// One game as the oracle records it (tests/_oracle.py play_game): per position ints p1x p1y p2x p2y p1_mud p2_mud turn a1 a2,
// floats p1_score p2_score value_p1 value_p2 visits[10] prior[10] policy_p1[5] policy_p2[5], and the cheese mask.
struct RsGame {
    uint32_t width, height, max_turns, n;
    float final1, final2;
    uint32_t final_p1, final_p2;  // cells of the final state
    const uint8_t* cost;          // [hw * 4]
    const uint8_t* outcomes;      // [hw]: the record's cheese outcomes
    const uint8_t* final_mask;    // [hw]
    const int32_t* ints;          // [n][9]
    const float* floats;          // [n][34]
    const uint8_t* masks;         // [n][hw]
};

}  // extern "C"

namespace {

template <int NW>
void set_mask(State<NW>& st, const uint8_t* mask, uint32_t hw) {
    for (uint32_t c = 0; c < hw; ++c)
        if (mask[c]) {
            st.cheese[c >> 6] |= 1ULL << (c & 63u);
            st.remaining += 1;
        }
}

template <int NW>
void records(const RsGame& g, std::vector<PosRec<NW>>& recs, State<NW>& final_st) {
    const uint32_t hw = g.width * g.height;
    recs.resize(g.n);
    for (uint32_t i = 0; i < g.n; ++i) {
        PosRec<NW>& p = recs[i];
        std::memset(&p, 0, sizeof p);
        const int32_t* v = g.ints + (size_t)i * 9;
        const float* f = g.floats + (size_t)i * 34;
        set_mask<NW>(p.st, g.masks + (size_t)i * hw, hw);
        p.st.p1 = (uint8_t)(v[1] * (int32_t)g.width + v[0]);
        p.st.p2 = (uint8_t)(v[3] * (int32_t)g.width + v[2]);
        p.st.m1 = (uint8_t)v[4];
        p.st.m2 = (uint8_t)v[5];
        p.st.turn = (uint16_t)v[6];
        p.a1 = (uint8_t)v[7];
        p.a2 = (uint8_t)v[8];
        p.st.s1 = f[0];
        p.st.s2 = f[1];
        std::memcpy(p.res.policy[0], f + 24, 20);
        std::memcpy(p.res.policy[1], f + 29, 20);
    }
    std::memset(&final_st, 0, sizeof final_st);
    set_mask<NW>(final_st, g.final_mask, hw);
    final_st.p1 = (uint8_t)g.final_p1;
    final_st.p2 = (uint8_t)g.final_p2;
    final_st.s1 = g.final1;
    final_st.s2 = g.final2;
}

template <int NW>
int build(const RsGame* gs, uint32_t n_games, const uint64_t* rows, uint64_t n_rows, int reverse, int use_rule,
          const RowOut& out) {
    std::vector<std::vector<PosRec<NW>>> recs(n_games);
    std::vector<std::vector<uint8_t>> outcomes(n_games);
    std::vector<RowGame> hdr(n_games);
    std::vector<uint32_t> pos_game;
    std::vector<uint32_t> pos_in_game;
    for (uint32_t k = 0; k < n_games; ++k) {
        const RsGame& g = gs[k];
        const uint32_t hw = g.width * g.height;
        State<NW> final_st;
        records<NW>(g, recs[k], final_st);
        outcomes[k].assign(g.outcomes, g.outcomes + hw);
        if (use_rule)  // as k_rows_append: a block of 128 threads over the cells
            for (uint32_t i = 0; i < 128u; ++i)
                rows_game_outcomes<NW>(reverse ? 127u - i : i, 128u, recs[k].data(), g.n, final_st, (int)hw, outcomes[k].data());
        RowGame& h = hdr[k];
        h.width = (uint16_t)g.width;
        h.height = (uint16_t)g.height;
        h.max_turns = (uint16_t)g.max_turns;
        h.pad = 0;
        h.final1 = g.final1;
        h.final2 = g.final2;
        h.game_index = k;
        h.n_rows = g.n;
        h.first_row = pos_game.size();
        for (uint32_t i = 0; i < g.n; ++i) {
            pos_game.push_back(k);
            pos_in_game.push_back(i);
        }
    }
    for (uint64_t r = 0; r < n_rows; ++r) {  // k_rows_build: one wavefront per row
        if (rows[r] >= pos_game.size()) return -1;
        const uint32_t k = pos_game[rows[r]];
        const PosRec<NW>& rec = recs[k][pos_in_game[rows[r]]];
        for (uint32_t i = 0; i < (uint32_t)ROWS_LANES; ++i)
            rows_build_row<NW>(reverse ? (uint32_t)ROWS_LANES - 1u - i : i, rec, hdr[k], gs[k].cost, outcomes[k].data(), out, r);
    }
    return 0;
}

}  // namespace

extern "C" {

// Output row r from position rows[r] of the set (positions numbered through the games in the order given).
// reverse: the lanes run in descending order (no lane may depend on another). use_rule: the games' cheese outcomes are
// computed from the records and the final state (an attached run), else taken from the record (ar_rows_add_games).
// Returns 0, -1 for a row index out of range, -2 for games of different board sizes.
int rs_build(const RsGame* gs, uint32_t n_games, const uint64_t* rows, uint64_t n_rows, int reverse, int use_rule, float* obs,
             float* policy_p1, float* policy_p2, float* value_p1, float* value_p2, int8_t* action_p1, int8_t* action_p2,
             int8_t* cheese_outcomes) {
    if (n_games == 0) return n_rows ? -1 : 0;
    for (uint32_t k = 1; k < n_games; ++k)
        if (gs[k].width != gs[0].width || gs[k].height != gs[0].height) return -2;
    const RowOut out = {obs, policy_p1, policy_p2, value_p1, value_p2, action_p1, action_p2, cheese_outcomes};
    return gs[0].width * gs[0].height <= 64u ? build<1>(gs, n_games, rows, n_rows, reverse, use_rule, out)
                                             : build<4>(gs, n_games, rows, n_rows, reverse, use_rule, out);
}

// rows_game_outcomes of one game with `lanes` lanes
void rs_outcomes(const RsGame* g, uint32_t lanes, int reverse, uint8_t* out) {
    const uint32_t hw = g->width * g->height;
    if (hw <= 64u) {
        std::vector<PosRec<1>> recs;
        State<1> fin;
        records<1>(*g, recs, fin);
        for (uint32_t i = 0; i < lanes; ++i) rows_game_outcomes<1>(reverse ? lanes - 1u - i : i, lanes, recs.data(), g->n, fin, (int)hw, out);
    } else {
        std::vector<PosRec<4>> recs;
        State<4> fin;
        records<4>(*g, recs, fin);
        for (uint32_t i = 0; i < lanes; ++i) rows_game_outcomes<4>(reverse ? lanes - 1u - i : i, lanes, recs.data(), g->n, fin, (int)hw, out);
    }
}

}  // extern "C"
