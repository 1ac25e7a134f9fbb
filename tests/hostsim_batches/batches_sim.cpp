// TEST HARNESS -- runs rows_build_row_as of alpharat_amd/csrc/dev_rows.h on the CPU: the row of a position as either player
// sees it, one wavefront per row in k_rows_batch, with a loop over the lanes where the device has a wavefront. The games come
// in as tests/hostsim_rows takes them, and its text turns them into position records (hence the include of its source: RsGame
// and records<NW>). It is NOT a CPU fallback: nothing in alpharat_amd/ loads this file.
#include "../hostsim_rows/rows_sim.cpp"

namespace {

template <int NW>
int batch(const RsGame* gs, uint32_t n_games, const uint64_t* rows, const uint8_t* swap, uint64_t n_rows, int reverse,
          const RowOut& out) {
    std::vector<std::vector<PosRec<NW>>> recs(n_games);
    std::vector<RowGame> hdr(n_games);
    std::vector<uint32_t> pos_game, pos_in_game;
    for (uint32_t k = 0; k < n_games; ++k) {
        const RsGame& g = gs[k];
        State<NW> final_st;
        records<NW>(g, recs[k], final_st);
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
    for (uint64_t r = 0; r < n_rows; ++r) {  // k_rows_batch: one wavefront per row
        if (rows[r] >= pos_game.size()) return -1;
        const uint32_t k = pos_game[rows[r]];
        const PosRec<NW>& rec = recs[k][pos_in_game[rows[r]]];
        for (uint32_t i = 0; i < (uint32_t)ROWS_LANES; ++i)
            rows_build_row_as<NW>(reverse ? (uint32_t)ROWS_LANES - 1u - i : i, rec, hdr[k], gs[k].cost, gs[k].outcomes, out, r,
                                  swap && swap[r]);
    }
    return 0;
}

}  // namespace

extern "C" {

// Output row r from position rows[r] of the set (positions numbered through the games in the order given), seen by P2 where
// swap[r] is set (swap == NULL: no row is). reverse: the lanes run in descending order. The cheese outcomes are the records'.
// Returns 0, -1 for a row index out of range, -2 for games of different board sizes.
int bs_build(const RsGame* gs, uint32_t n_games, const uint64_t* rows, const uint8_t* swap, uint64_t n_rows, int reverse,
             float* obs, float* policy_p1, float* policy_p2, float* value_p1, float* value_p2, int8_t* action_p1,
             int8_t* action_p2, int8_t* cheese_outcomes) {
    if (n_games == 0) return n_rows ? -1 : 0;
    for (uint32_t k = 1; k < n_games; ++k)
        if (gs[k].width != gs[0].width || gs[k].height != gs[0].height) return -2;
    const RowOut out = {obs, policy_p1, policy_p2, value_p1, value_p2, action_p1, action_p2, cheese_outcomes};
    return gs[0].width * gs[0].height <= 64u ? batch<1>(gs, n_games, rows, swap, n_rows, reverse, out)
                                             : batch<4>(gs, n_games, rows, swap, n_rows, reverse, out);
}

// sizeof(PosRec) for a board of `cells` cells: what a row set keeps per position (tools/bench_batches.py reports it)
uint32_t bs_record_bytes(uint32_t cells) { return cells <= 64u ? (uint32_t)sizeof(PosRec<1>) : (uint32_t)sizeof(PosRec<4>); }

}  // extern "C"
