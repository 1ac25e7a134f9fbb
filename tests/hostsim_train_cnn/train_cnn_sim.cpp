// TEST HARNESS -- runs alpharat_amd/csrc/dev_train_cnn.h on the CPU: the cell a tap of the 3x3 window reads (cnn_nbr, resolved
// per operand element in k_train_conv3) and its mirror, the columns of the flat row that make the stem's input, the side
// vectors and the player cells (one lane per element in k_cnn_split), and the two partitions of the n * hw trunk rows, with
// loops where the device has lanes. It is NOT a CPU fallback: nothing in alpharat_amd/ loads this file.
#include <cstdint>

#include "../../alpharat_amd/csrc/dev_train_cnn.h"

using namespace ar;

extern "C" {

int tcs_nbr(int cell, int tap, int bw, int bh) { return cnn_nbr(cell, tap, bw, bh); }
int tcs_mirror(int tap) { return cnn_tap_mirror(tap); }

// x [n][7hw + 6]; x5 [n hw][5]; side [2n][3] and cells [2n], P1's rows first
void tcs_split(uint64_t n, int hw, const float* x, float* x5, float* side, int32_t* cells) {
    const int D = 7 * hw + 6;
    for (uint64_t r = 0; r < n; ++r) {
        for (int c = 0; c < hw; ++c)
            for (int d = 0; d < 5; ++d) x5[(r * hw + c) * 5 + d] = x[r * D + cnn_plane_src(hw, c, d)];
        for (int p = 0; p < 2; ++p) {
            for (int j = 0; j < 3; ++j) side[(p * n + r) * 3 + j] = x[r * D + cnn_side_src(hw, p, j)];
            cells[p * n + r] = cnn_player_cell(x + r * D, hw, p);
        }
    }
}

// out: P, rpp
void tcs_cols(int n, int hw, int C, int32_t* out) {
    const TrainCols t = cnn_cols(n, hw, C);
    out[0] = t.P;
    out[1] = t.rpp;
}

// out: S, kps
void tcs_rows_split(int n, int hw, int32_t* out) {
    const TrainSplit s = cnn_split(n, hw);
    out[0] = s.S;
    out[1] = s.kps;
}

// out: the caps and the rows a part and a range have below them
void tcs_caps(int32_t* out) {
    out[0] = CNN_MAX_PARTS;
    out[1] = CNN_PART_ROWS;
    out[2] = CNN_MAX_SPLITS;
    out[3] = CNN_SPLIT_ROWS;
}

}  // extern "C"
