// The per-element arithmetic that one training step of PyRatCNN (train_cnn.h) adds to dev_train.h and dev_train_sym.h: what
// the reference does in
//   alpharat/nn/models/cnn/model.py  _parse_obs (the planes, the side vectors and the masks as columns of the flat row)
//                                                                              -> cnn_plane_src, cnn_side_src, cnn_player_cell
//   torch's Conv2d(kernel_size=3, padding=1): which cell a tap of the 3x3 window reads, zero outside the board
//                                                                              -> cnn_nbr, cnn_tap_mirror
// and the two fixed partitions of the n * hw rows of a trunk activation (cnn_cols, cnn_split). BatchNorm, the loss terms
// and the heads are dev_train.h's and dev_train_sym.h's. Plain C++ with no barrier, no reduction and no HIP call:
// tests/hostsim_train_cnn compiles this text.
#pragma once
#include "dev_train_sym.h"

namespace ar {

// Tap t = 3 ky + kx of W[co][ci][ky][kx] reads the cell at (y + ky - 1, x + kx - 1): torch's cross-correlation.
AR_HD int cnn_tap_dy(int tap) { return tap / 3 - 1; }
AR_HD int cnn_tap_dx(int tap) { return tap % 3 - 1; }
// the tap of the input gradient: dIn[y][x] takes W[..][ky][kx] dOut[y - ky + 1][x - kx + 1], the offsets negated
AR_HD int cnn_tap_mirror(int tap) { return 8 - tap; }

// the cell (y' * bw + x') that `tap` reads at (y, x) of a bw x bh board, -1 outside the board
AR_HD int cnn_nbr_yx(int y, int x, int tap, int bw, int bh) {
    const int yy = y + cnn_tap_dy(tap), xx = x + cnn_tap_dx(tap);
    return (yy >= 0 && yy < bh && xx >= 0 && xx < bw) ? yy * bw + xx : -1;
}
AR_HD int cnn_nbr(int cell, int tap, int bw, int bh) { return cnn_nbr_yx(cell / bw, cell % bw, tap, bw, bh); }

// the column of the flat row (planes [0, 7 hw), then six scalars) that channel d of `cell` of the stem's input is: the four
// maze channels lie cell by cell, the cheese plane is the seventh
AR_HD int cnn_plane_src(int hw, int cell, int d) { return d < 4 ? 4 * cell + d : 6 * hw + cell; }
// ... and that element j of player p's (0 / 1) side vector [score, mud, progress] is
AR_HD int cnn_side_src(int hw, int p, int j) { return 7 * hw + (j == 0 ? 4 + p : j == 1 ? 2 + p : 1); }
// the cell of player p: where its position plane is not zero (a one-hot plane; -1 for an empty one, whose features are 0)
AR_HD int cnn_player_cell(const float* row, int hw, int p) {
    const float* plane = row + (4 + p) * hw;
    for (int c = 0; c < hw; ++c)
        if (plane[c] != 0.0f) return c;
    return -1;
}

// The two fixed partitions of the R = n * hw rows of a trunk activation; as train_cols and train_split they set the order of
// every sum over the batch, a function of (n, hw, C) alone. Their caps are wider than the MLP's: 4096 rows of 7x7 are
// 200 704 rows here, which 32 parts would leave to 32 blocks.
enum { CNN_MAX_PARTS = 256, CNN_PART_ROWS = 64, CNN_MAX_SPLITS = 64, CNN_SPLIT_ROWS = 512 };

// for the column kernels: P consecutive parts of rpp rows, the last one maybe shorter. No thread walks the P parts: they are
// collapsed in index order first (k_cnn_collapse).
inline TrainCols cnn_cols(int n, int hw, int C) {
    const int R = n * hw;
    TrainCols t;
    t.n = R;
    t.H = C;
    t.P = (R + CNN_PART_ROWS - 1) / CNN_PART_ROWS < CNN_MAX_PARTS ? (R + CNN_PART_ROWS - 1) / CNN_PART_ROWS : CNN_MAX_PARTS;
    t.rpp = (R + t.P - 1) / t.P;
    t.P = (R + t.rpp - 1) / t.rpp;
    return t;
}

// of the rows a weight gradient is reduced over (k_train_conv3's blockIdx.z): S ranges of kps rows, kps a multiple of the k chunk
inline TrainSplit cnn_split(int n, int hw) {
    const int R = n * hw;
    TrainSplit s;
    s.S = (R + CNN_SPLIT_ROWS - 1) / CNN_SPLIT_ROWS < CNN_MAX_SPLITS ? (R + CNN_SPLIT_ROWS - 1) / CNN_SPLIT_ROWS : CNN_MAX_SPLITS;
    s.kps = ((R + s.S - 1) / s.S + TG_KC - 1) / TG_KC * TG_KC;
    s.S = (R + s.kps - 1) / s.kps;
    return s;
}

}  // namespace ar
