// The per-row arithmetic that one training step of SymmetricMLP (train_sym.h) adds to dev_train.h: what the reference does in
//   alpharat/nn/models/symmetric.py  _parse_obs (the three inputs as columns of the flat row)      -> sym_shared_src, sym_player_src
//   the same file, forward: both heads read cat(h_i, h_1 + h_2) with one set of weights            -> sym_head_pack, sym_head_dy
// BatchNorm, the loss terms and their derivatives are dev_train.h's (the loss of architectures/symmetric/loss.py is the
// MLP's). Plain C++ with no barrier, no reduction and no HIP call, as dev_train.h: tests/hostsim_train_sym compiles this text.
#pragma once
#include "dev_train.h"

namespace ar {

// widths of shared_raw = [maze (4 hw), cheese (hw), progress] and of p_raw = [position (hw), mud, score]
AR_HD int sym_shared_dim(int hw) { return 5 * hw + 1; }
AR_HD int sym_player_dim(int hw) { return hw + 2; }

// the column of the flat row (planes [0, 7 hw), then six scalars) that element j of shared_raw is
AR_HD int sym_shared_src(int hw, int j) { return j < 4 * hw ? j : j < 5 * hw ? j + 2 * hw : 7 * hw + 1; }
// ... and that element j of player p's (0 / 1) raw input is: its position plane, scalar 2 + p (mud), scalar 4 + p (score)
AR_HD int sym_player_src(int hw, int p, int j) { return j < hw ? (4 + p) * hw + j : j == hw ? 7 * hw + 2 + p : 7 * hw + 4 + p; }

// With Wh = [policy_head; value_head] of shape (6, 2H), out_i = Wh[:, :H] h_i + Wh[:, H:] (h_1 + h_2) + b, so
//   dh_i = dOut_i Wh[:, :H] + (dOut_1 + dOut_2) Wh[:, H:].
// dout is train_head_terms' [l1 (5), l2 (5), o1, o2]; a packed row is [dOut_i (5 policy, 1 value) | dOut_1 + dOut_2 (6)]:
// the twelve columns whose products with h_i, summed over both players' rows, are the two halves of dWh.
AR_HD void sym_head_pack(const float* dout, float* row_p1, float* row_p2) {
    for (int k = 0; k < 5; ++k) {
        row_p1[k] = dout[k];
        row_p2[k] = dout[5 + k];
    }
    row_p1[5] = dout[10];
    row_p2[5] = dout[11];
    for (int k = 0; k < 6; ++k) row_p1[6 + k] = row_p2[6 + k] = row_p1[k] + row_p2[k];
}

// one element of dh_i: w_lo[k] = Wh[k][col], w_hi[k] = Wh[k][H + col]
AR_HD float sym_head_dy(const float* row, const float* w_lo, const float* w_hi) {
    float dy = 0.0f;
    for (int k = 0; k < 6; ++k) dy += row[k] * w_lo[k];
    for (int k = 0; k < 6; ++k) dy += row[6 + k] * w_hi[k];
    return dy;
}

}  // namespace ar
