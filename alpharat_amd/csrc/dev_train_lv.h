// The per-cell arithmetic that one training step of LocalValueMLP (train_lv.h) adds to dev_train.h: what the reference does in
//   alpharat/nn/losses/ownership.py:26-46                  compute_ownership_loss: the mean over the cells with
//                                                          cheese_outcomes >= 0 of logsumexp(l) - l[target], 0 without
//                                                          such a cell                              -> lv_cell_terms, lv_own_scale
//   alpharat/nn/architectures/local_value/loss.py:55-59    the third term, ownership_weight * loss_ownership -> lv_own_scale
// and what loss.backward() then leaves in the logits' gradient. The trunk, the three heads, their loss terms and BatchNorm
// are dev_train.h's; the maximum, the exponentials and the order of their sum are dev_ownership.h's, the validation pass's.
// Plain C++ with no barrier, no reduction and no HIP call, as dev_train.h: tests/hostsim_train_lv compiles this text.
#pragma once
#include "dev_ownership.h"
#include "dev_train.h"

namespace ar {

// What every active cell's gradient is scaled by: ownership_weight / C, C the number of active cells of the window. C = 0
// is the reference's early return: the loss is a constant 0.0 there, so nothing flows back and the scale is 0.
AR_HD float lv_own_scale(float ow, uint32_t cells) { return cells ? ow / (float)cells : 0.0f; }

// the window's loss_ownership from the sum of its active cells' ce
AR_HD double lv_own_loss(double ce_sum, uint32_t cells) { return cells ? ce_sum / (double)cells : 0.0; }

// One cell from its four logits: ce = logsumexp(l) - l[target] and dl_k = scale * (softmax(l)_k - [k == target]). A cell
// with target < 0 is not active: ce = 0 and dl = 0 exactly, whatever its logits are.
AR_HD void lv_cell_terms(float l0, float l1, float l2, float l3, int target, float scale, float& ce, float* dl) {
    if (target < 0) {
        ce = 0.0f;
        dl[0] = dl[1] = dl[2] = dl[3] = 0.0f;
        return;
    }
    const float m = own_cell_max(l0, l1, l2, l3);
    const float e0 = expf(l0 - m), e1 = expf(l1 - m), e2 = expf(l2 - m), e3 = expf(l3 - m);
    float ev;
    own_cell_finish(l0, l1, l2, l3, e0, e1, e2, e3, m, target, ce, ev);
    const float s = ((e0 + e1) + e2) + e3;
    dl[0] = scale * (e0 / s - (target == 0 ? 1.0f : 0.0f));
    dl[1] = scale * (e1 / s - (target == 1 ? 1.0f : 0.0f));
    dl[2] = scale * (e2 / s - (target == 2 ? 1.0f : 0.0f));
    dl[3] = scale * (e3 / s - (target == 3 ? 1.0f : 0.0f));
}

// The fixed partition of the window's rows for the two kernels that walk its cells: B consecutive parts of rpb rows, the
// last one maybe shorter. As train_cols, a function of the row count alone.
enum { LV_MAX_BLOCKS = 1024, LV_MIN_ROWS = 16 };
struct LvCells {
    int n, hw, B, rpb;
};
inline LvCells lv_cells(int n, int hw) {
    LvCells t;
    t.n = n;
    t.hw = hw;
    t.B = (n + LV_MIN_ROWS - 1) / LV_MIN_ROWS < LV_MAX_BLOCKS ? (n + LV_MIN_ROWS - 1) / LV_MIN_ROWS : LV_MAX_BLOCKS;
    t.rpb = (n + t.B - 1) / t.B;
    t.B = (n + t.rpb - 1) / t.rpb;
    return t;
}

}  // namespace ar
