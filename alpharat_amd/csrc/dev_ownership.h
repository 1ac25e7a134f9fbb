// The ownership loss of the local_value architecture (LocalValueMLP) over stored positions: what the reference's validation
// pass adds for that architecture, as the terms of one cell and of one row.
//   alpharat/nn/losses/ownership.py:26-46      compute_ownership_loss: cross-entropy over the cells with
//                                              cheese_outcomes >= 0                                     -> ce, cells
//   alpharat/nn/models/local_value.py:186-193  ownership_value = sum over the cheese mask of
//                                              softmax(logits) . [1, 0, 0, -1]                          -> value
//
// The row rule. Cell c of a stored position is active iff the position still has the cheese (st_has_cheese): that is where
// rows_build_row writes the game's outcome, and -1 elsewhere. Its target is the game's outcomes[c]. A row's ce and value are
// the sums of its active cells' terms in increasing cell order, accumulated in double; cells counts the active cells. The
// order is fixed so that the same request gives the same bytes and the CPU harness under tests/hostsim_ownership can compare
// bit for bit what it computes with the same text.
//
// k_own_mfma (nets_ownership.h) computes a cell's four exponentials in the four lanes that hold its logits and hands them
// to own_cell_finish; own_cell_terms is the same arithmetic for one caller. No barrier and no reduction in this file.
#pragma once
#include "dev_rows.h"

namespace ar {

// Scalars, not arrays: the four values of a cell stay in registers whatever the caller holds them in.
// max of the four logits, taken in index order
AR_HD float own_cell_max(float l0, float l1, float l2, float l3) {
    float m = l0;
    m = l1 > m ? l1 : m;
    m = l2 > m ? l2 : m;
    m = l3 > m ? l3 : m;
    return m;
}

// From the logits l, their maximum m and e_k = expf(l_k - m): ce = logsumexp(l) - l[target] (F.cross_entropy with a class
// target) and ev = p[0] - p[3] with p = softmax(l) (the reference's (softmax . [1, 0, 0, -1]).sum()). A target outside
// 0..3 is read as 0, as the reference's clamp(min=0) reads -1; stored outcomes are 0..3.
AR_HD void own_cell_finish(float l0, float l1, float l2, float l3, float e0, float e1, float e2, float e3, float m, int target,
                           float& ce, float& ev) {
    const float s = ((e0 + e1) + e2) + e3;
    const float lse = m + logf(s);
    float lt = l0;
    lt = target == 1 ? l1 : lt;
    lt = target == 2 ? l2 : lt;
    lt = target == 3 ? l3 : lt;
    ce = lse - lt;
    ev = e0 / s - e3 / s;
}

// f32 log-softmax with expf / logf, as val_policy_terms
AR_HD void own_cell_terms(const float l[4], int target, float& ce, float& ev) {
    const float m = own_cell_max(l[0], l[1], l[2], l[3]);
    own_cell_finish(l[0], l[1], l[2], l[3], expf(l[0] - m), expf(l[1] - m), expf(l[2] - m), expf(l[3] - m), m, target, ce, ev);
}

// the target of cell c of a stored position, -1 where the cell is not active
template <int NW>
AR_HD int own_cell_target(const State<NW>& st, const uint8_t* outcomes, int c) {
    return st_has_cheese(st, c) ? (int)outcomes[c] : -1;
}

struct OwnRow {
    double ce, value;
    uint32_t cells;
};

AR_HD void own_row_clear(OwnRow& r) {
    r.ce = 0.0;
    r.value = 0.0;
    r.cells = 0u;
}

// one active cell's terms, added in cell order
AR_HD void own_row_add(OwnRow& r, float ce, float ev) {
    r.ce += (double)ce;
    r.value += (double)ev;
    r.cells += 1u;
}

// the whole row by one caller: logits [hw][4], the game's outcomes [hw]
template <int NW>
AR_HD OwnRow own_row_terms(const PosRec<NW>& rec, const uint8_t* outcomes, const float* logits, int hw) {
    OwnRow r;
    own_row_clear(r);
    for (int c = 0; c < hw; ++c) {
        const int t = own_cell_target<NW>(rec.st, outcomes, c);
        if (t < 0) continue;
        float ce, ev;
        own_cell_terms(logits + 4 * c, t, ce, ev);
        own_row_add(r, ce, ev);
    }
    return r;
}

}  // namespace ar
