// Validation of a checkpoint over stored positions: what the reference's validation pass computes per row
// (alpharat/nn/training/loop.py:306-361: eval-mode forward, the architecture's loss, the detailed metrics), as the terms of
// one row that k_val_terms reduces to sums.
//   alpharat/nn/architectures/*/loss.py  F.cross_entropy with soft targets, F.mse_loss   -> ce, pred / target
//   alpharat/nn/metrics.py:15-31         top_k_accuracy                                  -> top1, top2
//   alpharat/nn/metrics.py:34-46         policy_entropy                                  -> ent_pred
//   alpharat/nn/metrics.py:49-62         target_entropy                                  -> ent_target
//   alpharat/nn/metrics.py:65-116        explained_variance, value_correlation           -> pred / target (moments: val_accumulate)
//
// One lane computes one row. There is no barrier and no reduction in this file, so the CPU harness under
// tests/hostsim_validate runs the same text. The terms of a row are f32; every product of two of them (squared errors,
// second and cross moments) is formed in double by val_accumulate, where it is exact.
//
// Top-k with ties. `a` is the first index of the largest target. The rank of `a` among the logits is
//     rank = #{k : l_k > l_a} + #{k < a : l_k == l_a},
// i.e. among equal logits the lower index comes first; top1 = rank < 1, top2 = rank < 2. torch.topk leaves the order among
// equal logits undefined, so for rows with an exact logit tie at l_a this rule is this library's, not the reference's.
#pragma once
#include "dev_rows.h"

namespace ar {

struct ValTerms {
    float ce[2], ent_pred[2], ent_target[2];
    uint32_t top1[2], top2[2];
    float pred[2], target[2];
};

// the terms of one player: five logits `l`, five target probabilities `t`
AR_HD void val_policy_terms(const float* l, const float* t, float& ce, float& ent_pred, float& ent_target, uint32_t& top1,
                            uint32_t& top2) {
    float m = l[0];
    for (int k = 1; k < 5; ++k) m = l[k] > m ? l[k] : m;
    float e[5], s = 0.0f;
    for (int k = 0; k < 5; ++k) {
        e[k] = expf(l[k] - m);
        s += e[k];
    }
    const float ls = logf(s);
    float c = 0.0f, hp = 0.0f, ht = 0.0f;
    for (int k = 0; k < 5; ++k) {
        // log_softmax as (l - max) - log(sum), the order torch takes: l - (max + log(sum)) rounds the sum at the size of the
        // logits, which at |l| of 100 is 4e-6 on a term that is itself -log(sum), near 0 for the largest logit
        const float lp = (l[k] - m) - ls;
        c += t[k] * lp;
        hp += (e[k] / s) * lp;
        const float tc = t[k] > 1e-8f ? t[k] : 1e-8f;
        ht += t[k] * logf(tc);
    }
    ce = -c;
    ent_pred = -hp;
    ent_target = -ht;
    // (selects, no dynamic index: the lane's values stay in registers)
    int a = 0;
    float ta = t[0];
    for (int k = 1; k < 5; ++k)
        if (t[k] > ta) {
            ta = t[k];
            a = k;
        }
    float la = l[0];
    for (int k = 1; k < 5; ++k) la = k == a ? l[k] : la;
    uint32_t rank = 0;
    for (int k = 0; k < 5; ++k) rank += (l[k] > la || (k < a && l[k] == la)) ? 1u : 0u;
    top1 = rank < 1u ? 1u : 0u;
    top2 = rank < 2u ? 1u : 0u;
}

// `logits`: P1's five, then P2's five; v1, v2: the evaluator's values (softplus). The value targets are
// final score - score at the position, the f32 subtraction of rows_build_row.
template <int NW>
AR_HD ValTerms val_row_terms(const PosRec<NW>& rec, const RowGame& g, const float logits[10], float v1, float v2) {
    ValTerms t;
    for (int p = 0; p < 2; ++p)
        val_policy_terms(logits + 5 * p, rec.res.policy[p], t.ce[p], t.ent_pred[p], t.ent_target[p], t.top1[p], t.top2[p]);
    t.pred[0] = v1;
    t.pred[1] = v2;
    t.target[0] = g.final1 - rec.st.s1;
    t.target[1] = g.final2 - rec.st.s2;
    return t;
}

// The sums of ArValSums as one vector: for player p the nine doubles
//   ce, sq_err, ent_pred, ent_target, sum_pred, sum_target, sum_pred2, sum_target2, sum_pred_target
// at d[9 * p ..], and the counts top1[2], top2[2].
enum { VAL_D_PER_PLAYER = 9, VAL_N_DOUBLE = 18, VAL_N_COUNT = 4 };
struct ValAcc {
    double d[VAL_N_DOUBLE];
    uint64_t c[VAL_N_COUNT];
};

AR_HD void val_accumulate(ValAcc& acc, const ValTerms& t) {
    for (int p = 0; p < 2; ++p) {
        double* d = acc.d + VAL_D_PER_PLAYER * p;
        const double v = (double)t.pred[p], y = (double)t.target[p];
        d[0] += (double)t.ce[p];
        d[1] += (v - y) * (v - y);
        d[2] += (double)t.ent_pred[p];
        d[3] += (double)t.ent_target[p];
        d[4] += v;
        d[5] += y;
        d[6] += v * v;
        d[7] += y * y;
        d[8] += v * y;
        acc.c[p] += t.top1[p];
        acc.c[2 + p] += t.top2[p];
    }
}

}  // namespace ar
