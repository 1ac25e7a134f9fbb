// The per-element arithmetic of one training step of PyRatMLP (train_mlp.h): what the reference computes with
//   alpharat/nn/models/mlp.py              PyRatMLP.forward, BatchNorm1d in training mode        -> train_bn_forward
//   alpharat/nn/architectures/mlp/loss.py  compute_mlp_losses and the backward of its terms      -> train_head_terms
//   torch's batch-norm backward                                                                  -> train_bn_backward
// Plain C++ with no barrier, no reduction and no HIP call: the kernels of train_mlp.h call these functions, and the CPU
// harness under tests/hostsim_train compiles the same text. Every function is f32 in and f32 out; the sums over the batch
// that they take as arguments (mean, variance, the two backward column sums) are formed by the kernels in double. The
// column's mean stays a double: z - mu is then exact before it is rounded once, so the xhat of a column sum to zero as
// well as their own rounding allows. With the mean rounded to f32 first, every xhat of the column would carry the same
// error, rstd times that rounding, which the backward multiplies by rstd once more -- visible in the gradients of a column
// whose batch variance is near eps.
#pragma once
#include "dev_rng.h"

namespace ar {

#define AR_TRAIN_BN_EPS 1e-5f

// what a BatchNorm column needs of its batch statistics: the mean and 1 / sqrt(var + eps), var the biased (centred) one
AR_HD float train_bn_rstd(float var) { return 1.0f / sqrtf(var + AR_TRAIN_BN_EPS); }

AR_HD float train_bn_centred(float z, double mu) { return (float)((double)z - mu); }
AR_HD float train_bn_xhat(float z, double mu, float rstd) { return train_bn_centred(z, mu) * rstd; }

// xhat = (z - mu) * rstd;  y = gamma * xhat + beta. The activation is max(y, 0); its mask is y > 0.
AR_HD float train_bn_forward(float z, double mu, float rstd, float gamma, float beta, float& xhat) {
    xhat = train_bn_xhat(z, mu, rstd);
    return gamma * xhat + beta;
}

// dz of one element from dy (already masked by the ReLU), the element's xhat and the column's means over the batch
// mean_dy = mean(dy), mean_dy_xhat = mean(dy * xhat):
//   dxhat = dy * gamma;  dz = rstd * (dxhat - mean(dxhat) - xhat * mean(dxhat * xhat))
// with gamma taken out of the bracket. dy - mean(dy) is formed first: it is what cancels over the column, and subtracting
// before any scaling keeps that cancellation as good as the rounding of the mean allows (the column sum of dz, which is the
// gradient of the bias in front of the BatchNorm, is then noise of that size and no larger).
AR_HD float train_bn_backward(float dy, float xhat, float rstd, float gamma, float mean_dy, float mean_dy_xhat) {
    return (gamma * rstd) * ((dy - mean_dy) - xhat * mean_dy_xhat);
}

// The heads' outputs of one row: the five logits of either player, the two raw value outputs `o`.
struct TrainHeadTerms {
    float ce[2];     // -sum_k t_k log_softmax(l)_k
    float v[2];      // softplus(o), torch's threshold: v = o above 20
    float sq[2];     // (v - y)^2
    float dout[12];  // d loss / d (l1[0..5], l2[0..5], o[0..2])
};

// one player's policy term: dl_k = pw_n * (softmax(l)_k * sum_j t_j - t_k), pw_n = policy_weight / n
AR_HD void train_policy_terms(const float* l, const float* t, float pw_n, float& ce, float* dl) {
    float m = l[0];
    for (int k = 1; k < 5; ++k) m = l[k] > m ? l[k] : m;
    float e[5], s = 0.0f, ts = 0.0f;
    for (int k = 0; k < 5; ++k) {
        e[k] = expf(l[k] - m);
        s += e[k];
        ts += t[k];
    }
    const float lse = m + logf(s);
    float c = 0.0f;
    for (int k = 0; k < 5; ++k) {
        c += t[k] * (l[k] - lse);
        dl[k] = pw_n * ((e[k] / s) * ts - t[k]);
    }
    ce = -c;
}

// one player's value term: do = vw_n * (v - y) * sigmoid(o), vw_n = value_weight / n (loss_value is the mean of the two
// players' means, so each squared error carries 0.5 * 2 = 1 of it); above the threshold the derivative of v is 1
AR_HD void train_value_terms(float o, float y, float vw_n, float& v, float& sq, float& d_o) {
    const bool lin = o > 20.0f;
    v = lin ? o : log1pf(expf(o));
    const float d = v - y;
    sq = d * d;
    const float sg = lin ? 1.0f : 1.0f / (1.0f + expf(-o));
    d_o = vw_n * d * sg;
}

// out[12]: l1, l2, o as the heads give them; t1, t2: target policies; y1, y2: target values
AR_HD TrainHeadTerms train_head_terms(const float* out, const float* t1, const float* t2, float y1, float y2, float pw_n,
                                      float vw_n) {
    TrainHeadTerms h;
    train_policy_terms(out, t1, pw_n, h.ce[0], h.dout);
    train_policy_terms(out + 5, t2, pw_n, h.ce[1], h.dout + 5);
    train_value_terms(out[10], y1, vw_n, h.v[0], h.sq[0], h.dout[10]);
    train_value_terms(out[11], y2, vw_n, h.v[1], h.sq[1], h.dout[11]);
    return h;
}

// The two fixed partitions of a step. They set the order of every sum over the batch, and with it every byte of the
// gradients: a function of the row count alone, never of the device or the launch.
enum { TG_KC = 16, TRAIN_MAX_PARTS = 32, TRAIN_MAX_SPLITS = 32 };

// of a BatchNorm call's n rows for the column kernels: P consecutive parts of rpp rows, the last one maybe shorter
struct TrainCols {
    int n, H, P, rpp;
};
inline TrainCols train_cols(int n, int H) {
    TrainCols t;
    t.n = n;
    t.H = H;
    t.P = (n + 63) / 64 < TRAIN_MAX_PARTS ? (n + 63) / 64 : TRAIN_MAX_PARTS;
    t.rpp = (n + t.P - 1) / t.P;
    t.P = (n + t.rpp - 1) / t.rpp;
    return t;
}

// of the rows a product is reduced over (k_train_gemm's blockIdx.z): S ranges of kps rows, kps a multiple of the k chunk
struct TrainSplit {
    int S, kps;
};
inline TrainSplit train_split(int rows) {
    TrainSplit s;
    s.S = (rows + 255) / 256 < TRAIN_MAX_SPLITS ? (rows + 255) / 256 : TRAIN_MAX_SPLITS;
    s.kps = ((rows + s.S - 1) / s.S + TG_KC - 1) / TG_KC * TG_KC;
    s.S = (rows + s.kps - 1) / s.kps;
    return s;
}

}  // namespace ar
