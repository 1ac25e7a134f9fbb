// One training step of SymmetricMLP (alpharat/nn/models/symmetric.py, BatchNorm in training mode, dropout when asked for)
// over a window of the row set's order: the forward, the losses of alpharat/nn/architectures/symmetric/loss.py and what
// loss.backward() leaves in the twenty .grad tensors, f32 throughout. The products, the column kernels and the ordered
// reductions are train_mlp.h's; the per-row arithmetic is dev_train.h and dev_train_sym.h; this file holds what the
// network adds.
//
// P1's and P2's rows are stacked as [2n][.] arrays (P1's n rows, then P2's): every layer the two players share is then one
// product over 2n rows, and every gradient of a shared weight -- the sum of its two calls' contributions, P1's before P2's --
// one batch-reduced product over 2n rows with its ordered reduction. BatchNorm never pools the two: the column kernels run on
// each half with a pointer offset, each call with its own statistics, P1's call updating the running statistics before P2's.
//
// The chain of one step, every launch on the caller's stream: rows_grad_symmetric in alpharat_hip.hip is this listing as
// calls on the TrainStep it shares with train_mlp.h's driver. "bn" is k_train_colsum<SUM>, k_train_colsum<SQ>,
// k_train_bn_apply (TrainStep::bn_forward); "bn'" is k_train_colsum<DTRUNK>, k_train_bn_bwd (bn_backward_trunk):
//    1  k_rows_batch                X and the targets of the window (dev_rows.h)
//    2  k_sym_split                 shared_raw [n], p_raw [2n]
//    3  k_train_gemm, bn            shared = relu(bn(shared_raw Ws^T + bs))                                        [n]    4
//    7  k_train_gemm, bn, bn        p = relu(bn(p_raw Wp^T + bp)), a BatchNorm call per half                       [2n]   7
//   14  k_sym_cat                   cat(shared, p_i)                                                               [2n]
//   15  k_train_gemm, bn, bn        trunk.0, trunk.1                                                               [2n]   7
//   22  k_train_gemm, bn, bn        trunk.4, trunk.5: h_1, h_2                                                     [2n]   7
//   29  k_sym_heads                 both heads over cat(h_i, h_1 + h_2), the row's loss terms, the packed dOut rows
//   30  k_train_loss_sum            the six losses
//   31  k_train_gemm (split), k_sym_head_reduce   packed dOut^T h: the four head gradients                                2
//   33  (k_sym_dhead, k_train_bn_bwd) per half    dh_i masked by the ReLU, its column sums; dZ in place                   4
//   37  k_sym_bn_grad               trunk.5's two gradients: both calls' column sums, P1's first
//   38  k_train_gemm (split), k_train_reduce      trunk.4's two gradients                                                 2
//   40  k_train_gemm                dA = dZ W4
//   41  bn', bn', k_sym_bn_grad     trunk.1's two gradients                                                               5
//   46  k_train_gemm (split), k_train_reduce      trunk.0's two gradients                                                 2
//   48  k_train_gemm                d cat = dZ W0
//   49  k_sym_uncat                 d shared = the first H columns of both halves, P1's + P2's; d p_i = the last H
//   50  bn', bn', k_sym_bn_grad     player_encoder.1's two gradients                                                      5
//   55  k_train_gemm (split), k_train_reduce      player_encoder.0's two gradients                                        2
//   57  bn'                         shared_encoder.1's two gradients (one call: k_train_bn_bwd writes them)               2
//   59  k_train_gemm (split), k_train_reduce      shared_encoder.0's two gradients                                        2
// With dropout (ar_rows_grad_symmetric_dropout) the same 60 launches: each of the seven BatchNorm calls has its own mask
// (call index 0 .. 6 in the order above, rows counted within the call's half), applied by k_train_bn_apply_drop and undone by
// the DROP forms of k_sym_dhead and k_train_colsum<DTRUNK> (train_mlp.h, dev_dropout.h).
// 60 launches. k_sym_cat and k_sym_uncat are copies that a leading dimension on the column kernels' arrays would save; so
// would everything train_mlp.h lists for its own chain.
//
// shared_encoder.0.bias, player_encoder.0.bias, trunk.0.bias and trunk.4.bias sit in front of a BatchNorm: their true gradient
// is zero, and what is written is the honest column sum of dZ, rounding noise (train_mlp.h).
//
// Determinism: as train_mlp.h. No atomics; every sum over the batch over a partition that depends only on (n, H, D), the
// parts in index order in double.
#pragma once
#include "dev_train_sym.h"
#include "train_mlp.h"

namespace ar {

// shared_raw [n][Ds] and p_raw [2n][Dp] (P1's rows, then P2's) from the flat rows x [n][D]: one thread an output element
__global__ void __launch_bounds__(256) k_sym_split(const float* x, float* xs, float* xp, int n, int hw) {
    const int D = 7 * hw + 6, Ds = sym_shared_dim(hw), Dp = sym_player_dim(hw), W = Ds + 2 * Dp;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * W) return;
    const size_t r = i / (size_t)W;
    const int j = (int)(i - r * W);
    const float* row = x + r * D;
    if (j < Ds) xs[r * Ds + j] = row[sym_shared_src(hw, j)];
    else {
        const int p = j - Ds >= Dp, k = j - Ds - p * Dp;
        xp[((size_t)p * n + r) * Dp + k] = row[sym_player_src(hw, p, k)];
    }
}

// cat [2n][2H]: row r = [shared[r mod n] | p[r]]
__global__ void __launch_bounds__(256) k_sym_cat(const float* shared, const float* p, float* cat, int n, int H) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)4 * n * H) return;
    const size_t r = i / (size_t)(2 * H);
    const int c = (int)(i - r * (2 * H));
    cat[i] = c < H ? shared[(r < (size_t)n ? r : r - n) * H + c] : p[r * H + (c - H)];
}

// dcat [2n][2H] -> dshared [n][H] = P1's first H columns + P2's, dp [2n][H] = the last H columns
__global__ void __launch_bounds__(256) k_sym_uncat(const float* dcat, float* dshared, float* dp, int n, int H) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)2 * n * H) return;
    const size_t r = i / (size_t)H;
    const int c = (int)(i - r * H);
    dp[i] = dcat[r * (2 * H) + H + c];
    if (r < (size_t)n) dshared[i] = dcat[r * (2 * H) + c] + dcat[(r + n) * (2 * H) + c];
}

// Both heads of 64 rows a block, sixteen lanes a row as k_train_heads: lane j takes k = j, j + 16, ... of h_1, h_2 and
// their sum against the six rows of Wh = [policy_head; value_head] (6, 2H) in LDS, then a fixed xor tree; the group's first
// lane forms the row's terms (train_head_terms over [l1, l2, o1, o2]), writes the outputs asked for and the two packed dOut
// rows (sym_head_pack) at rows r and n + r of d12. Loss partial sums per block, in row order, in double.
struct SymHeads {
    const float* h;                   // [2n][H]: h_1, then h_2
    const float *w_p, *b_p, *w_v, *b_v;  // (5, 2H), (5), (1, 2H), (1)
    const float *t1, *t2, *y1, *y2;   // targets
    float* d12;                       // [2n][12]
    double* loss_part;                // [blocks][4]
    float *logits_p1, *logits_p2, *value_p1, *value_p2;  // may be null
    int n, H;
    float pw_n, vw_n;
};

__global__ void __launch_bounds__(256) k_sym_heads(SymHeads t) {
    extern __shared__ float wh[];  // [6][2H]
    __shared__ float terms[TRAIN_HEAD_ROWS][4];
    const int tid = threadIdx.x, H = t.H, H2 = 2 * t.H;
    for (int i = tid; i < 6 * H2; i += 256) wh[i] = i < 5 * H2 ? t.w_p[i] : t.w_v[i - 5 * H2];
    __syncthreads();
    const int grp = tid >> 4, j16 = tid & 15;
    for (int q = 0; q < 4; ++q) {
        const int lr = grp * 4 + q, row = blockIdx.x * TRAIN_HEAD_ROWS + lr;
        const bool live = row < t.n;  // (uniform over the group)
        float o[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) o[k] = 0.0f;
        if (live) {
            const float *x1 = t.h + (size_t)row * H, *x2 = t.h + ((size_t)t.n + row) * H;
            for (int j = j16; j < H; j += 16) {
                const float a = x1[j], b = x2[j], g = a + b;
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const float wl = wh[k * H2 + j], gu = g * wh[k * H2 + H + j];
                    const int k1 = k < 5 ? k : 10, k2 = k < 5 ? 5 + k : 11;
                    o[k1] += a * wl;
                    o[k1] += gu;
                    o[k2] += b * wl;
                    o[k2] += gu;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 12; ++k)
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) o[k] += __shfl_xor(o[k], off, 16);
        if (j16 == 0) {
            float ce0 = 0.0f, ce1 = 0.0f, sq0 = 0.0f, sq1 = 0.0f;
            if (live) {
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    o[k] += t.b_p[k];
                    o[5 + k] += t.b_p[k];
                }
                o[10] += t.b_v[0];
                o[11] += t.b_v[0];
                const TrainHeadTerms ht =
                    train_head_terms(o, t.t1 + (size_t)row * 5, t.t2 + (size_t)row * 5, t.y1[row], t.y2[row], t.pw_n, t.vw_n);
                float r1[12], r2[12];
                sym_head_pack(ht.dout, r1, r2);
#pragma unroll
                for (int k = 0; k < 12; ++k) {
                    t.d12[(size_t)row * 12 + k] = r1[k];
                    t.d12[((size_t)t.n + row) * 12 + k] = r2[k];
                }
                if (t.logits_p1)
                    for (int k = 0; k < 5; ++k) t.logits_p1[(size_t)row * 5 + k] = o[k];
                if (t.logits_p2)
                    for (int k = 0; k < 5; ++k) t.logits_p2[(size_t)row * 5 + k] = o[5 + k];
                if (t.value_p1) t.value_p1[row] = ht.v[0];
                if (t.value_p2) t.value_p2[row] = ht.v[1];
                ce0 = ht.ce[0];
                ce1 = ht.ce[1];
                sq0 = ht.sq[0];
                sq1 = ht.sq[1];
            }
            terms[lr][0] = ce0;
            terms[lr][1] = ce1;
            terms[lr][2] = sq0;
            terms[lr][3] = sq1;
        }
    }
    __syncthreads();
    if (tid < 4) {
        double s = 0.0;
        for (int l = 0; l < TRAIN_HEAD_ROWS; ++l) s += (double)terms[l][tid];
        t.loss_part[(size_t)blockIdx.x * 4 + tid] = s;
    }
}

// k_train_colsum<TC_DHEAD>'s sibling for one player's half (every pointer at that half): dy = dh_i of sym_head_dy masked by
// the ReLU, written to d, and the column sums of dy and dy * xhat per row block. Grid and block as TrainCols says.
struct SymDHead {
    const float *z, *act;  // the half's pre-BatchNorm values and relu(bn(z))
    float* d;              // dy written
    const float* d12;      // the half's packed dOut rows [n][12]
    const float *w_p, *w_v;
    const double* mu;
    const float* rstd;
    double *part0, *part1;  // [P][H]
    float scale;            // DROP: 1 / (1 - p)
};

// DROP: behind trunk.7's dropout, dy = dh_i * a.scale before the mask (k_train_colsum's DROP, train_mlp.h).
template <bool DROP = false>
__global__ void __launch_bounds__(256) k_sym_dhead(TrainCols t, SymDHead a) {
    __shared__ double s0[4][64], s1[4][64];
    const int c = threadIdx.x & 63, sub = threadIdx.x >> 6, col = blockIdx.x * 64 + c;
    const int r0 = blockIdx.y * t.rpp, r1 = t.n - r0 < t.rpp ? t.n : r0 + t.rpp;
    double acc0 = 0.0, acc1 = 0.0;
    if (col < t.H) {
        const double mu = a.mu[col];
        const float rstd = a.rstd[col];
        float w_lo[6], w_hi[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const float* w = k < 5 ? a.w_p + (size_t)k * 2 * t.H : a.w_v;
            w_lo[k] = w[col];
            w_hi[k] = w[t.H + col];
        }
        for (int r = r0 + sub; r < r1; r += 4) {
            const size_t i = (size_t)r * t.H + col;
            float dy = sym_head_dy(a.d12 + (size_t)r * 12, w_lo, w_hi);
            if (DROP) dy *= a.scale;
            dy = a.act[i] > 0.0f ? dy : 0.0f;
            a.d[i] = dy;
            const float xhat = train_bn_xhat(a.z[i], mu, rstd);
            acc0 += (double)dy;
            acc1 += (double)dy * (double)xhat;
        }
    }
    s0[sub][c] = acc0;
    s1[sub][c] = acc1;
    __syncthreads();
    if (sub == 0 && col < t.H) {
        a.part0[(size_t)blockIdx.y * t.H + col] = ((s0[0][c] + s0[1][c]) + s0[2][c]) + s0[3][c];
        a.part1[(size_t)blockIdx.y * t.H + col] = ((s1[0][c] + s1[1][c]) + s1[2][c]) + s1[3][c];
    }
}

// the two gradients of a BatchNorm module called once per player: dgamma = sum(dy * xhat), dbeta = sum(dy), each call's row
// blocks in order, P1's call before P2's, in double
__global__ void __launch_bounds__(256)
k_sym_bn_grad(int P, int H, const double* dy_p1, const double* dyx_p1, const double* dy_p2, const double* dyx_p2, float* dgamma,
              float* dbeta) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= H) return;
    dgamma[col] = (float)(train_col_total(dyx_p1, P, H, col) + train_col_total(dyx_p2, P, H, col));
    dbeta[col] = (float)(train_col_total(dy_p1, P, H, col) + train_col_total(dy_p2, P, H, col));
}

// The split partial products of packed dOut^T h, [S][12][H], and partial column sums [S][12], added in split order in
// double: rows 0..5 are d Wh[:, :H], rows 6..11 d Wh[:, H:] (row 5 / 11 the value head's); the first six column sums are
// the biases' gradients, colsum(dOut_1) + colsum(dOut_2).
__global__ void __launch_bounds__(256)
k_sym_head_reduce(const float* wpart, const float* bpart, int S, int H, float* w_p, float* b_p, float* w_v, float* b_v) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 12 * H + 6) return;
    const bool is_w = i < 12 * H;
    const int j = is_w ? i : i - 12 * H;
    const size_t stride = is_w ? (size_t)12 * H : 12;
    const float* part = is_w ? wpart : bpart;
    double s = 0.0;
    for (int k = 0; k < S; ++k) s += (double)part[(size_t)k * stride + j];
    if (is_w) {
        const int m = j / H, col = j - m * H, row = m % 6, hi = m / 6;
        float* dst = row < 5 ? w_p + (size_t)row * 2 * H : w_v;
        dst[hi * H + col] = (float)s;
    } else if (j < 5) b_p[j] = (float)s;
    else b_v[0] = (float)s;
}

}  // namespace ar
