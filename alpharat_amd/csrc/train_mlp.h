// One training step of PyRatMLP (alpharat/nn/models/mlp.py, BatchNorm in training mode, dropout when asked for) over a
// window of the row set's order: the forward, the losses of alpharat/nn/architectures/mlp/loss.py and what
// loss.backward() leaves in the fourteen .grad tensors, f32 throughout. The per-element arithmetic is dev_train.h; this
// file holds the kernels.
//
// The chain of one step, every launch on the caller's stream. rows_grad_mlp in alpharat_hip.hip is this listing as calls;
// the checks, the workspace, the stream rule and the launches themselves are TrainStep's, shared with train_sym.h:
//   k_rows_batch                X and the targets of the window, by the row routine the batches use (dev_rows.h)
//   k_train_gemm                Z1 = X W0^T + b0
//   k_train_colsum<SUM, SQ>     column sums of Z1, then of (Z1 - mu)^2: the centred two-pass variance
//   k_train_bn_apply            A1 = relu(bn(Z1)); the column's mu and rstd; the running statistics
//   ... the same four for Z2 = A1 W4^T + b4 and A2
//   k_train_heads               the twelve head outputs of a row, its loss terms and dOut; loss partial sums per block
//   k_train_loss_sum            the six losses
//   k_train_gemm (split)        dOut^T A2 and the column sums of dOut, per row range
//   k_train_reduce              the row ranges added in order: the six head gradients
//   k_train_colsum<DHEAD>       dY2 = (dOut Wh) masked by the ReLU, and the column sums of dY2 and dY2 * xhat
//   k_train_bn_bwd              dZ2 in place; trunk.5's two gradients
//   k_train_gemm (split), k_train_reduce   dZ2^T A1: trunk.4's two gradients
//   k_train_gemm                dA1 = dZ2 W4
//   k_train_colsum<DTRUNK>, k_train_bn_bwd dZ1 in place; trunk.1's two gradients
//   k_train_gemm (split), k_train_reduce   dZ1^T X: trunk.0's two gradients
// With dropout (ar_rows_grad_mlp_dropout) the chain is the same 23 launches: k_train_bn_apply_drop stands where
// k_train_bn_apply did and multiplies the kept elements of A by 1 / (1 - p) as it writes them, 0 for the dropped ones
// (dev_dropout.h: a hash of (seed, step, BatchNorm call, row, column), no mask stored), and the DROP forms of
// k_train_colsum<DHEAD> and <DTRUNK> multiply dA by the same scale before the mask they already read off A.
// 23 launches. Fusing the column sums into the products' epilogues and the BatchNorm arithmetic into their load side
// would shorten the chain; the first layer could also use the evaluators' sparse-operand shortcut.
//
// trunk.0.bias and trunk.4.bias sit in front of a BatchNorm, which removes any constant added to its input: their true
// gradient is zero. What is written is the honest column sum of dZ, i.e. rounding noise of the size torch writes too.
//
// Matrix products. All three shapes -- In W^T, dOut W and dOut^T In -- are k_train_gemm with other strides: C[m][n] =
// sum_k A(m, k) B(k, n) on __builtin_amdgcn_mfma_f32_32x32x2f32 (full f32 operands, f32 accumulation, products summed in
// increasing k). A block of four wavefronts owns a 64 x 64 tile of C, a wavefront a 32 x 32 quarter; the operands of 16
// values of k are staged in LDS as [k][64 + 1] (8.3 KB: many blocks share a CU), with zeros beyond M, N and the end of the
// k range, so every tail costs no branch in the inner loop. A product that reduces over the batch is split over fixed
// ranges of rows (blockIdx.z); every range writes its own partial C and k_train_reduce adds them in range order in double.
//
// Determinism: no atomics anywhere. Every sum over the batch is taken over a partition that depends only on (n, H, D)
// (train_cols and train_split, dev_train.h), each part in a fixed order, the parts combined in index order: the same
// request gives the same bytes.
#pragma once
#include "dev_dropout.h"
#include "dev_rows.h"
#include "dev_train.h"

namespace ar {

typedef float tr_f32x16 __attribute__((ext_vector_type(16)));

enum { TG_TILE = 64, TG_LD = TG_TILE + 1, TG_THREADS = 256, TRAIN_HEAD_ROWS = 64, TRAIN_MAX_ROWS = 65536 };  // TG_KC: dev_train.h

// C[m][n] = sum_{k in the block's range} A(m, k) B(k, n) (+ bias[n]); A(m, k) = a[m * sam + k * sak], B(k, n) =
// b[k * sbk + n * sbn]. blockIdx.z takes k from z * k_per_split and writes C at c + z * c_split. a_kfast / b_kfast: the
// operand is contiguous in k (else in m / n); it only chooses which neighbour lanes load. colsum (may be null):
// [splits][M], the sums over the range's k of A(m, k), written by the blocks of the first column tile.
struct TrainGemm {
    const float *a, *b, *bias;
    float *c, *colsum;
    int M, N, K, k_per_split, ldc;
    long sam, sak, sbk, sbn;
    size_t c_split;
    int a_kfast, b_kfast;
};

__global__ void __launch_bounds__(TG_THREADS) k_train_gemm(TrainGemm g) {
    __shared__ float As[TG_KC][TG_LD], Bs[TG_KC][TG_LD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.y * TG_TILE, n0 = blockIdx.x * TG_TILE;
    const int k_begin = blockIdx.z * g.k_per_split;
    const int k_end = g.K - k_begin < g.k_per_split ? g.K : k_begin + g.k_per_split;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    tr_f32x16 c;
#pragma unroll
    for (int v = 0; v < 16; ++v) c[v] = 0.0f;
    double cs = 0.0;
    // the chunk's operands go through registers: the next chunk's global loads are in flight under this chunk's MFMAs
    constexpr int PER = TG_TILE * TG_KC / TG_THREADS;
    float ra[PER], rb[PER];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int e = tid + TG_THREADS * i;
            const int ka = g.a_kfast ? (e & (TG_KC - 1)) : (e >> 6), mm = g.a_kfast ? (e >> 4) : (e & (TG_TILE - 1));
            const int kb = g.b_kfast ? (e & (TG_KC - 1)) : (e >> 6), nn = g.b_kfast ? (e >> 4) : (e & (TG_TILE - 1));
            const int gm = m0 + mm, gn = n0 + nn;
            ra[i] = (gm < g.M && k0 + ka < k_end) ? g.a[(long)gm * g.sam + (long)(k0 + ka) * g.sak] : 0.0f;
            rb[i] = (gn < g.N && k0 + kb < k_end) ? g.b[(long)(k0 + kb) * g.sbk + (long)gn * g.sbn] : 0.0f;
        }
    };
    if (k_begin < k_end) fetch(k_begin);
    for (int k0 = k_begin; k0 < k_end; k0 += TG_KC) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int e = tid + TG_THREADS * i;
            const int ka = g.a_kfast ? (e & (TG_KC - 1)) : (e >> 6), mm = g.a_kfast ? (e >> 4) : (e & (TG_TILE - 1));
            const int kb = g.b_kfast ? (e & (TG_KC - 1)) : (e >> 6), nn = g.b_kfast ? (e >> 4) : (e & (TG_TILE - 1));
            As[ka][mm] = ra[i];
            Bs[kb][nn] = rb[i];
        }
        __syncthreads();
        if (k0 + TG_KC < k_end) fetch(k0 + TG_KC);
#pragma unroll
        for (int kk = 0; kk < TG_KC; kk += 2)
            c = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + h][wm + r], Bs[kk + h][wn + r], c, 0, 0, 0);
        if (g.colsum && tid < TG_TILE)
            for (int kk = 0; kk < TG_KC; ++kk) cs += (double)As[kk][tid];
        __syncthreads();
    }
    float* cz = g.c + (size_t)blockIdx.z * g.c_split;
    const int col = n0 + wn + r;
    if (col < g.N) {
        const float bias = g.bias ? g.bias[col] : 0.0f;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int row = m0 + wm + (v & 3) + 8 * (v >> 2) + 4 * h;
            if (row < g.M) cz[(size_t)row * g.ldc + col] = c[v] + bias;
        }
    }
    if (g.colsum && blockIdx.x == 0 && tid < TG_TILE && m0 + tid < g.M)
        g.colsum[(size_t)blockIdx.z * g.M + m0 + tid] = (float)cs;
}

// The split partial products and partial column sums added in split order, in double, into up to three destinations: the
// rows of C are cut into consecutive segments of rows[0], rows[1], rows[2] rows (the three heads; one segment otherwise).
// The M bias lanes always run: a product without a bias (the convolutions of train_cnn.h) points bpart at any S * M readable
// floats and b[0] at M floats of scratch.
struct TrainReduce {
    const float *wpart, *bpart;  // [S][M][N], [S][M]
    int S, M, N;
    float *w[3], *b[3];
    int rows[3];
};

__global__ void __launch_bounds__(256) k_train_reduce(TrainReduce t) {
    const size_t wn = (size_t)t.M * t.N, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= wn + (size_t)t.M) return;
    const bool is_w = i < wn;
    const size_t j = is_w ? i : i - wn;
    const float* part = is_w ? t.wpart : t.bpart;
    const size_t stride = is_w ? wn : (size_t)t.M;
    double s = 0.0;
    for (int k = 0; k < t.S; ++k) s += (double)part[(size_t)k * stride + j];
    int row = (int)(is_w ? j / (size_t)t.N : j);
    const int col = (int)(is_w ? j - (size_t)row * t.N : 0);
    int seg = 0;
    while (seg < 2 && row >= t.rows[seg]) row -= t.rows[seg++];
    if (is_w) t.w[seg][(size_t)row * t.N + col] = (float)s;
    else t.b[seg][row] = (float)s;
}

// A layer's [n][H] arrays for the column kernels (TrainCols, dev_train.h): grid (ceil(H / 64), P); block (p) takes rows
// p * rpp .. of 64 columns with four rows in flight (thread = column + 64 * (row & 3)).
__device__ inline double train_col_total(const double* part, int P, int H, int col) {
    double s = 0.0;
    for (int p = 0; p < P; ++p) s += part[(size_t)p * H + col];
    return s;
}

// TC_DHEAD_ADD (train_lv.h): DHEAD with what another consumer of the activation already left in d added before the mask
enum { TC_SUM = 0, TC_SQ = 1, TC_DHEAD = 2, TC_DTRUNK = 3, TC_DHEAD_ADD = 4 };
struct TrainColArgs {
    const float* z;        // SUM, SQ, DHEAD, DTRUNK: the layer's pre-BatchNorm values
    const float* act;      // DHEAD, DTRUNK: relu(bn(z)), whose sign is the mask
    float* d;              // DHEAD: dY written; DTRUNK: dA masked in place; DHEAD_ADD: the other part of dA in, dY out
    const float* dout;     // DHEAD: [n][12]
    const float *w_p1, *w_p2, *w_v;  // DHEAD: the head weights
    const double* sum_in;  // SQ: the partial sums of z
    const double* mu;      // DHEAD, DTRUNK: the column's mean
    const float* rstd;     // DHEAD, DTRUNK: and 1 / sqrt(var + eps)
    double *part0, *part1;   // [P][H]
    float scale;           // DROP: 1 / (1 - p) of the dropout behind the activation
};

// DROP: the activation went through dropout (dev_dropout.h), so dy = dA * a.scale before the mask; act > 0 is then the
// combined mask of the ReLU and the dropout, since a dropped element is exactly 0 and a kept positive one stays positive.
// DHEAD_ADD scales the sum of both consumers' gradients.
template <int MODE, bool DROP = false>
__global__ void __launch_bounds__(256) k_train_colsum(TrainCols t, TrainColArgs a) {
    static_assert(!DROP || MODE >= TC_DHEAD, "the forward's column sums see no dropout");
    __shared__ double s0[4][64], s1[4][64];
    const int c = threadIdx.x & 63, sub = threadIdx.x >> 6, col = blockIdx.x * 64 + c;
    const int r0 = blockIdx.y * t.rpp, r1 = t.n - r0 < t.rpp ? t.n : r0 + t.rpp;
    double acc0 = 0.0, acc1 = 0.0;
    if (col < t.H) {
        double mu = 0.0;
        float rstd = 0.0f, w[12];
        if (MODE == TC_SQ) mu = train_col_total(a.sum_in, t.P, t.H, col) / (double)t.n;
        if (MODE >= TC_DHEAD) {
            mu = a.mu[col];
            rstd = a.rstd[col];
        }
        if (MODE == TC_DHEAD || MODE == TC_DHEAD_ADD) {
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                w[k] = a.w_p1[(size_t)k * t.H + col];
                w[5 + k] = a.w_p2[(size_t)k * t.H + col];
            }
            w[10] = a.w_v[col];
            w[11] = a.w_v[t.H + col];
        }
        for (int r = r0 + sub; r < r1; r += 4) {
            const size_t i = (size_t)r * t.H + col;
            const float z = a.z[i];
            if (MODE == TC_SUM) acc0 += (double)z;
            else if (MODE == TC_SQ) {
                const float d = train_bn_centred(z, mu);
                acc0 += (double)d * (double)d;
            } else {
                float dy;
                if (MODE == TC_DHEAD || MODE == TC_DHEAD_ADD) {
                    const float* o = a.dout + (size_t)r * 12;
                    dy = 0.0f;
#pragma unroll
                    for (int k = 0; k < 12; ++k) dy += o[k] * w[k];
                    if (MODE == TC_DHEAD_ADD) dy += a.d[i];
                } else
                    dy = a.d[i];
                if (DROP) dy *= a.scale;
                dy = a.act[i] > 0.0f ? dy : 0.0f;
                a.d[i] = dy;
                const float xhat = train_bn_xhat(z, mu, rstd);
                acc0 += (double)dy;
                acc1 += (double)dy * (double)xhat;
            }
        }
    }
    s0[sub][c] = acc0;
    s1[sub][c] = acc1;
    __syncthreads();
    if (sub == 0 && col < t.H) {
        a.part0[(size_t)blockIdx.y * t.H + col] = ((s0[0][c] + s0[1][c]) + s0[2][c]) + s0[3][c];
        if (MODE >= TC_DHEAD) a.part1[(size_t)blockIdx.y * t.H + col] = ((s1[0][c] + s1[1][c]) + s1[2][c]) + s1[3][c];
    }
}

// act = relu(bn(z)) with the batch's statistics from the partial sums; the first row block also keeps mu and rstd for the
// backward and updates the running statistics (momentum 0.1, the unbiased variance), when they are given.
// DROP: inverted dropout on top, act = keep(row * H + column) ? relu(bn(z)) * scale : 0 (dev_dropout.h); nothing is stored.
template <bool DROP>
__device__ __forceinline__ void train_bn_apply(const TrainCols& t, const float* z, const double* part_sum, const double* part_sq,
                                               const float* gamma, const float* beta, float* act, double* mu_out,
                                               float* rstd_out, float* run_mean, float* run_var, const TrainDrop& dr) {
    const int c = threadIdx.x & 63, sub = threadIdx.x >> 6, col = blockIdx.x * 64 + c;
    if (col >= t.H) return;
    const double mean = train_col_total(part_sum, t.P, t.H, col) / (double)t.n;
    const double var = train_col_total(part_sq, t.P, t.H, col) / (double)t.n;
    const float rstd = train_bn_rstd((float)var), ga = gamma[col], be = beta[col];
    if (blockIdx.y == 0 && sub == 0) {
        mu_out[col] = mean;
        rstd_out[col] = rstd;
        if (run_mean) run_mean[col] = (float)(0.9 * (double)run_mean[col] + 0.1 * mean);
        if (run_var) run_var[col] = (float)(0.9 * (double)run_var[col] + 0.1 * (var * (double)t.n / (double)(t.n - 1)));
    }
    const int r0 = blockIdx.y * t.rpp, r1 = t.n - r0 < t.rpp ? t.n : r0 + t.rpp;
    for (int r = r0 + sub; r < r1; r += 4) {
        const size_t i = (size_t)r * t.H + col;
        float xhat;
        const float y = train_bn_forward(z[i], mean, rstd, ga, be, xhat);
        if (DROP) act[i] = (y > 0.0f && dropout_keep(dr.key, dr.thr, (uint64_t)i)) ? y * dr.scale : 0.0f;
        else act[i] = y > 0.0f ? y : 0.0f;
    }
}

__global__ void __launch_bounds__(256)
k_train_bn_apply(TrainCols t, const float* z, const double* part_sum, const double* part_sq, const float* gamma,
                 const float* beta, float* act, double* mu_out, float* rstd_out, float* run_mean, float* run_var) {
    train_bn_apply<false>(t, z, part_sum, part_sq, gamma, beta, act, mu_out, rstd_out, run_mean, run_var, TrainDrop{});
}

__global__ void __launch_bounds__(256)
k_train_bn_apply_drop(TrainCols t, const float* z, const double* part_sum, const double* part_sq, const float* gamma,
                      const float* beta, float* act, double* mu_out, float* rstd_out, float* run_mean, float* run_var,
                      TrainDrop dr) {
    train_bn_apply<true>(t, z, part_sum, part_sq, gamma, beta, act, mu_out, rstd_out, run_mean, run_var, dr);
}

// the mask of one call as k_train_bn_apply_drop forms it, element by element (ar_train_dropout_mask): keep [n][H] bytes, 1 for
// a kept element, 0 for a dropped one
__global__ void __launch_bounds__(256) k_train_dropout_mask(TrainDrop dr, uint64_t count, uint8_t* keep) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < count) keep[e] = dropout_keep(dr.key, dr.thr, e) ? 1 : 0;
}

// dz in place of the masked dy; the first row block writes dgamma = sum(dy * xhat) and dbeta = sum(dy)
__global__ void __launch_bounds__(256)
k_train_bn_bwd(TrainCols t, const float* z, float* d, const double* part_dy, const double* part_dyx, const double* mu_in,
               const float* rstd_in, const float* gamma, float* dgamma, float* dbeta) {
    const int c = threadIdx.x & 63, sub = threadIdx.x >> 6, col = blockIdx.x * 64 + c;
    if (col >= t.H) return;
    const double sdy = train_col_total(part_dy, t.P, t.H, col), sdyx = train_col_total(part_dyx, t.P, t.H, col);
    if (blockIdx.y == 0 && sub == 0) {
        dgamma[col] = (float)sdyx;
        dbeta[col] = (float)sdy;
    }
    const float mean_dy = (float)(sdy / (double)t.n), mean_dyx = (float)(sdyx / (double)t.n);
    const double mu = mu_in[col];
    const float rstd = rstd_in[col], ga = gamma[col];
    const int r0 = blockIdx.y * t.rpp, r1 = t.n - r0 < t.rpp ? t.n : r0 + t.rpp;
    for (int r = r0 + sub; r < r1; r += 4) {
        const size_t i = (size_t)r * t.H + col;
        const float xhat = train_bn_xhat(z[i], mu, rstd);
        d[i] = train_bn_backward(d[i], xhat, rstd, ga, mean_dy, mean_dyx);
    }
}

// The heads of 64 rows a block: sixteen lanes share a row's twelve dot products (lane j takes k = j, j + 16, ..., then a
// fixed xor tree), four rows after one another; the group's first lane forms the row's terms (train_head_terms) and
// writes dOut and the outputs asked for. The rows' four loss terms go through LDS and are added in row order, in double:
// one partial vector per block.
struct TrainHeads {
    const float* act;                // [n][H]
    const float *w_p1, *b_p1, *w_p2, *b_p2, *w_v, *b_v;
    const float *t1, *t2, *y1, *y2;  // targets
    float* dout;                     // [n][12]
    double* loss_part;               // [blocks][4]
    float *logits_p1, *logits_p2, *value_p1, *value_p2;  // may be null
    int n, H;
    float pw_n, vw_n;
};

__global__ void __launch_bounds__(256) k_train_heads(TrainHeads t) {
    extern __shared__ float wh[];  // [12][H]
    __shared__ float terms[TRAIN_HEAD_ROWS][4];
    const int tid = threadIdx.x, H = t.H;
    for (int i = tid; i < 12 * H; i += 256) {
        const int k = i / H, j = i - k * H;
        wh[i] = k < 5 ? t.w_p1[k * H + j] : k < 10 ? t.w_p2[(k - 5) * H + j] : t.w_v[(k - 10) * H + j];
    }
    __syncthreads();
    const int grp = tid >> 4, j16 = tid & 15;
    for (int q = 0; q < 4; ++q) {
        const int lr = grp * 4 + q, row = blockIdx.x * TRAIN_HEAD_ROWS + lr;
        const bool live = row < t.n;  // (uniform over the group)
        float o[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) o[k] = 0.0f;
        if (live) {
            const float* x = t.act + (size_t)row * H;
            for (int j = j16; j < H; j += 16) {
                const float xv = x[j];
#pragma unroll
                for (int k = 0; k < 12; ++k) o[k] += xv * wh[k * H + j];
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
                    o[k] += t.b_p1[k];
                    o[5 + k] += t.b_p2[k];
                }
                o[10] += t.b_v[0];
                o[11] += t.b_v[1];
                const TrainHeadTerms ht =
                    train_head_terms(o, t.t1 + (size_t)row * 5, t.t2 + (size_t)row * 5, t.y1[row], t.y2[row], t.pw_n, t.vw_n);
#pragma unroll
                for (int k = 0; k < 12; ++k) t.dout[(size_t)row * 12 + k] = ht.dout[k];
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

// The six losses from the blocks' partial sums: wavefront j owns term j; lane l adds partials l, l + 64, ... in order, the
// lanes are combined by a fixed tree. losses: loss_p1, loss_p2, loss_value_p1, loss_value_p2, loss_value, loss.
__global__ void __launch_bounds__(256)
k_train_loss_sum(const double* part, uint32_t n_part, uint32_t n, float pw, float vw, float* losses, float* losses_out) {
    __shared__ double tot[4];
    const uint32_t j = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    double s = 0.0;
    for (uint32_t b = lane; b < n_part; b += 64) s += part[(size_t)b * 4 + j];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) tot[j] = s / (double)n;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double value = 0.5 * (tot[2] + tot[3]);
        const double all[6] = {tot[0], tot[1], tot[2], tot[3], value, (double)pw * (tot[0] + tot[1]) + (double)vw * value};
        for (int k = 0; k < 6; ++k) {
            losses[k] = (float)all[k];
            if (losses_out) losses_out[k] = (float)all[k];
        }
    }
}

}  // namespace ar
