// One training step of PyRatCNN (alpharat/nn/models/cnn/model.py as CNNModelConfig builds it by default: a stem, B
// pre-activation ResBlocks, the DeepSet heads; BatchNorm2d in training mode, dropout 0) over a window of the row set's order:
// the forward, the losses of alpharat/nn/architectures/cnn/loss.py and what loss.backward() leaves in the 11 + 6 B .grad
// tensors, f32 throughout. The column kernels, the products of the Linear layers and the ordered reductions are
// train_mlp.h's, the heads train_sym.h's; the per-element arithmetic is dev_train.h, dev_train_sym.h and dev_train_cnn.h;
// this file holds what the network adds: the 3x3 convolution and the small kernels around the player cells.
//
// Layout. Every trunk activation is channels-last, [R][C] with R = n hw and row m = row * hw + cell, cell = y * w + x:
// BatchNorm2d over (N, H, W) is then the column statistics of an [R][C] array, which k_train_colsum, k_train_bn_apply and
// k_train_bn_bwd take as they are under the partition cnn_cols gives (dev_train_cnn.h). Its up to 256 parts are collapsed
// to one row of totals in index order, in double (k_cnn_collapse), before a column kernel needs them: the kernels are then
// launched with P = 1 in their TrainCols and the partition's grid, and no thread walks 256 partial sums. The sum is the
// one train_col_total would have formed, term for term.
//
// The chain of one step, every launch on the caller's stream: rows_grad_cnn in alpharat_hip.hip is this listing as calls
// on the TrainStep it shares with the other drivers. "bn" is k_train_colsum<SUM>, k_cnn_collapse, k_train_colsum<SQ>,
// k_cnn_collapse, k_train_bn_apply (5); "bn'" is k_train_colsum<DTRUNK>, k_cnn_collapse, k_train_bn_bwd (3); "conv", "conv^T"
// and "conv dW" are k_train_conv3<CV_FWD>, <CV_DIN> and <CV_DW>, the last one followed by k_train_reduce:
//    k_rows_batch                 X and the targets of the window (dev_rows.h)
//    k_cnn_split                  the stem's input [R][5], the side vectors [2n][3], the player cells [2n]
//    conv, bn                     x_0 = relu(stem_bn(stem(in)))                                                     6
//    per block b:                 bn (a = relu(bn1(x_b))), conv (z = conv1(a)), bn (a' = relu(bn2(z))),
//                                 conv with the skip added as it stores (x_b+1 = conv2(a') + x_b)                 12
//    k_train_gemm                 the side vectors through player_encoder.0                                       [2n]
//    k_cnn_gather                 cat(x_B at the player's cell, relu(encoder))                                    [2n][C + PD]
//    k_train_gemm, k_train_lv_relu   h_1, h_2 = relu(combiner.0(cat))                                             [2n][HD]
//    k_sym_heads, k_train_loss_sum   both heads over cat(h_i, h_1 + h_2), the packed dOut rows; the six losses
//    k_train_gemm (split), k_sym_head_reduce    the four head gradients
//    k_cnn_dhead                  dZc = dh_i masked by the ReLU (k_sym_dhead without a BatchNorm)
//    k_train_gemm (split), k_train_reduce       combiner.0's two gradients
//    k_train_gemm                 dcat = dZc Wc
//    k_cnn_enc_bwd                dZe = dcat[:, C:] masked by the encoder's ReLU
//    k_train_gemm (split), k_train_reduce       player_encoder.0's two gradients
//    k_cnn_scatter                g = d x_B: dcat[:, :C] of P1 and then of P2 at their cells, zero elsewhere
//    per block b, downwards:      conv dW (conv2), conv^T, bn' (bn2), conv dW (conv1), conv^T, bn' (bn1),
//                                 k_cnn_add (g = g + that)                                                        13
//    bn' (stem_bn), conv dW (stem)                                                                                 5
// (A GPoolResBlock's pool path and the dropout behind the two ReLUs of the heads are train_gpool.h, over ar_rows_grad_cnn_gpool:
// the chain above is that function's with no gpool block and no dropout.)
// 29 + 25 B launches: 104 at B = 3. Fusing the column sums into the convolution's epilogue and the BatchNorm into its
// operand fetch would take most of the "bn" launches and a read and a write of [R][C] each out of the chain.
//
// The 3x3 convolution is an implicit GEMM with k_train_gemm's tile scheme: a block of four wavefronts owns a 64 x 64 tile of
// C, a wavefront a 32 x 32 quarter on __builtin_amdgcn_mfma_f32_32x32x2f32; 16 values of k are staged in LDS through
// registers, so the next chunk's loads fly under this chunk's MFMAs; zeros past M, N and the end of the k range; products
// summed in increasing k. The 3x3 neighbourhood is resolved as the operand is fetched (cnn_nbr): no im2col array exists.
//   CV_FWD  out[m][co]  = sum_k A(m, k) W(k, co),    k = tap * Cin + ci:   A = in[nbr(m, tap)][ci], 0 off the board
//   CV_DIN  dIn[m][ci]  = sum_k A(m, k) W(k, ci),    k = tap * Cout + co:  A = dOut[nbr(m, mirror(tap))][co]
//   CV_DW   dW[co][j]   = sum_m dOut[m][co] B(m, j), j = ci * 9 + tap:     B = in[nbr(m, tap)][ci]; torch's [Cout][Cin][3][3]
// with the weights read in the caller's layout, W[(co * Cin + ci) * 9 + tap]. CV_DW reduces over the rows: they are split
// over blockIdx.z into the fixed ranges of cnn_split, each range writes its own partial product and k_train_reduce adds
// them in range order in double. (The convolutions have no bias: the reduction's bias lanes read the first partial product
// again and write to a scratch row.) The stem is CV_FWD with K = 45 and CV_DW with N = 45.
//
// Determinism: as train_mlp.h. No atomics; every sum over the batch over a partition that depends only on (n, hw, C), the
// parts in index order in double; the scatter has one writer per element.
#pragma once
#include "dev_train_cnn.h"
#include "train_lv.h"
#include "train_sym.h"

namespace ar {

enum { CV_FWD = 0, CV_DIN = 1, CV_DW = 2, CNN_MAX_BLOCKS_TRAIN = 8, CNN_MAX_TRUNK_ROWS = 1 << 22 };

struct TrainConv {
    const float* x;    // the spatial operand whose neighbourhood is read: in [R][Cin] (FWD, DW), dOut [R][Cout] (DIN)
    const float* w;    // FWD, DIN: the weights [Cout][Cin][3][3]
    const float* d;    // DW: dOut [R][Cout]
    const float* add;  // FWD: added to the product as it is stored, [R][Cout] (the skip; may be null)
    float* c;
    int R, hw, bw, bh, Cin, Cout, k_per_split;
    size_t c_split;
};

template <int FORM>
__global__ void __launch_bounds__(TG_THREADS) k_train_conv3(TrainConv g) {
    __shared__ float As[TG_KC][TG_LD], Bs[TG_KC][TG_LD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    // FWD, DIN: the row tiles, up to 65536 of them, go over blockIdx.x
    const int m0 = (FORM == CV_DW ? blockIdx.y : blockIdx.x) * TG_TILE, n0 = (FORM == CV_DW ? blockIdx.x : blockIdx.y) * TG_TILE;
    const int Cx = FORM == CV_DIN ? g.Cout : g.Cin;  // the channels of the spatial operand
    const int M = FORM == CV_DW ? g.Cout : g.R, N = FORM == CV_FWD ? g.Cout : FORM == CV_DIN ? g.Cin : 9 * g.Cin;
    const int K = FORM == CV_DW ? g.R : 9 * Cx;
    const int k_begin = blockIdx.z * g.k_per_split;
    const int k_end = K - k_begin < g.k_per_split ? K : k_begin + g.k_per_split;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    tr_f32x16 c;
#pragma unroll
    for (int v = 0; v < 16; ++v) c[v] = 0.0f;
    constexpr int PER = TG_TILE * TG_KC / TG_THREADS;
    float ra[PER], rb[PER];
    // What a thread's elements keep over the whole k range. FWD, DIN (element e = tid + 256 i is (m, k) = (e >> 4, e & 15) of
    // A and (k, n) = (e & 15, e >> 4) of the weights): the row's first cell, its (y, x) -- y far off the board beyond M, so
    // every tap misses -- and n. DW ((k, m) = (k, n) = (e >> 6, e & 63)): n's channel and tap.
    int base[PER], cy[PER], cx[PER];
    const int sub = FORM == CV_DW ? tid >> 6 : tid & (TG_KC - 1), own = FORM == CV_DW ? tid & (TG_TILE - 1) : tid >> 4;
    int dw_ci = 0, dw_tap = 0;
    if (FORM == CV_DW) {
        dw_ci = (n0 + own) / 9;
        dw_tap = (n0 + own) - 9 * dw_ci;
    } else {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int m = m0 + own + 16 * i, cell = m % g.hw;
            base[i] = m - cell;
            cy[i] = m < M ? cell / g.bw : -4;
            cx[i] = cell % g.bw;
        }
    }
    auto fetch = [&](int k0) {
        if (FORM == CV_DW) {
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int row = k0 + sub + 4 * i, co = m0 + own, j = n0 + own;
                const bool live = row < k_end;
                ra[i] = (live && co < M) ? g.d[(size_t)row * g.Cout + co] : 0.0f;
                int nb = -1;
                if (live && j < N) {
                    const int cell = row % g.hw;
                    nb = cnn_nbr(cell, dw_tap, g.bw, g.bh);
                    if (nb >= 0) nb += row - cell;
                }
                rb[i] = nb >= 0 ? g.x[(size_t)nb * g.Cin + dw_ci] : 0.0f;
            }
        } else {
            const int k = k0 + sub;
            const bool live = k < k_end;
            const int tap = live ? k / Cx : 0, ch = live ? k - tap * Cx : 0;
            const int at = FORM == CV_DIN ? cnn_tap_mirror(tap) : tap;
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int nb = live ? cnn_nbr_yx(cy[i], cx[i], at, g.bw, g.bh) : -1;
                ra[i] = nb >= 0 ? g.x[(size_t)(base[i] + nb) * Cx + ch] : 0.0f;
                const int gn = n0 + own + 16 * i;
                const size_t wi = FORM == CV_FWD ? (size_t)gn * g.Cin + ch : (size_t)ch * g.Cin + gn;
                rb[i] = (live && gn < N) ? g.w[wi * 9 + tap] : 0.0f;
            }
        }
    };
    if (k_begin < k_end) fetch(k_begin);
    for (int k0 = k_begin; k0 < k_end; k0 += TG_KC) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            if (FORM == CV_DW) {
                As[sub + 4 * i][own] = ra[i];
                Bs[sub + 4 * i][own] = rb[i];
            } else {
                As[sub][own + 16 * i] = ra[i];
                Bs[sub][own + 16 * i] = rb[i];
            }
        }
        __syncthreads();
        if (k0 + TG_KC < k_end) fetch(k0 + TG_KC);
#pragma unroll
        for (int kk = 0; kk < TG_KC; kk += 2)
            c = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + h][wm + r], Bs[kk + h][wn + r], c, 0, 0, 0);
        __syncthreads();
    }
    float* cz = g.c + (size_t)blockIdx.z * g.c_split;
    const int col = n0 + wn + r;
    if (col < N) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int row = m0 + wm + (v & 3) + 8 * (v >> 2) + 4 * h;
            if (row < M) {
                const size_t at = (size_t)row * N + col;
                if (FORM == CV_FWD && g.add) cz[at] = c[v] + g.add[at];
                else cz[at] = c[v];
            }
        }
    }
}

// train_col_total's sum, the same additions in the same order, with eight parts' loads in flight at a time: one thread walks
// up to 256 parts here, and one load per trip of the memory would be most of a BatchNorm call's time.
__device__ inline double cnn_col_total(const double* part, int P, int H, int col) {
    double s = 0.0;
    int p = 0;
    for (; p + 8 <= P; p += 8) {
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = part[(size_t)(p + k) * H + col];
#pragma unroll
        for (int k = 0; k < 8; ++k) s += v[k];
    }
    for (; p < P; ++p) s += part[(size_t)p * H + col];
    return s;
}

// The column sums of up to two [P][H] arrays of partial sums, the parts in index order, in double: what train_col_total
// gives every thread of a column kernel, formed once per column. `b` may be null.
__global__ void __launch_bounds__(256) k_cnn_collapse(int P, int H, const double* a, double* a_tot, const double* b, double* b_tot) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= H) return;
    a_tot[col] = cnn_col_total(a, P, H, col);
    if (b) b_tot[col] = cnn_col_total(b, P, H, col);
}

// From the flat rows x [n][7 hw + 6]: the stem's input x5 [n hw][5], the side vectors [2n][3] and the player cells [2n]
// (P1's rows, then P2's). One thread an element of x5; the first 6n threads also a side element, the first 2n a cell.
__global__ void __launch_bounds__(256) k_cnn_split(const float* x, float* x5, float* side, int* cells, int n, int hw) {
    const int D = 7 * hw + 6;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * hw * 5) return;
    {
        const size_t m = i / 5, row = m / (size_t)hw;
        x5[i] = x[row * D + cnn_plane_src(hw, (int)(m - row * hw), (int)(i - m * 5))];
    }
    if (i < (size_t)6 * n) {
        const size_t r = i / 3;
        const int p = r >= (size_t)n;
        side[i] = x[(r - (size_t)p * n) * D + cnn_side_src(hw, p, (int)(i - r * 3))];
    }
    if (i < (size_t)2 * n) {
        const int p = i >= (size_t)n;
        cells[i] = cnn_player_cell(x + (i - (size_t)p * n) * D, hw, p);
    }
}

// cat [2n][C + PD]: row r = [x_B[(r mod n) hw + cell_r] | relu(ze[r])]: the mask-multiply-sum of a one-hot mask, and the cat
__global__ void __launch_bounds__(256)
k_cnn_gather(const float* f, const int* cells, const float* ze, float* cat, int n, int hw, int C, int PD) {
    const int W = C + PD;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)2 * n * W) return;
    const size_t r = i / (size_t)W;
    const int j = (int)(i - r * W);
    if (j < C) {
        const int cell = cells[r];
        cat[i] = cell >= 0 ? f[((r < (size_t)n ? r : r - n) * hw + cell) * C + j] : 0.0f;
    } else {
        const float z = ze[r * PD + (j - C)];
        cat[i] = z > 0.0f ? z : 0.0f;
    }
}

// dZc [2n][H] = dh_i masked by the combiner's ReLU: k_sym_dhead's dy (sym_head_dy over the packed dOut rows) with no
// BatchNorm behind it, so no column sums
__global__ void __launch_bounds__(256)
k_cnn_dhead(const float* d12, const float* w_p, const float* w_v, const float* h, float* dz, int rows, int H) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)rows * H) return;
    const size_t r = i / (size_t)H;
    const int col = (int)(i - r * H);
    float w_lo[6], w_hi[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float* w = k < 5 ? w_p + (size_t)k * 2 * H : w_v;
        w_lo[k] = w[col];
        w_hi[k] = w[H + col];
    }
    const float dy = sym_head_dy(d12 + r * 12, w_lo, w_hi);
    dz[i] = h[i] > 0.0f ? dy : 0.0f;
}

// dZe [2n][PD] = the last PD columns of dcat [2n][C + PD] masked by the encoder's ReLU
__global__ void __launch_bounds__(256) k_cnn_enc_bwd(const float* dcat, const float* ze, float* dze, int rows, int C, int PD) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)rows * PD) return;
    const size_t r = i / (size_t)PD;
    dze[i] = ze[i] > 0.0f ? dcat[r * (C + PD) + C + (i - r * PD)] : 0.0f;
}

// d x_B [n hw][C]: the first C columns of dcat at the players' cells, P1's term before P2's where they share one, zero
// everywhere else. One thread an element: one writer, no atomics.
__global__ void __launch_bounds__(256)
k_cnn_scatter(const float* dcat, const int* cells, float* df, int n, int hw, int C, int PD) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * hw * C) return;
    const size_t m = i / (size_t)C, row = m / (size_t)hw;
    const int col = (int)(i - m * C), cell = (int)(m - row * hw), W = C + PD;
    float v = 0.0f;
    if (cells[row] == cell) v += dcat[row * W + col];
    if (cells[(size_t)n + row] == cell) v += dcat[((size_t)n + row) * W + col];
    df[i] = v;
}

// g = g + e, four elements a thread: the skip's share of a block's input gradient
__global__ void __launch_bounds__(256) k_cnn_add(float4* g, const float4* e, size_t count4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count4) return;
    const float4 a = g[i], b = e[i];
    g[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

}  // namespace ar
