// What ar_rows_grad_cnn_gpool adds to train_cnn.h's step: the pool path of a GPoolResBlock (alpharat/nn/models/cnn/blocks.py)
// and the dropout behind the ReLU of player_encoder and of combiner. The per-element arithmetic is dev_train_gpool.h and
// dev_dropout.h; the BatchNorm, the products and the ordered reductions are the kernels train_cnn.h already launches. No
// kernel of the existing chain is touched: the masked forms below are kernels of their own.
//
// A gpool block b with G = gpool_channels, in train_cnn.h's layout ([R][C], R = n hw, row m = row * hw + cell). Forward,
// behind the block's bn, conv, bn and a conv that stores conv2(a') without the skip:
//    bn                           ap = relu(pool_bn(x_b)), a BatchNorm call of its own (index 2 B + 1 + b)           5
//    k_train_gemm                 pz [R][G] = ap pool_conv.weight^T (a 1x1 convolution is a plain product)
//    k_gpool_reduce               pool_cat [n][2G] = [mean | max] over a row's hw cells, and the tie count [n][G]
//    k_train_gemm                 po [n][C] = pool_cat pool_linear.weight^T + pool_linear.bias
//    k_gpool_join                 x_b+1 = (conv2(a') + po[row]) + x_b, torch's order of regular + pool_out + identity
// 9 launches more than a ResBlock's 12. Backward, behind the regular path's 12 launches (which leave their input gradient
// in E), with g = d x_b+1:
//    k_gpool_rowsum               dpo [n][C] = the sum of g over a row's cells
//    k_train_gemm (split), k_train_reduce   pool_linear's two gradients, dpo^T pool_cat and colsum(dpo), over train_split(n)
//    k_train_gemm                 dcat [n][2G] = dpo pool_linear.weight
//    k_gpool_dpz                  dpz [R][G]: dcat's mean half / hw, and the max half / count where pz equals the maximum
//    k_train_gemm (split), k_train_reduce   pool_conv.weight.grad [G][C] = dpz^T ap over cnn_split's ranges, as CV_DW
//    k_train_gemm                 dap [R][C] = dpz pool_conv.weight
//    bn'                          pool_bn, masked by ap > 0                                                          3
//    k_cnn_add, k_cnn_add         g = (g + E) + that: the skip's, the regular path's and the pool path's share
// 12 launches more than a ResBlock's 13: a step of B blocks, P of them gpool, is 29 + 25 B + 21 P launches, 125 for the
// shipped res, res, gpool trunk.
//
// Dropout (ArTrainDropout, p > 0): cat = [f | drop(relu(enc))] and h = drop(relu(comb(cat))), the modules called once per
// player on that player's n rows -- call 0, 1: player_encoder on P1's, P2's rows; call 2, 3: combiner on P1's, P2's rows;
// element e = row * H + column with row counted within the call's n rows and H = PD resp. HD. k_cnn_gather_drop,
// k_cnn_relu_drop, k_cnn_dhead_drop and k_cnn_enc_bwd_drop stand where k_cnn_gather, k_train_lv_relu, k_cnn_dhead and
// k_cnn_enc_bwd did: the same launch count. No mask is stored; the backward reads it off the activation (act > 0).
//
// Workspace per gpool block: ap [R][C], pz [R][G], pool_cat [n][2G] and the counts [n][G]. With any gpool block, once per
// step: a sixth transient array [R][C] (conv2 without the skip in the forward, the pool path's gradient in the backward),
// one array [n][C] that holds po in the forward and dpo in the backward, dcat [n][2 Gmax] and dpz [R][Gmax], Gmax the widest
// gpool block's G; and B more rows of means and rstd.
//
// Determinism as train_cnn.h: no atomics; k_gpool_reduce and k_gpool_rowsum have one thread per output, which walks the
// cells in increasing order and sums in double; the weight gradients are reduced over partitions that depend only on
// (n, hw, C, G) and added in index order in double.
#pragma once
#include "dev_train_gpool.h"
#include "train_cnn.h"

namespace ar {

enum { CNN_MAX_GPOOL = 256 };

// pool_cat [n][2G] and the tie counts [n][G] from pz [n hw][G]: one thread a (row, channel), neighbours neighbouring channels
__global__ void __launch_bounds__(256) k_gpool_reduce(const float* pz, float* cat, int* count, int n, int hw, int G) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * G) return;
    const size_t row = i / (size_t)G;
    const int g = (int)(i - row * G);
    const GPoolRow r = gpool_reduce(pz + row * hw * G + g, hw, (size_t)G);
    cat[row * 2 * G + g] = r.mean;
    cat[row * 2 * G + G + g] = r.max;
    count[i] = r.count;
}

// x_b+1 [R][C] = (c2 + po[row]) + x_b, four channels a thread (C is a multiple of 32)
__global__ void __launch_bounds__(256)
k_gpool_join(const float4* c2, const float* po, const float4* x, float4* out, size_t count4, int hw, int C) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count4) return;
    const size_t e = i * 4, m = e / (size_t)C, row = m / (size_t)hw;
    const float4 a = c2[i], s = x[i], p = *(const float4*)(po + row * C + (e - m * C));
    out[i] = make_float4((a.x + p.x) + s.x, (a.y + p.y) + s.y, (a.z + p.z) + s.z, (a.w + p.w) + s.w);
}

// dpo [n][C]: g [n hw][C] summed over a row's cells, in cell order in double; one thread an element
__global__ void __launch_bounds__(256) k_gpool_rowsum(const float* g, float* dpo, int n, int hw, int C) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * C) return;
    const size_t row = i / (size_t)C;
    const float* at = g + row * hw * C + (i - row * C);
    double s = 0.0;
    for (int c = 0; c < hw; ++c) s += (double)at[(size_t)c * C];
    dpo[i] = (float)s;
}

// dpz [n hw][G] from dcat [n][2G], the stored maxima (pool_cat's second half) and their tie counts
__global__ void __launch_bounds__(256)
k_gpool_dpz(const float* pz, const float* cat, const int* count, const float* dcat, float* dpz, int n, int hw, int G) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * hw * G) return;
    const size_t m = i / (size_t)G, row = m / (size_t)hw;
    const int g = (int)(i - m * G);
    const size_t at = row * 2 * G + g;
    dpz[i] = gpool_dpz(pz[i], cat[at + G], count[row * G + g], dcat[at], dcat[at + G], hw);
}

// ---- the masked forms of the four kernels around the player cells ---------------------------------------------------------------
// k_cnn_gather with the dropout behind the encoder's ReLU: d[p] is the mask of player p's call
__global__ void __launch_bounds__(256)
k_cnn_gather_drop(const float* f, const int* cells, const float* ze, float* cat, int n, int hw, int C, int PD, TrainDrop d0, TrainDrop d1) {
    const int W = C + PD;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)2 * n * W) return;
    const size_t r = i / (size_t)W;
    const int j = (int)(i - r * W);
    if (j < C) {
        const int cell = cells[r];
        cat[i] = cell >= 0 ? f[((r < (size_t)n ? r : r - n) * hw + cell) * C + j] : 0.0f;
    } else {
        const bool p2 = r >= (size_t)n;
        const TrainDrop& d = p2 ? d1 : d0;
        const float z = ze[r * PD + (j - C)];
        const uint64_t e = (uint64_t)(p2 ? r - n : r) * PD + (j - C);
        cat[i] = (z > 0.0f && dropout_keep(d.key, d.thr, e)) ? z * d.scale : 0.0f;
    }
}

// h [2n][H] = drop(relu(z)): k_train_lv_relu with the combiner's dropout, an element a thread
__global__ void __launch_bounds__(256) k_cnn_relu_drop(const float* z, float* act, int n, int H, TrainDrop d0, TrainDrop d1) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, half = (size_t)n * H;
    if (i >= 2 * half) return;
    const bool p2 = i >= half;
    const TrainDrop& d = p2 ? d1 : d0;
    const float v = z[i];
    act[i] = (v > 0.0f && dropout_keep(d.key, d.thr, (uint64_t)(p2 ? i - half : i))) ? v * d.scale : 0.0f;
}

// k_cnn_dhead behind the combiner's dropout: dy * scale before the mask, which h > 0 now holds whole
__global__ void __launch_bounds__(256)
k_cnn_dhead_drop(const float* d12, const float* w_p, const float* w_v, const float* h, float* dz, int rows, int H, float scale) {
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
    const float dy = sym_head_dy(d12 + r * 12, w_lo, w_hi) * scale;
    dz[i] = h[i] > 0.0f ? dy : 0.0f;
}

// k_cnn_enc_bwd behind the encoder's dropout: the mask is read off cat's last PD columns, where drop(relu(ze)) stands
__global__ void __launch_bounds__(256)
k_cnn_enc_bwd_drop(const float* dcat, const float* cat, float* dze, int rows, int C, int PD, float scale) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)rows * PD) return;
    const size_t r = i / (size_t)PD, at = r * (C + PD) + C + (i - r * PD);
    dze[i] = cat[at] > 0.0f ? dcat[at] * scale : 0.0f;
}

}  // namespace ar
