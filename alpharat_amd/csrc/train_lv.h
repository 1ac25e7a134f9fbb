// One training step of LocalValueMLP (alpharat/nn/models/local_value.py, BatchNorm in training mode, dropout when asked
// for) over a window of the row set's order: PyRatMLP's step (train_mlp.h) with the ownership head, its masked
// cross-entropy (alpharat/nn/losses/ownership.py) as the third term of the loss
// (alpharat/nn/architectures/local_value/loss.py) and what loss.backward() leaves in the eighteen .grad tensors, f32
// throughout. The trunk, the three heads, the products, the column kernels and the ordered reductions are train_mlp.h's;
// the per-cell arithmetic is dev_train_lv.h; this file holds what the head adds.
//
// The chain of one step, every launch on the caller's stream: rows_grad_mlp in alpharat_hip.hip with its `lv` argument set
// is this listing as calls. The lines without a number are train_mlp.h's own, issued by the same code:
//        k_rows_batch ... k_train_bn_apply            X, the targets (the window's swapped cheese outcomes among them), A2    9
//        k_train_heads                                the three heads of a row, their loss terms and dOut                     1
//   11   k_train_gemm                                 Zo = A2 Wo0^T + bo0                                    [n][H]
//   12   k_train_lv_relu                              Ao = relu(Zo)
//   13   k_train_gemm                                 L = Ao Wo2^T + bo2                                     [n][4 hw], class fastest
//   14   k_train_own_count                            the active cells of each row part, from the int8 outcomes
//        (a device-to-device copy of L, when the caller asks for the logits)
//   15   k_train_own_cells                            dL in place of L; the ce of the active cells per row part
//   16   k_train_lv_loss_sum                          the seven losses
//        k_train_gemm (split), k_train_reduce         dOut^T A2: the six head gradients                                       2
//   19   k_train_gemm (split), k_train_reduce         dL^T Ao: ownership_head.2's two gradients (M = 4 hw)
//   21   k_train_gemm                                 dAo = dL Wo2 (K = 4 hw)
//   22   k_train_lv_relu_bwd                          dZo = dAo where Zo > 0, in place
//   23   k_train_gemm (split), k_train_reduce         dZo^T A2: ownership_head.0's two gradients
//   25   k_train_gemm                                 dZo Wo0, into the array the trunk's backward starts from
//   26   k_train_colsum<DHEAD_ADD>                    dY2 = (dOut Wh + dZo Wo0) masked by trunk.5's ReLU, its column sums
//        k_train_bn_bwd ... k_train_reduce            the rest of train_mlp.h's backward                                      9
// With dropout (ar_rows_grad_local_value_dropout) A2 is the trunk output behind the second dropout, which the ownership head
// reads as the other heads do, so the DROP form of k_train_colsum<DHEAD_ADD> scales the sum of both consumers' gradients.
// 35 launches, 12 more than the MLP's step: k_train_lv_loss_sum stands where k_train_loss_sum stood and
// k_train_colsum<DHEAD_ADD> where k_train_colsum<DHEAD> did.
//
// No active cell in the window (stored positions always hold a cheese, so only a harness gets there): the scale of
// lv_own_scale is 0, every dL is 0, and with it the head's four gradients and its share of dA2; loss_ownership is 0.
//
// Determinism: as train_mlp.h. No atomics. The cells are counted in integers; their ce is added in double over the fixed
// partition of lv_cells (dev_train_lv.h): thread t of a row part takes its cells t, t + 256, ... in row-then-cell order, the
// 256 sums are added in thread order, the parts in index order.
#pragma once
#include "dev_train_lv.h"
#include "train_mlp.h"

namespace ar {

// out = max(z, 0), four elements a thread
__global__ void __launch_bounds__(256) k_train_lv_relu(const float4* z, float4* act, size_t count4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count4) return;
    const float4 v = z[i];
    act[i] = make_float4(v.x > 0.0f ? v.x : 0.0f, v.y > 0.0f ? v.y : 0.0f, v.z > 0.0f ? v.z : 0.0f, v.w > 0.0f ? v.w : 0.0f);
}

// d = d where z > 0, else 0, in place
__global__ void __launch_bounds__(256) k_train_lv_relu_bwd(const float4* z, float4* d, size_t count4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count4) return;
    const float4 v = z[i], g = d[i];
    d[i] = make_float4(v.x > 0.0f ? g.x : 0.0f, v.y > 0.0f ? g.y : 0.0f, v.z > 0.0f ? g.z : 0.0f, v.w > 0.0f ? g.w : 0.0f);
}

// the sum of a block's 256 counts, in every thread (w: four words of LDS)
__device__ inline uint32_t lv_block_count(uint32_t c, uint32_t* w) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = c;
    __syncthreads();
    return ((w[0] + w[1]) + w[2]) + w[3];
}

// part[b]: the active cells (outcome >= 0) of row part b, counted from the int8 outcomes [n][hw]. Grid t.B, 256 threads.
__global__ void __launch_bounds__(256) k_train_own_count(LvCells t, const int8_t* co, uint32_t* part) {
    __shared__ uint32_t w[4];
    const int r0 = blockIdx.x * t.rpb, r1 = t.n - r0 < t.rpb ? t.n : r0 + t.rpb;
    const size_t i1 = (size_t)r1 * t.hw;
    uint32_t c = 0;
    for (size_t i = (size_t)r0 * t.hw + threadIdx.x; i < i1; i += 256) c += co[i] >= 0 ? 1u : 0u;
    c = lv_block_count(c, w);
    if (threadIdx.x == 0) part[blockIdx.x] = c;
}

// Every cell of row part blockIdx.x: one float4 load of its logits, lv_cell_terms, one float4 store of its dL in their
// place (cell i of the window is float4 i of l: rows are 4 hw floats). The scale is ownership_weight over the window's
// count, which every block adds up from the parts. ce_part[b]: the ce of the part's active cells, in double.
struct LvOwn {
    float* l;                    // [n][hw][4]: L in, dL out
    const int8_t* co;            // [n][hw]
    const uint32_t* count_part;  // [B]
    double* ce_part;             // [B]
    float ow;
};

__global__ void __launch_bounds__(256) k_train_own_cells(LvCells t, LvOwn a) {
    __shared__ uint32_t w[4];
    __shared__ double sums[256];
    const int tid = threadIdx.x;
    uint32_t c = 0;
    for (int b = tid; b < t.B; b += 256) c += a.count_part[b];
    const float scale = lv_own_scale(a.ow, lv_block_count(c, w));
    const int r0 = blockIdx.x * t.rpb, r1 = t.n - r0 < t.rpb ? t.n : r0 + t.rpb;
    const size_t i1 = (size_t)r1 * t.hw;
    float4* l4 = (float4*)a.l;
    double s = 0.0;
    for (size_t i = (size_t)r0 * t.hw + tid; i < i1; i += 256) {
        const int target = a.co[i];
        const float4 v = l4[i];
        float ce, dl[4];
        lv_cell_terms(v.x, v.y, v.z, v.w, target, scale, ce, dl);
        s += (double)ce;  // (0 for a cell that is not active)
        l4[i] = make_float4(dl[0], dl[1], dl[2], dl[3]);
    }
    sums[tid] = s;
    __syncthreads();
    if (tid == 0) {
        double b = 0.0;
        for (int k = 0; k < 256; ++k) b += sums[k];
        a.ce_part[blockIdx.x] = b;
    }
}

// k_train_loss_sum with the third term: wavefronts 0..3 own the four terms of the heads as there (the same lanes, the same
// tree), wavefront 4 the ownership head's: lane l adds row parts l, l + 64, ... in order, a fixed tree combines the lanes.
// losses: loss_p1, loss_p2, loss_value_p1, loss_value_p2, loss_value, loss, loss_ownership; loss includes ow * loss_ownership.
__global__ void __launch_bounds__(320)
k_train_lv_loss_sum(const double* part, uint32_t n_part, uint32_t n, const double* ce_part, const uint32_t* count_part,
                    uint32_t n_own, float pw, float vw, float ow, float* losses, float* losses_out) {
    __shared__ double tot[5];
    const uint32_t j = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    double s = 0.0;
    uint32_t c = 0;
    if (j < 4)
        for (uint32_t b = lane; b < n_part; b += 64) s += part[(size_t)b * 4 + j];
    else
        for (uint32_t b = lane; b < n_own; b += 64) {
            s += ce_part[b];
            c += count_part[b];
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_down(s, off, 64);
        c += __shfl_down(c, off, 64);
    }
    if (lane == 0) tot[j] = j < 4 ? s / (double)n : lv_own_loss(s, c);
    __syncthreads();
    if (threadIdx.x == 0) {
        const double value = 0.5 * (tot[2] + tot[3]);
        const double all[7] = {tot[0], tot[1], tot[2], tot[3], value,
                               (double)pw * (tot[0] + tot[1]) + (double)vw * value + (double)ow * tot[4], tot[4]};
        for (int k = 0; k < 7; ++k) {
            losses[k] = (float)all[k];
            if (losses_out) losses_out[k] = (float)all[k];
        }
    }
}

}  // namespace ar
