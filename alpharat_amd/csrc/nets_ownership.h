// The ownership head of LocalValueMLP (alpharat/nn/models/local_value.py:103-107, 182-193) and the terms of its loss
// (dev_ownership.h) for a tile of stored positions, on the matrix cores:
//   logits[hw][4] = Linear(H -> 4 hw)(relu(Linear(H -> H)(features))),
// where `features` is the trunk's output that k_mlp_mfma<.., FEAT = true> (nets.h) stored. Validation only: no evaluator
// of the self-play loop runs this head (model.predict() takes its values from value_head).
//
// One block of four wavefronts takes 64 rows. The feature tile sits in LDS as [64][H + 4], k_mlp_mfma's layout. The hidden
// layer is one mfma_pass per wavefront (64 of the H columns each), held in the accumulators until every wavefront has read
// the tile and then written over it with ReLU. The output layer walks the padded [H][Npad] weights in passes of 256 columns
// (64 cells), a wavefront taking 64 columns of the pass. In the accumulator layout a lane holds column `lane & 31` of its
// tile, so the four classes of a cell sit in four adjacent lanes: each lane takes the exponential of its own logit, and
// the quad's logits and exponentials reach every lane of the quad by DPP quad broadcasts (no LDS traffic). The quad's
// first lane writes the cell's terms (own_cell_finish) to LDS; after the pass one thread per row adds the pass's active
// cells in cell order to its running doubles (own_row_add). No atomics anywhere: the same request gives the same bytes.
//
// LDS: the tile (66.5 KB at H = 256) + the pass's terms (64 rows x 65 x 2 floats = 32.5 KB) + targets and states (7 KB):
// 106 KB at H = 256, 57 KB at H = 64. A CU holds one block (one wavefront per SIMD) at every width: at H = 256 by its LDS,
// below that by the kernel's 289 registers a lane (profiles/ownership_resource_usage.txt). Not tuned and not timed.
#pragma once
// (included from nets.h after the shared helpers)
#include "dev_ownership.h"

namespace arnet {

// ownership_head.0 and ownership_head.2, transposed to [in][out]; the output layer's columns padded with zeros to a
// multiple of 64 so that a column pass needs no guard
struct OwnDev {
    int H, hw, Npad;
    const float *w1t, *b1;  // [H][H], [H]
    const float *w2t, *b2;  // [H][Npad], [Npad]
};

enum { OWN_ROWS = 64, OWN_PASS_COLS = 256, OWN_PASS_CELLS = 64, OWN_TERM_LD = 65, OWN_TGT_LD = 68 };

inline size_t own_smem_bytes(int H) { return (size_t)OWN_ROWS * (H + 4) * 4; }

// lane K of every quad, to the four lanes of the quad (DPP quad_perm:[K,K,K,K])
template <int K>
__device__ inline float quad_bcast(float x) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), K * 0x55, 0xF, 0xF, true));
}

// `feat` [n][H]: the trunk's output of request i; `req` [n]: its position and, as `slot`, its stored game; `outcomes`
// [games][hw]. Per-row outputs row_ce / row_cells / row_value [n]; `logits` [n][hw][4] or null.
template <int NW>
__global__ void __launch_bounds__(NTHREADS) k_own_mfma(OwnDev own, const float* __restrict__ feat, const ar::LeafReq<NW>* req,
                                                       const uint8_t* __restrict__ outcomes, uint32_t n, double* row_ce,
                                                       uint32_t* row_cells, float* row_value, float* logits) {
    constexpr int MT = 2, L = OWN_ROWS;
    extern __shared__ float smem[];
    const int H = own.H, hw = own.hw, ld = H + 4, Npad = own.Npad;
    float* act = smem;  // [L][ld]: the features, then the hidden layer
    __shared__ float t_ce[L][OWN_TERM_LD], t_ev[L][OWN_TERM_LD];  // a pass's terms: [row][cell of the pass]
    __shared__ signed char tgt[L][OWN_TGT_LD];                    // a pass's targets, -1 = not active
    __shared__ ar::State<NW> st[L];
    __shared__ uint32_t game[L];
    const uint32_t base = blockIdx.x * L;
    if (base >= n) return;
    const int cnt = (int)((n - base) < (uint32_t)L ? (n - base) : (uint32_t)L);
    const int tid = threadIdx.x;
    if (tid < L) {  // (rows past the request repeat its first row; nothing of theirs is written)
        const ar::LeafReq<NW>& q = req[base + (tid < cnt ? tid : 0)];
        st[tid] = q.st;
        game[tid] = q.slot;
    }
    const int H4 = H >> 2;
    for (int item = tid; item < L * H4; item += NTHREADS) {
        const int l = item / H4, c4 = item - l * H4;
        *(float4*)(act + (size_t)l * ld + 4 * c4) = ((const float4*)(feat + (size_t)(base + (l < cnt ? l : 0)) * H))[c4];
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const float* ap = act + (size_t)r * ld + h;
    auto a_of = [&](int k, int t) -> float { return ap[(size_t)(32 * t) * ld + k]; };
    f32x16 c[MT][2];
    {
        // hidden layer, result held in the accumulators until every wavefront is done reading `act`
        const int n0 = wave * 64;
        const bool has = n0 < H, two = n0 + 32 < H;  // wave-uniform; H <= 64 * waves
        if (has) {
            const float b0 = own.b1[n0 + r], b1 = own.b1[n0 + (two ? 32 : 0) + r];
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    c[t][0][v] = b0;
                    c[t][1][v] = b1;
                }
            mfma_pass<MT, 8>(own.w1t + (size_t)h * H + n0 + r, two, H, H, h, a_of, c);
        }
        __syncthreads();
        if (has) {
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int i = acc_row(t, v, h);
                    act[(size_t)i * ld + n0 + r] = fmaxf(c[t][0][v], 0.0f);
                    if (two) act[(size_t)i * ld + n0 + 32 + r] = fmaxf(c[t][1][v], 0.0f);
                }
        }
        __syncthreads();
    }
    ar::OwnRow acc;  // of row `tid`, in the first L threads
    ar::own_row_clear(acc);
    const size_t row_floats = (size_t)hw * 4;
    for (int p0 = 0; p0 < Npad; p0 += OWN_PASS_COLS) {
        {
            // the targets of the pass's cells: four threads per row, sixteen cells each
            const int l = tid >> 2;
            const uint8_t* oc = outcomes + (size_t)game[l] * hw;
            for (int j = 0; j < 16; ++j) {
                const int cl = (tid & 3) * 16 + j, cell = (p0 >> 2) + cl;
                tgt[l][cl] = (signed char)(cell < hw ? ar::own_cell_target<NW>(st[l], oc, cell) : -1);
            }
        }
        const int q0 = p0 + wave * 64;  // this wavefront's 64 columns: 16 cells
        const bool has = q0 < Npad;     // wave-uniform; Npad is a multiple of 64, so both column tiles are whole
        if (has) {
            const float b0 = own.b2[q0 + r], b1 = own.b2[q0 + 32 + r];
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    c[t][0][v] = b0;
                    c[t][1][v] = b1;
                }
            mfma_pass<MT, 8>(own.w2t + (size_t)h * Npad + q0 + r, true, H, Npad, h, a_of, c);
        }
        __syncthreads();  // the pass's targets are in LDS
        if (has) {
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const int i = acc_row(t, v, h);
                        const int col = q0 + 32 * s + r;
                        const float x = c[t][s][v];
                        if (logits && i < cnt && col < 4 * hw) logits[(size_t)(base + i) * row_floats + col] = x;
                        const float l0 = quad_bcast<0>(x), l1 = quad_bcast<1>(x), l2 = quad_bcast<2>(x), l3 = quad_bcast<3>(x);
                        const float m = ar::own_cell_max(l0, l1, l2, l3);
                        const float e = expf(x - m);
                        const int cl = (wave * 64 + 32 * s + r) >> 2;
                        float ce, ev;
                        ar::own_cell_finish(l0, l1, l2, l3, quad_bcast<0>(e), quad_bcast<1>(e), quad_bcast<2>(e), quad_bcast<3>(e),
                                            m, (int)tgt[i][cl], ce, ev);
                        if ((r & 3) == 0) {
                            t_ce[i][cl] = ce;
                            t_ev[i][cl] = ev;
                        }
                    }
        }
        __syncthreads();
        if (tid < L) {
            const int left = hw - (p0 >> 2), n_cells = left < OWN_PASS_CELLS ? left : (int)OWN_PASS_CELLS;
            for (int cl = 0; cl < n_cells; ++cl)
                if (tgt[tid][cl] >= 0) ar::own_row_add(acc, t_ce[tid][cl], t_ev[tid][cl]);
        }
        __syncthreads();  // the pass's terms and targets are read before the next pass writes them
    }
    if (tid < cnt) {
        row_ce[base + tid] = acc.ce;
        row_cells[base + tid] = acc.cells;
        row_value[base + tid] = (float)acc.value;
    }
}

}  // namespace arnet
