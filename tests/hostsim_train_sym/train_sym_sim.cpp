// TEST HARNESS -- runs alpharat_amd/csrc/dev_train_sym.h on the CPU: the columns of the flat row that make SymmetricMLP's three
// inputs (sym_shared_src, sym_player_src, one lane per element in k_sym_split), the packed dOut rows of the heads
// (sym_head_pack, one lane per row in k_sym_heads) and an element of dh_i (sym_head_dy, one lane per element in k_sym_dhead),
// with loops where the device has lanes. It is NOT a CPU fallback: nothing in alpharat_amd/ loads this file.
#include <cstdint>

#include "../../alpharat_amd/csrc/dev_train_sym.h"

using namespace ar;

extern "C" {

// x [n][7hw + 6]; xs [n][5hw + 1]; xp [2n][hw + 2], P1's rows first
void tss_split(uint64_t n, int hw, const float* x, float* xs, float* xp) {
    const int D = 7 * hw + 6, Ds = sym_shared_dim(hw), Dp = sym_player_dim(hw);
    for (uint64_t r = 0; r < n; ++r) {
        for (int j = 0; j < Ds; ++j) xs[r * Ds + j] = x[r * D + sym_shared_src(hw, j)];
        for (int p = 0; p < 2; ++p)
            for (int j = 0; j < Dp; ++j) xp[(p * n + r) * Dp + j] = x[r * D + sym_player_src(hw, p, j)];
    }
}

// dout [n][12] as train_head_terms gives it; d12 [2n][12], P1's rows first
void tss_pack(uint64_t n, const float* dout, float* d12) {
    for (uint64_t r = 0; r < n; ++r) sym_head_pack(dout + r * 12, d12 + r * 12, d12 + (n + r) * 12);
}

// d12 [rows][12]; wh [6][2H]; dy [rows][H]
void tss_head_dy(uint64_t rows, uint32_t H, const float* d12, const float* wh, float* dy) {
    for (uint32_t c = 0; c < H; ++c) {
        float lo[6], hi[6];
        for (int k = 0; k < 6; ++k) {
            lo[k] = wh[(uint64_t)k * 2 * H + c];
            hi[k] = wh[(uint64_t)k * 2 * H + H + c];
        }
        for (uint64_t r = 0; r < rows; ++r) dy[r * H + c] = sym_head_dy(d12 + r * 12, lo, hi);
    }
}

}  // extern "C"
