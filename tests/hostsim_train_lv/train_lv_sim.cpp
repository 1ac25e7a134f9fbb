// TEST HARNESS -- runs alpharat_amd/csrc/dev_train_lv.h on the CPU: one cell's ce and dL from its four logits, its target and
// the scale (lv_cell_terms, one lane per cell in k_train_own_cells), the scale and the loss with their rule for a window
// without an active cell (lv_own_scale, lv_own_loss) and the fixed partition of the rows (lv_cells), with loops where the
// device has lanes. It is NOT a CPU fallback: nothing in alpharat_amd/ loads this file.
#include <cstdint>

#include "../../alpharat_amd/csrc/dev_train_lv.h"

using namespace ar;

extern "C" {

struct TlsCell {
    float ce, dl[4];
};

int tls_cell_words() { return (int)(sizeof(TlsCell) / 4); }

// logits [cells][4]; targets [cells] (negative: not active)
void tls_cells(uint64_t cells, const float* logits, const int8_t* targets, float scale, TlsCell* out) {
    for (uint64_t i = 0; i < cells; ++i) {
        const float* l = logits + 4 * i;
        lv_cell_terms(l[0], l[1], l[2], l[3], (int)targets[i], scale, out[i].ce, out[i].dl);
    }
}

float tls_scale(float ow, uint32_t cells) { return lv_own_scale(ow, cells); }

double tls_loss(double ce_sum, uint32_t cells) { return lv_own_loss(ce_sum, cells); }

void tls_parts(int n, int hw, int* out) {
    const LvCells t = lv_cells(n, hw);
    out[0] = t.B;
    out[1] = t.rpb;
}

}  // extern "C"
