// TEST HARNESS -- runs alpharat_amd/csrc/dev_ownership.h on the CPU: the terms of one cell (own_cell_terms) and of one row
// (own_row_terms: the active cells of a stored position against its game's outcomes, added in cell order in double), with a
// loop over the rows where the device has a block per 64 rows. Boards of up to 64 cells run the NW = 1 instantiation, larger
// ones NW = 4, as the library chooses. It is NOT a CPU fallback: nothing in alpharat_amd/ loads this file.
#include <cstdint>
#include <cstring>

#include "../../alpharat_amd/csrc/dev_ownership.h"

using namespace ar;

namespace {

// Row r: its cheese mask mask[r][hw] (bytes), its game's outcomes out[r][hw], the head's logits [r][hw][4]
template <int NW>
void run(uint64_t n, int hw, const uint8_t* mask, const uint8_t* outcomes, const float* logits, double* ce, uint32_t* cells,
         float* value) {
    for (uint64_t r = 0; r < n; ++r) {
        PosRec<NW> rec;
        std::memset(&rec, 0, sizeof rec);
        for (int c = 0; c < hw; ++c)
            if (mask[r * hw + c]) rec.st.cheese[c >> 6] |= 1ULL << (c & 63);
        const OwnRow t = own_row_terms<NW>(rec, outcomes + r * hw, logits + r * (uint64_t)hw * 4, hw);
        ce[r] = t.ce;
        cells[r] = t.cells;
        value[r] = (float)t.value;
    }
}

}  // namespace

extern "C" {

void os_rows(int nw, uint64_t n, int hw, const uint8_t* mask, const uint8_t* outcomes, const float* logits, double* ce,
             uint32_t* cells, float* value) {
    if (nw == 1) run<1>(n, hw, mask, outcomes, logits, ce, cells, value);
    else run<4>(n, hw, mask, outcomes, logits, ce, cells, value);
}

// n cells: logits [n][4], targets [n] -> ce [n], ev [n]
void os_cells(uint64_t n, const float* logits, const int32_t* targets, float* ce, float* ev) {
    for (uint64_t i = 0; i < n; ++i) own_cell_terms(logits + 4 * i, targets[i], ce[i], ev[i]);
}

}  // extern "C"
