// The per-element arithmetic that a GPoolResBlock (alpharat/nn/models/cnn/blocks.py) adds to one training step of PyRatCNN
// (train_gpool.h): what the reference does in
//   pool.mean(dim=(2, 3)), pool.amax(dim=(2, 3))   over the hw cells of one (row, channel)        -> gpool_reduce
//   their backward: the mean's gradient spread evenly over the cells, the maximum's shared evenly among the cells that
//   equal it (amax's rule; a first-index rule would be another function)                          -> gpool_dpz
// Plain C++ with no barrier, no reduction across threads and no HIP call, for host and device as dev_train_cnn.h:
// tests/hostsim_train_gpool compiles this text.
#pragma once
#include "dev_train_cnn.h"

namespace ar {

// mean, maximum and the number of cells that equal the maximum
struct GPoolRow {
    float mean, max;
    int count;
};

// over z[0], z[stride], ..., z[(hw - 1) stride]: the cells in increasing order, the sum in double and rounded once
AR_HD GPoolRow gpool_reduce(const float* z, int hw, size_t stride) {
    double s = 0.0;
    float mx = z[0];
    int count = 0;
    for (int c = 0; c < hw; ++c) {
        const float v = z[(size_t)c * stride];
        s += (double)v;
        if (v > mx) {
            mx = v;
            count = 1;
        } else if (v == mx) {
            ++count;
        }
    }
    GPoolRow r;
    r.mean = (float)(s / (double)hw);
    r.max = mx;
    r.count = count;
    return r;
}

// d pz of one cell: its share of the mean's gradient, and of the maximum's where the cell holds the maximum
AR_HD float gpool_dpz(float z, float max, int count, float dmean, float dmax, int hw) {
    const float a = dmean / (float)hw;
    return z == max ? a + dmax / (float)count : a;
}

}  // namespace ar
