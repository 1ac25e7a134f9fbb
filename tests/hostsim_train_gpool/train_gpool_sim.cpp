// TEST HARNESS -- runs alpharat_amd/csrc/dev_train_gpool.h on the CPU: the mean, the maximum and the tie count of one
// (row, channel) over its cells (one thread of k_gpool_reduce) and the gradient of every cell (one thread each of
// k_gpool_dpz), with loops where the device has lanes. It is NOT a CPU fallback: nothing in alpharat_amd/ loads this file.
#include <cstdint>

#include "../../alpharat_amd/csrc/dev_train_gpool.h"

using namespace ar;

extern "C" {

// z[0], z[stride], ..., hw of them; mean_max [2]; count [1]
void tgs_reduce(const float* z, int hw, uint64_t stride, float* mean_max, int32_t* count) {
    const GPoolRow r = gpool_reduce(z, hw, (size_t)stride);
    mean_max[0] = r.mean;
    mean_max[1] = r.max;
    count[0] = r.count;
}

// out [hw]: gpool_dpz of every cell, from gpool_reduce's maximum and count
void tgs_dpz(const float* z, int hw, uint64_t stride, float dmean, float dmax, float* out) {
    const GPoolRow r = gpool_reduce(z, hw, (size_t)stride);
    for (int c = 0; c < hw; ++c) out[c] = gpool_dpz(z[(size_t)c * stride], r.max, r.count, dmean, dmax, hw);
}
}
