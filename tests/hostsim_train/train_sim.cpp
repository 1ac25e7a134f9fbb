// TEST HARNESS -- runs alpharat_amd/csrc/dev_train.h on the CPU: the heads' terms of a row (train_head_terms, one lane per
// row in k_train_heads) and the BatchNorm forward and backward of an element (train_bn_forward, train_bn_backward, one lane
// per element in k_train_bn_apply, k_train_colsum and k_train_bn_bwd), with loops where the device has lanes. The column
// statistics are arguments, as they are for the kernels. Also the two partitions of a step (train_cols, train_split), which
// the host drivers call as they stand. It is NOT a CPU fallback: nothing in alpharat_amd/ loads this file.
#include <cstdint>
#include <cstring>

#include "../../alpharat_amd/csrc/dev_train.h"

using namespace ar;

extern "C" {

// out [n][12]: l1, l2, o of every row; terms [n]: TrainHeadTerms (18 floats each)
void ts_heads(uint64_t n, const float* out, const float* t1, const float* t2, const float* y1, const float* y2, float pw_n,
              float vw_n, void* terms) {
    TrainHeadTerms* t = (TrainHeadTerms*)terms;
    for (uint64_t r = 0; r < n; ++r) t[r] = train_head_terms(out + r * 12, t1 + r * 5, t2 + r * 5, y1[r], y2[r], pw_n, vw_n);
}

int ts_terms_words(void) { return (int)(sizeof(TrainHeadTerms) / 4); }

// z, y, xhat [n][H]; mu (double), var, gamma, beta [H]
void ts_bn_forward(uint64_t n, uint32_t H, const float* z, const double* mu, const float* var, const float* gamma,
                   const float* beta, float* y, float* xhat) {
    for (uint64_t r = 0; r < n; ++r)
        for (uint32_t c = 0; c < H; ++c) {
            const uint64_t i = r * H + c;
            y[i] = train_bn_forward(z[i], mu[c], train_bn_rstd(var[c]), gamma[c], beta[c], xhat[i]);
        }
}

// dy, xhat, dz [n][H]; var, gamma, mean_dy, mean_dy_xhat [H]
void ts_bn_backward(uint64_t n, uint32_t H, const float* dy, const float* xhat, const float* var, const float* gamma,
                    const float* mean_dy, const float* mean_dy_xhat, float* dz) {
    for (uint64_t r = 0; r < n; ++r)
        for (uint32_t c = 0; c < H; ++c) {
            const uint64_t i = r * H + c;
            dz[i] = train_bn_backward(dy[i], xhat[i], train_bn_rstd(var[c]), gamma[c], mean_dy[c], mean_dy_xhat[c]);
        }
}

// P, rpp of train_cols(n, H); S, kps of train_split(rows)
void ts_cols(int n, int H, int* out) {
    const TrainCols t = train_cols(n, H);
    out[0] = t.P;
    out[1] = t.rpp;
}

void ts_split(int rows, int* out) {
    const TrainSplit s = train_split(rows);
    out[0] = s.S;
    out[1] = s.kps;
}

}  // extern "C"
