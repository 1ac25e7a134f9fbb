// TEST HARNESS -- runs alpharat_amd/csrc/dev_dropout.h on the CPU: the key of a BatchNorm call, the threshold and the scale
// as the host drivers form them, and keep() of every element of a call's [n][H] array (one lane per element in
// k_train_bn_apply_drop and k_train_dropout_mask), with a loop where the device has lanes. It is NOT a CPU fallback: nothing
// in alpharat_amd/ loads this file.
#include <cstdint>

#include "../../alpharat_amd/csrc/dev_dropout.h"

using namespace ar;

extern "C" {

uint64_t ds_key(uint64_t seed, uint64_t step, uint32_t call) { return dropout_key(seed, step, (uint64_t)call); }
uint64_t ds_thr(float p) { return dropout_thr(p); }
float ds_scale(float p) { return dropout_scale(p); }
uint64_t ds_mix(uint64_t v) { return dropout_mix(v); }

// keep [n][H] bytes: 1 kept, 0 dropped; bits [n][H] (may be null): the element's 64 bits
void ds_mask(uint64_t seed, uint64_t step, uint32_t call, uint64_t n, uint32_t H, float p, uint8_t* keep, uint64_t* bits) {
    const uint64_t key = dropout_key(seed, step, (uint64_t)call), thr = dropout_thr(p);
    for (uint64_t e = 0; e < n * H; ++e) {
        keep[e] = dropout_keep(key, thr, e) ? 1 : 0;
        if (bits) bits[e] = dropout_bits(key, e);
    }
}

}  // extern "C"
