// The dropout mask of the training steps (train_mlp.h, train_sym.h, train_lv.h): inverted dropout as nn.Dropout applies it
// in training mode, from a counter-based generator. Whether an element is kept is a pure function of
//   (seed, step, call, row, column)
// -- the caller's seed, the count of training steps, the index of the BatchNorm call the dropout follows, and the element's
// place in that call's own [n][H] array -- so it depends on no grid, no row partition and no stream, and nothing is stored:
// the forward writes 0 for a dropped element and the backward reads the mask off the activation (act > 0).
// Plain C++ with no barrier and no HIP call, for host and device as dev_train.h: the kernels call these functions, and the
// CPU harness under tests/hostsim_dropout compiles the same text. All arithmetic is uint64_t and wraps.
//
// This is the project's own generator, not torch's Philox stream: a run is reproducible from (seed, step), it is not
// mask-for-mask equal to a torch run.
#pragma once
#include "dev_rng.h"

namespace ar {

#define AR_DROPOUT_G 0x9e3779b97f4a7c15ULL

// SplitMix64's finaliser (dev_rng.h spells it inside rng_seed)
AR_HD uint64_t dropout_mix(uint64_t v) {
    v = (v ^ (v >> 30)) * 0xbf58476d1ce4e5b9ULL;
    v = (v ^ (v >> 27)) * 0x94d049bb133111ebULL;
    return v ^ (v >> 31);
}

// one key per (seed, step, call): the host forms it once per BatchNorm call
AR_HD uint64_t dropout_key(uint64_t seed, uint64_t step, uint64_t call) {
    return dropout_mix(dropout_mix(dropout_mix(seed + AR_DROPOUT_G) + step * AR_DROPOUT_G + AR_DROPOUT_G) + call * AR_DROPOUT_G +
                       AR_DROPOUT_G);
}

// the 64 bits of element e = row * H + column, row counted within the call's own n rows
AR_HD uint64_t dropout_bits(uint64_t key, uint64_t e) { return dropout_mix(key + (e + 1) * AR_DROPOUT_G); }

// kept iff the upper 32 bits reach the threshold: thr = 0 keeps everything, thr = 2^32 would drop everything
AR_HD bool dropout_keep(uint64_t key, uint64_t thr, uint64_t e) { return (dropout_bits(key, e) >> 32) >= thr; }

// thr = floor(p * 2^32 + 0.5); the kept elements are multiplied by 1 / (1 - p), rounded as torch rounds it
AR_HD uint64_t dropout_thr(float p) { return (uint64_t)floor((double)p * 4294967296.0 + 0.5); }
AR_HD float dropout_scale(float p) { return 1.0f / (float)(1.0 - (double)p); }

// what a kernel receives for one BatchNorm call
struct TrainDrop {
    uint64_t key, thr;
    float scale;
};

}  // namespace ar
