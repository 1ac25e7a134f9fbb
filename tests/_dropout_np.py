"""The dropout mask of the training steps in NumPy uint64 -- test infrastructure only.

A restatement of alpharat_amd/csrc/dev_dropout.h from its definition: with G = 0x9e3779b97f4a7c15, mix SplitMix64's
finaliser and all arithmetic wrapping at 2^64,

    key(seed, step, call) = mix(mix(mix(seed + G) + step * G + G) + call * G + G)
    bits(key, e)          = mix(key + (e + 1) * G),  e = row * H + column within the call's own n rows
    thr(p)                = floor(p * 2^32 + 0.5)
    keep(e)               = (bits >> 32) >= thr
    scale                 = float32(1) / float32(1 - p)

``p`` reaches the library as a float32, so it is rounded to one before anything is formed from it.
tests/test_dropout_mask_cpu.py holds this file, the header compiled for the host (tests/hostsim_dropout) and literals
worked out from the definition against one another.
"""
from __future__ import annotations

import numpy as np

G = np.uint64(0x9E3779B97F4A7C15)
_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
_MASK64 = (1 << 64) - 1

# the BatchNorm call a dropout follows (include/alpharat_hip.h): PyRatMLP and LocalValueMLP, then SymmetricMLP
MLP_CALLS = ("trunk.3", "trunk.7")
SYM_CALLS = ("shared_encoder.3", "player_encoder.3/p1", "player_encoder.3/p2", "trunk.3/p1", "trunk.3/p2", "trunk.7/p1",
             "trunk.7/p2")


def mix(v):
    """SplitMix64's finaliser over a uint64 array (or scalar)"""
    v = np.asarray(v, np.uint64)
    with np.errstate(over="ignore"):
        v = (v ^ (v >> np.uint64(30))) * _M1
        v = (v ^ (v >> np.uint64(27))) * _M2
    return v ^ (v >> np.uint64(31))


def _u64(x: int):
    return np.uint64(int(x) & _MASK64)


def key(seed: int, step: int, call: int):
    with np.errstate(over="ignore"):
        k = mix(_u64(seed) + G)
        k = mix(k + _u64(step) * G + G)
        return mix(k + _u64(call) * G + G)


def thr(p: float) -> int:
    return int(np.floor(float(np.float32(p)) * 4294967296.0 + 0.5))


def scale(p: float) -> np.float32:
    return np.float32(1.0) / np.float32(1.0 - float(np.float32(p)))


def bits(seed: int, step: int, call: int, n: int, H: int):
    """the 64 bits of every element of the call's [n][H] array"""
    e = np.arange(n * H, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return mix(key(seed, step, call) + (e + np.uint64(1)) * G).reshape(n, H)


def mask(seed: int, step: int, call: int, n: int, H: int, p: float):
    """bool [n][H]: True where the element is kept"""
    return (bits(seed, step, call, n, H) >> np.uint64(32)) >= np.uint64(thr(p))


def masks(seed: int, step: int, calls: int, n: int, H: int, p: float) -> list:
    """the masks of calls 0 .. calls - 1 of one step"""
    return [mask(seed, step, c, n, H, p) for c in range(calls)]
