"""Made-up trees for the tree-reuse tests, the scalar compaction restated in NumPy, and the driver of tests/hostsim_advance
-- test infrastructure only.

A tree is an array [hi, 80] of uint32: node records of twenty 16-byte groups (alpharat_amd/csrc/dev_search.h NodeStats).
Word 47 (word 3 of group 11) is the parent id, words 52..76 are the 25 child ids, words 77..79 are pad."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent / "hostsim_advance"
NIL = 0xFFFFFFFF
WORDS, PARENT, KIDS, PAD = 80, 47, slice(52, 77), slice(77, 80)


def random_tree(hi: int, seed: int, under_first_child: bool = False) -> np.ndarray:
    """Parent ids below child ids, child tables consistent with the parents, every other word random, pad non-zero.
    under_first_child: every node from 2 on descends from node 1 (re-rooting at 1 keeps everything but node 0)."""
    rng = np.random.default_rng(seed)
    rec = rng.integers(1, 1 << 32, size=(hi, WORDS), dtype=np.uint64).astype(np.uint32)
    rec[:, KIDS] = NIL
    rec[0, PARENT] = NIL
    used = [0] * hi  # child slots taken, per node
    lo = 1 if under_first_child else 0
    draws = rng.random(hi)
    slots = rng.integers(0, 25, size=hi)
    for i in range(1, hi):
        p = 0 if i == 1 else lo + int(draws[i] * (i - lo))
        while used[p] == 25:  # (a full table: the next node down)
            p = p + 1 if p + 1 < i else lo
        k = int(slots[i])
        while rec[p, 52 + k] != NIL:
            k = (k + 1) % 25
        rec[p, 52 + k] = i
        rec[i, PARENT] = p
        used[p] += 1
    return rec


def first_leaf(rec: np.ndarray) -> int:
    """the lowest node from 1 on without a child"""
    leaves = np.nonzero((rec[1:, KIDS] == NIL).all(axis=1))[0]
    return int(leaves[0]) + 1


def compact_np(rec: np.ndarray, keep_root: int):
    """advance_tree_scalar restated: (the kept records with their ids mapped, in new-id order; the count)"""
    hi = rec.shape[0]
    parent = rec[:, PARENT].tolist()
    keep = [False] * hi
    keep[keep_root] = True
    for i in range(keep_root + 1, hi):
        p = parent[i]
        keep[i] = p != NIL and keep[p]
    keep = np.asarray(keep)
    fwd = np.where(keep, np.cumsum(keep) - 1, NIL).astype(np.uint32)
    out = rec[keep].copy()
    out[1:, PARENT] = fwd[out[1:, PARENT]]
    out[0, PARENT] = NIL
    kids = out[:, KIDS]
    has = kids != NIL
    kids[has] = fwd[kids[has]]
    out[:, KIDS] = kids
    return out, int(keep.sum())


# ---- tests/hostsim_advance --------------------------------------------------------------------------------------------
_sim = None


def sim() -> C.CDLL:
    global _sim
    if _sim is None:
        subprocess.run(["make", "-s", "-C", str(HERE)], check=True)
        L = C.CDLL(str(HERE / "libadvancesim.so"))
        L.av_scalar.restype = C.c_uint32
        L.av_scalar.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.av_units.restype = C.c_uint32
        L.av_units.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint64]
        _sim = L
    return _sim


def sim_scalar(rec: np.ndarray, keep_root: int):
    """advance_tree_scalar itself, in place: (all hi records afterwards, count)"""
    buf = np.ascontiguousarray(rec.copy())
    cnt = sim().av_scalar(buf.ctypes.data, rec.shape[0], keep_root)
    return buf, int(cnt)


def sim_units(rec: np.ndarray, keep_root: int, chunk_units: int, order: int, moved: bool, seed: int = 0):
    """The move unit by unit with the kernel's index helpers, in chunks of `chunk_units` (loads of a chunk before its
    stores); order 0 forward, 1 reversed, 2 shuffled within a chunk. Returns (source buffer afterwards, destination
    buffer, count); in place they are the same array."""
    src = np.ascontiguousarray(rec.copy())
    dst = np.full_like(src, 0xEEEEEEEE) if moved else src
    cnt = sim().av_units(src.ctypes.data, dst.ctypes.data, rec.shape[0], keep_root, chunk_units, order, seed)
    return src, dst, int(cnt)
