"""Trees for the tests of the tree-reuse kernel's pipelined move (alpharat_amd/csrc/dev_advance.h: a source list per chunk
of whole kept nodes, several chunks in flight) and the driver of tests/hostsim_advance_pipe -- test infrastructure only.
Records are those of tests/_advance.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import _advance as A

HERE = Path(__file__).resolve().parent / "hostsim_advance_pipe"
CHUNK_NODES = 51  # N: dev_advance.h ADV_CHUNK_NODES = 512 threads x 2 units / 20 units a node (the CPU test checks it against the header)
DEPTHS = (2, 3)    # D: chunks in flight (the harness runs any depth; dev_advance.h ADV_DEPTH is one of these)


def tree_from_parents(parents, seed: int) -> np.ndarray:
    """Records like A.random_tree's for the given parents (parents[i] < i, at most 25 children each; parents[0] is ignored)."""
    hi = len(parents)
    rng = np.random.default_rng(seed)
    rec = rng.integers(1, 1 << 32, size=(hi, A.WORDS), dtype=np.uint64).astype(np.uint32)
    rec[:, A.KIDS] = A.NIL
    rec[0, A.PARENT] = A.NIL
    slots = rng.integers(0, 25, size=hi)
    for i in range(1, hi):
        p, k = int(parents[i]), int(slots[i])
        while rec[p, 52 + k] != A.NIL:
            k = (k + 1) % 25
        rec[p, 52 + k] = i
        rec[i, A.PARENT] = p
    return rec


class _Family:
    """nodes of one subtree that still have room for a child"""

    def __init__(self, rng, first):
        self.rng, self.open, self.used = rng, [first], {first: 0}

    def parent_for(self, child):
        i = int(self.rng.integers(0, len(self.open)))
        p = self.open[i]
        self.used[p] += 1
        if self.used[p] == 25:
            self.open[i] = self.open[-1]
            self.open.pop()
        self.open.append(child)
        self.used[child] = 0
        return p


def prefix_tree(prefix: int, kept: int, seed: int):
    """(records, keep_root): `prefix` nodes that are all dropped, then `kept` nodes that all descend from node `prefix`"""
    rng = np.random.default_rng(seed)
    low, top = _Family(rng, 0), None
    parents = [0] * (prefix + kept)
    for i in range(1, prefix + kept):
        if i < prefix:
            parents[i] = low.parent_for(i)
        elif i == prefix:
            parents[i] = low.parent_for(i)
            top = _Family(rng, i)
        else:
            parents[i] = top.parent_for(i)
    return tree_from_parents(parents, seed), prefix


def sparse_tree(hi: int, ratio: int, seed: int):
    """(records, keep_root = 2): a root with the children 1 and 2; `ratio` nodes under 1 for every one node under 2, so the
    kept nodes (2's subtree) are far apart in id order and whole bitmap words between them are empty"""
    rng = np.random.default_rng(seed)
    a, b = _Family(rng, 1), _Family(rng, 2)
    parents = [0] * hi
    for i in range(3, hi):
        parents[i] = b.parent_for(i) if (i - 3) % (ratio + 1) == ratio else a.parent_for(i)
    return tree_from_parents(parents, seed), 2


def two_kept_tree(seed: int):
    """(records, keep_root = 40): node 40 has one child, the leaf 49"""
    rng = np.random.default_rng(seed)
    low = _Family(rng, 0)
    parents = [0] * 50
    for i in range(1, 49):
        parents[i] = low.parent_for(i)
        if i == 40:
            low.open.remove(40)
    parents[49] = 40
    return tree_from_parents(parents, seed), 40


_cases = None


def cases():
    """[(name, records, keep_root, kept count)]: built once, never changed"""
    global _cases
    if _cases is not None:
        return _cases
    N, out = CHUNK_NODES, []
    counts = sorted({k * N + d for k in range(1, max(DEPTHS) + 2) for d in (-1, 0, 1)})
    for m in counts:  # everything from keep_root = 1 on is kept: src[n] = n + 1, the tightest in-place case
        out.append((f"tight-{m}", A.random_tree(m + 1, 31 * m, under_first_child=True), 1, m))
    for m in counts:
        rec, k = prefix_tree(3000, m, 17 * m)
        out.append((f"prefix-{m}", rec, k, m))
    for ratio in (200, 100):
        rec, k = sparse_tree(32000, ratio, ratio)
        out.append((f"sparse-{ratio}", rec, k, 1 + len(range(3 + ratio, 32000, ratio + 1))))
    rec = A.random_tree(500, 11)
    out.append(("kept-1", rec, A.first_leaf(rec), 1))
    rec, k = two_kept_tree(5)
    out.append(("kept-2", rec, k, 2))
    for _, rec, _, _ in out:
        rec.setflags(write=False)
    _cases = out
    return out


_expect = {}


def expect(name):
    """compact_np of the named case: (kept records with their ids mapped, count, old ids of the kept nodes relative to keep_root)"""
    if name not in _expect:
        rec, keep_root = next((r, k) for n, r, k, _ in cases() if n == name)
        out, cnt = A.compact_np(rec, keep_root)
        parent = rec[:, A.PARENT].tolist()
        keep = [False] * rec.shape[0]
        keep[keep_root] = True
        for i in range(keep_root + 1, rec.shape[0]):
            keep[i] = parent[i] != A.NIL and keep[parent[i]]
        _expect[name] = (out, cnt, (np.nonzero(keep)[0] - keep_root).astype(np.uint16))
    return _expect[name]


# ---- tests/hostsim_advance_pipe ------------------------------------------------------------------------------------------
_sim = None


def sim() -> C.CDLL:
    global _sim
    if _sim is None:
        subprocess.run(["make", "-s", "-C", str(HERE)], check=True)
        L = C.CDLL(str(HERE / "libadvancepipesim.so"))
        L.ap_chunk_nodes.restype = L.ap_depth.restype = C.c_uint32
        L.ap_lists.restype = C.c_uint32
        L.ap_lists.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64]
        L.ap_move.restype = C.c_uint32
        L.ap_move.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint64]
        _sim = L
    return _sim


def sim_lists(rec: np.ndarray, keep_root: int, seed: int = 0):
    """(the source lists of all chunks, [chunks, CHUNK_NODES] uint16 with 0xFFFF where nothing was written; count)"""
    src = np.ascontiguousarray(rec)
    out = np.full(((rec.shape[0] + CHUNK_NODES - 1) // CHUNK_NODES + 1, CHUNK_NODES), 0xFFFF, np.uint16)
    cnt = int(sim().ap_lists(src.ctypes.data, rec.shape[0], keep_root, out.ctypes.data, seed))
    return out, cnt


def sim_move(rec: np.ndarray, keep_root: int, depth: int, mode: int, moved: bool, seed: int = 0):
    """The pipelined move under one random legal schedule: (source buffer afterwards, destination buffer, count); in
    place they are the same array. mode 0: any order, 1: loads first, 2: stores first."""
    src = np.ascontiguousarray(rec.copy())
    dst = np.full_like(src, 0xEEEEEEEE) if moved else src
    cnt = int(sim().ap_move(src.ctypes.data, dst.ctypes.data, rec.shape[0], keep_root, depth, mode, seed))
    return src, dst, cnt
