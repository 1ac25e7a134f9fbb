"""CPU-only: the pipelined move of the tree-reuse kernel (alpharat_amd/csrc/dev_advance.h), compiled for the CPU by
tests/hostsim_advance_pipe. (a) The source list of every chunk, filled as the block's threads fill it, equals the kept
nodes' old ids. (b) The move with D chunks in flight, the single loads and stores of all threads interleaved at random
under the two rules the kernel keeps, equals the scalar compaction (tests/_advance.py compact_np) byte for byte, in place
and moved."""
import numpy as np
import pytest

import _advance_pipe as P

N = P.CHUNK_NODES
NAMES = [c[0] for c in P.cases()]


def _case(name):
    return next(c for c in P.cases() if c[0] == name)


def test_constants_are_the_headers():
    assert P.sim().ap_chunk_nodes() == N and P.sim().ap_depth() in P.DEPTHS


def test_the_cases_are_what_they_claim():
    for name, rec, keep_root, kept in P.cases():
        out, cnt, ids = P.expect(name)
        assert cnt == kept == len(ids), name
        if name.startswith(("tight", "prefix")):
            assert (ids == np.arange(kept)).all(), name  # (src[n] = n + keep_root: everything from keep_root on)
        if name.startswith("prefix"):
            assert keep_root == 3000
        if name.startswith("sparse"):
            words = np.unique(ids[:N] >> 6)
            assert words[-1] - words[0] >= 75 and len(words) < words[-1] - words[0], name  # (empty words in between)
    counts = {c[3] for c in P.cases() if c[0].startswith("tight")}
    assert counts >= {k * N + d for k in range(1, max(P.DEPTHS) + 2) for d in (-1, 0, 1)}


@pytest.mark.parametrize("name", NAMES)
def test_source_list_of_every_chunk(name):
    _, rec, keep_root, kept = _case(name)
    _, cnt, ids = P.expect(name)
    for seed in (0, 1):
        lists, got = P.sim_lists(rec, keep_root, seed)
        assert got == cnt
        flat = lists.reshape(-1)
        assert (flat[:cnt] == ids).all(), name  # (chunk c's entry k is kept node c * N + k)
        assert (flat[cnt:] == 0xFFFF).all(), name  # (nothing else is written)


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["any-order", "loads-first", "stores-first"])
@pytest.mark.parametrize("depth", P.DEPTHS)
@pytest.mark.parametrize("name", NAMES)
def test_pipelined_move_equals_the_scalar_compaction(name, depth, mode):
    _, rec, keep_root, kept = _case(name)
    out, cnt, _ = P.expect(name)
    src, dst, got = P.sim_move(rec, keep_root, depth, mode, moved=False, seed=depth * 10 + mode)
    assert got == cnt
    assert dst[:cnt].tobytes() == out.tobytes(), (name, "in place")
    assert dst[cnt:].tobytes() == rec[cnt:].tobytes(), (name, "records from the count on are left as they were")
    src, dst, got = P.sim_move(rec, keep_root, depth, mode, moved=True, seed=depth * 10 + mode)
    assert got == cnt and src.tobytes() == rec.tobytes(), (name, "the source of a moved tree is left alone")
    assert dst[:cnt].tobytes() == out.tobytes() and (dst[cnt:] == 0xEEEEEEEE).all(), (name, "moved")
