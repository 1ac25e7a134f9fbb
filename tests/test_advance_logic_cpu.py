"""CPU-only: the index logic of the tree-reuse kernel's move (alpharat_amd/csrc/dev_advance.h: unit -> (node, group), which
words of which group are ids, old id -> new id from the keep bitmap), compiled for the CPU by tests/hostsim_advance and run
unit by unit as the kernel runs it -- in chunks, every load of a chunk before its stores, in place and to a second buffer --
against advance_tree_scalar: all hi x 320 bytes and the count."""
import numpy as np
import pytest

import _advance as A

NIL = A.NIL


def _expect_in_place(rec, keep_root):
    want, cnt = A.sim_scalar(rec, keep_root)
    out, n = A.compact_np(rec, keep_root)  # (the NumPy restatement the GPU test uses says the same)
    assert n == cnt and want[:cnt].tobytes() == out.tobytes() and want[cnt:].tobytes() == rec[cnt:].tobytes()
    return want, cnt


@pytest.mark.parametrize("order", [0, 1, 2], ids=["forward", "reversed", "shuffled"])
@pytest.mark.parametrize("chunk", [2048, 1024, 20, 7, 1])
def test_units_in_chunks_equal_the_scalar_compaction(order, chunk):
    """2048 units is the kernel's chunk (512 threads x 4); 20 is one record, 7 cuts records apart, 1 is unit by unit."""
    cases = [(1, 0, 0), (2, 1, 1), (65, 1, 2), (65, 37, 3), (300, 1, 4), (300, 299, 5), (700, 37, 6), (700, 300, 7), (1500, 1, 8)]
    for hi, keep_root, seed in cases:
        rec = A.random_tree(hi, seed)
        assert (rec[:, A.PAD] != 0).all() and (rec[1:, A.PARENT] < np.arange(1, hi)).all()
        want, cnt = _expect_in_place(rec, keep_root)
        src, dst, got = A.sim_units(rec, keep_root, chunk, order, moved=False, seed=seed)
        assert got == cnt and dst.tobytes() == want.tobytes(), (hi, keep_root, "in place")
        src, dst, got = A.sim_units(rec, keep_root, chunk, order, moved=True, seed=seed)
        assert got == cnt and src.tobytes() == rec.tobytes(), (hi, keep_root, "the source of a moved tree is left alone")
        assert dst[:cnt].tobytes() == want[:cnt].tobytes() and (dst[cnt:] == 0xEEEEEEEE).all(), (hi, keep_root, "moved")


def test_leaf_and_tight_cases():
    rec = A.random_tree(500, 11)
    leaf = A.first_leaf(rec)
    want, cnt = _expect_in_place(rec, leaf)
    assert cnt == 1
    for order in (0, 1, 2):
        assert A.sim_units(rec, leaf, 1024, order, False)[1].tobytes() == want.tobytes()
    # everything from keep_root on is kept: src[n] = n + 1, the tightest in-place case
    rec = A.random_tree(500, 12, under_first_child=True)
    want, cnt = _expect_in_place(rec, 1)
    assert cnt == 499
    for order in (0, 1, 2):
        for chunk in (1024, 20, 3):
            assert A.sim_units(rec, 1, chunk, order, False, seed=5)[1].tobytes() == want.tobytes()


def _bare(hi):
    rec = np.zeros((hi, A.WORDS), np.uint32)
    rec[:, A.KIDS] = NIL
    rec[:, A.PARENT] = NIL
    rec[:, A.PAD] = [[0xA0 + i, 0xB0 + i, 0xC0 + i] for i in range(hi)]
    rec[:, 0] = 100 + np.arange(hi)  # (a word that is no id)
    return rec


def test_three_node_chain_kept_from_its_middle():
    rec = _bare(3)
    rec[0, 52 + 3], rec[1, A.PARENT] = 1, 0
    rec[1, 52 + 24], rec[2, A.PARENT] = 2, 1
    want = _bare(3)
    want[0] = rec[1]
    want[0, A.PARENT], want[0, 52 + 24] = NIL, 1
    want[1] = rec[2]
    want[1, A.PARENT] = 0
    want[2] = rec[2]  # (beyond the count: as it was)
    got, cnt = A.sim_scalar(rec, 1)
    assert cnt == 2 and got.tobytes() == want.tobytes()
    for order in (0, 1, 2):
        src, dst, n = A.sim_units(rec, 1, 1024, order, False)
        assert n == 2 and dst.tobytes() == want.tobytes()
    assert want[0, 0] == 101 and want[1, 0] == 102 and list(want[1, A.PAD]) == [0xA2, 0xB2, 0xC2]


def test_root_with_two_children_keeping_a_leaf():
    rec = _bare(3)
    rec[0, 52], rec[0, 52 + 7] = 1, 2
    rec[1, A.PARENT] = rec[2, A.PARENT] = 0
    for keep_root in (1, 2):
        want = rec.copy()
        want[0] = rec[keep_root]
        want[0, A.PARENT] = NIL
        got, cnt = A.sim_scalar(rec, keep_root)
        assert cnt == 1 and got.tobytes() == want.tobytes()
        for moved in (False, True):
            src, dst, n = A.sim_units(rec, keep_root, 1024, 2, moved, seed=keep_root)
            assert n == 1 and dst[:1].tobytes() == want[:1].tobytes()
            if not moved:
                assert dst.tobytes() == want.tobytes()


def test_which_words_are_ids():
    """adv_id_words through the move: exactly the parent word and the 25 child words of a record change when every id moves."""
    rec = A.random_tree(40, 3, under_first_child=True)
    rec[0, A.KIDS] = NIL
    rec[0, 52] = 1
    _, dst, cnt = A.sim_units(rec, 1, 1024, 0, True)
    assert cnt == 39
    changed = np.nonzero((dst[:39] != rec[1:40]).any(axis=0))[0]
    assert set(changed) <= {A.PARENT, *range(52, 77)} and A.PARENT in changed
    assert dst[:39, A.PAD].tobytes() == rec[1:40, A.PAD].tobytes()
