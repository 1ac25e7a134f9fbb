"""CPU: alpharat_amd/csrc/dev_train_lv.h -- the text the LocalValueMLP training kernels add per cell -- through
tests/hostsim_train_lv against the float64 restatement (tests/_train_lv_np.py): a cell's ce and its four dL for every target
class, an inactive cell, logits of +-80 and ties, the scale and the loss at C = 0 and C = 1, and the fixed partition of the
rows. The expectation is the same formula in float64 on the same float32 inputs, to 1e-6 (the bound of
tests/test_train_logic_cpu.py) relative to 1 + |ce| + max|l| for a ce -- dev_ownership.h forms logsumexp = m + log(s) in float32
before the target's logit is taken off, so its rounding is that of a number of the logits' size: 2^-24 * 81.4 = 4.9e-6 at
logits of 80, whatever the ce -- and relative to the scale for a dL, whose factor softmax - onehot lies in [-1, 1]."""
import numpy as np
import pytest

import _train_lv as TL
import _train_lv_np as NL

REL = 1e-6


def _expect(logits, targets, scale):
    ce, dl = zip(*[NL.cell_terms(l, int(t), scale) for l, t in zip(np.asarray(logits, np.float32), targets)])
    return np.array(ce), np.array(dl)


def _check(logits, targets, scale):
    got = TL.sim_cells(logits, targets, scale)
    ce, dl = _expect(logits, targets, scale)
    assert np.isfinite(got["ce"]).all() and np.isfinite(got["dl"]).all()
    size = 1.0 + np.abs(ce) + np.abs(np.asarray(logits, np.float64)).max(axis=1)
    assert (np.abs(got["ce"] - ce) / size).max() <= REL
    assert np.abs(got["dl"].astype(np.float64) - dl).max() <= REL * max(abs(scale), 1e-30)
    return got


def test_every_target_class():
    rng = np.random.default_rng(0)
    logits = rng.standard_normal((64, 4)) * 3.0
    for target in range(4):
        got = _check(logits, np.full(64, target, np.int8), 0.25 / 7)
        assert (got["dl"][:, target] < 0).all() and (np.delete(got["dl"], target, axis=1) > 0).all()
        assert np.abs(got["dl"].sum(axis=1)).max() <= 1e-7  # softmax - onehot sums to zero
        assert (got["ce"] > 0).all()


def test_an_inactive_cell_is_all_zeros():
    logits = np.array([[1.0, -2.0, 3.0, 0.5], [80.0, -80.0, 0.0, 80.0], [np.float32(3e38), 0.0, 0.0, 0.0]], np.float32)
    for target in (-1, -128):
        got = TL.sim_cells(logits, np.full(3, target, np.int8), 0.5)
        assert got.tobytes() == np.zeros(3, TL.CELL).tobytes()  # +0.0 everywhere, whatever the logits


def test_saturated_logits_and_ties():
    logits = np.array([[80.0, -80.0, 0.0, 0.0], [-80.0, 80.0, -80.0, -80.0], [80.0, 80.0, 80.0, 80.0], [0.0, 0.0, 0.0, 0.0],
                       [-80.0, -80.0, -80.0, -80.0], [5.0, 5.0, -3.0, -3.0], [80.0, 80.0, -80.0, -80.0], [1.0, 2.0, 2.0, 1.0]],
                      np.float32)
    for target in range(4):
        got = _check(logits, np.full(len(logits), target, np.int8), 1.0)
        assert np.abs(got["ce"][2:5] - np.log(4.0)).max() <= REL * (1.0 + np.log(4.0) + 80.0)  # four equal logits, wherever
        assert np.array_equal(got["dl"][3], got["dl"][2]) and np.array_equal(got["dl"][3], got["dl"][4])
    got = _check(logits, np.array([1, 0, 0, 0, 0, 0, 0, 0], np.int8), 1.0)
    assert abs(got["ce"][0] - 160.0) <= 1e-4 and abs(got["ce"][1] - 160.0) <= 1e-4  # the target 160 below the maximum
    assert abs(got["dl"][0][1] + 1.0) <= 1e-7 and abs(got["dl"][0][0] - 1.0) <= 1e-7


def test_scale_and_loss_at_zero_and_one_cell():
    assert TL.sim_scale(0.25, 0) == 0.0 and TL.sim_loss(0.0, 0) == 0.0 and TL.sim_loss(3.5, 0) == 0.0
    assert TL.sim_scale(0.25, 1) == 0.25 and TL.sim_loss(3.5, 1) == 3.5
    assert TL.sim_scale(0.25, 7) == float(np.float32(0.25) / np.float32(7)) and TL.sim_loss(3.5, 7) == 3.5 / 7
    assert TL.sim_scale(0.0, 5) == 0.0
    # C = 0: whatever the cells hold, nothing but zeros comes out (every cell of such a window is inactive)
    rng = np.random.default_rng(1)
    got = TL.sim_cells(rng.standard_normal((10, 4)) * 50, np.full(10, -1, np.int8), TL.sim_scale(0.25, 0))
    assert not got["ce"].any() and not got["dl"].any()
    # C = 1: the one active cell carries the whole weight
    l = np.array([[0.3, -1.2, 2.0, 0.1]], np.float32)
    got = _check(l, np.array([2], np.int8), TL.sim_scale(0.25, 1))
    want = NL.cell_terms(l[0], 2, 0.25)
    assert abs(TL.sim_loss(float(got["ce"][0]), 1) - want[0]) <= REL * (1 + want[0])


@pytest.mark.parametrize("name", TL.GOLDEN)
def test_cells_of_the_goldens(name):
    """every cell of a golden, from the reference's float32 logits: the terms, their sum as the loss, dL as the float64 step's"""
    case = TL.golden_case(name)
    r = NL.step(case)
    co = case["cheese_outcomes"].reshape(-1)
    scale = TL.sim_scale(case["ownership_weight"], r["cells"])
    got = _check(case["f32"]["ownership_logits"].reshape(-1, 4), co, scale)
    assert int((co >= 0).sum()) == r["cells"]
    loss = TL.sim_loss(float(got["ce"].astype(np.float64).sum()), r["cells"])
    want = float(case["f64"]["losses"]["loss_ownership"])
    assert abs(loss - want) <= 1e-5 * (1.0 + want)
    assert np.abs(got["dl"] - r["dl"].reshape(-1, 4)).max() <= 1e-5 * scale
    assert not got["dl"][co < 0].any()


def test_partition_of_the_rows():
    for n, hw in ((2, 25), (16, 25), (17, 256), (33, 25), (300, 49), (16384, 49), (16385, 49), (65536, 256), (40000, 165)):
        B, rpb = TL.sim_parts(n, hw)
        assert 1 <= B <= 1024 and (B - 1) * rpb < n <= B * rpb, (n, B, rpb)  # every row in one part, no part empty
    assert TL.sim_parts(2, 25) == (1, 2) and TL.sim_parts(33, 25) == (3, 11) and TL.sim_parts(65536, 256) == (1024, 64)
