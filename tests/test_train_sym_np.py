"""CPU: the float64 restatements of the SymmetricMLP training step (tests/_train_sym_np.py in NumPy, tests/_sym_torch.py with
autograd) against the reference's own model, loss and backward (tests/golden/train_sym, tools/gen_train_sym_golden.py), the
ReLU guard of every fixture a gradient is compared on, here or on the device (tests/_train_sym.py), and the network's
symmetry in the step: all rows swapped give the same gradients, with the two players' losses exchanged."""
import numpy as np
import pytest

import _train_sym as TS
import _train_sym_np as NS

REL = 1e-12


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max()
    assert err <= REL * max(1.0, np.abs(want).max()), (what, err)


def _check(res, want, what):
    for k in NS.LOSS_KEYS:
        _close(res["losses"][k], want["losses"][k], f"{what} {k}")
    for k in NS.OUT_KEYS:
        _close(res[k], want[k], f"{what} {k}")
    for k in NS.PARAM_KEYS:
        _close(res["grads"][k], want["grads"][k], f"{what} grad {k}")
    for k in NS.RUNNING_KEYS:
        _close(res["running"][k], want["running"][k], f"{what} {k}")


@pytest.mark.parametrize("name", TS.GOLDEN)
def test_numpy_step_reproduces_the_reference_in_float64(name):
    case = TS.golden_case(name)
    assert case["f64"]["grads"]["trunk.0.weight"].dtype == np.float64
    assert set(case["f64"]["grads"]) == set(NS.PARAM_KEYS) and len(NS.PARAM_KEYS) == 20 and len(NS.RUNNING_KEYS) == 8
    res = NS.step(case)
    assert len(res["bn_out"]) == 7
    _check(res, case["f64"], name)


@pytest.mark.parametrize("name", TS.GOLDEN)
def test_torch_restatement_reproduces_the_reference_in_float64(name):
    import torch

    import _sym_torch as ST

    case = TS.golden_case(name)
    _check(ST.step(case, torch.float64), case["f64"], name)


@pytest.mark.parametrize("name", TS.GOLDEN)
def test_golden_rows_are_the_boards_rows(name):
    """the device test uploads the board's games and sets the golden's order: the rows must be those"""
    case = TS.golden_case(name)
    again = TS.make_case(case["board"], case["sd"], case["order"], case["swap"])
    for k in ("observation", "policy_p1", "policy_p2", "value_p1", "value_p2"):
        assert np.asarray(again[k]).reshape(-1).tobytes() == np.asarray(case[k]).reshape(-1).tobytes(), k


# ---- the ReLU guard: a condition on the fixtures, not a tolerance ---------------------------------------------------------
@pytest.mark.parametrize("name", TS.GOLDEN)
def test_relu_guard_goldens(name):
    assert NS.relu_margin(TS.golden_case(name)) >= TS.MARGIN


@pytest.mark.parametrize("shape", TS.SHAPES, ids=TS.SHAPE_IDS)
def test_relu_guard_shapes(shape):
    assert NS.relu_margin(TS.shape_case(*shape)) >= TS.MARGIN


def test_relu_guard_windows_and_swaps():
    _, windows = TS.window_cases()
    for (first, n), case in zip(TS.WINDOWS, windows):
        assert len(case["observation"]) == n
        assert NS.relu_margin(case) >= TS.MARGIN, (first, n)
    plain, swapped = TS.swap_cases()
    assert NS.relu_margin(plain) >= TS.MARGIN and NS.relu_margin(swapped) >= TS.MARGIN
    assert not np.array_equal(plain["observation"], swapped["observation"])


def test_relu_guard_trajectory():
    steps = TS.trajectory_cases_f64()
    assert len(steps) == TS.TRAJ_STEPS
    for i, s in enumerate(steps):
        assert len(s["case"]["observation"]) == TS.TRAJ_BATCH and not s["case"]["swap"].any()
        assert NS.relu_margin(s["case"], s["result"]) >= TS.MARGIN, i


# ---- the symmetry of the network, in the step ------------------------------------------------------------------------------
def test_all_swapped_rows_give_the_unswapped_gradients():
    plain, swapped = TS.swap_cases()
    a, b = NS.step(plain), NS.step(swapped)
    for k in NS.PARAM_KEYS:
        scale = max(1.0, np.abs(a["grads"][k]).max())
        assert np.abs(a["grads"][k] - b["grads"][k]).max() <= 1e-10 * scale, k
    for k, other in (("loss_p1", "loss_p2"), ("loss_value_p1", "loss_value_p2"), ("loss_value", "loss_value"), ("loss", "loss")):
        assert abs(a["losses"][k] - b["losses"][other]) <= 1e-12 * max(1.0, abs(a["losses"][k])), k
    assert abs(a["losses"]["loss_p1"] - a["losses"]["loss_p2"]) > 1e-6  # the exchange is not vacuous
    assert np.abs(a["logits_p1"] - b["logits_p2"]).max() <= 1e-10 and np.abs(a["logits_p1"] - b["logits_p1"]).max() > 1e-3
