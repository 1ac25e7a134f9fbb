"""CPU: the float64 restatements of the PyRatMLP training step (tests/_train_np.py in NumPy, tests/_mlp_torch.py with
autograd) against the reference's own model, loss and backward (tests/golden/train, tools/gen_train_golden.py), and the
ReLU guard of every fixture a gradient is compared on, here or on the device (tests/_train.py)."""
import numpy as np
import pytest

import _train as TR
import _train_np as N

REL = 1e-12


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max()
    assert err <= REL * max(1.0, np.abs(want).max()), (what, err)


def _check(res, want, what):
    for k in N.LOSS_KEYS:
        _close(res["losses"][k], want["losses"][k], f"{what} {k}")
    for k in N.OUT_KEYS:
        _close(res[k], want[k], f"{what} {k}")
    for k in N.PARAM_KEYS:
        _close(res["grads"][k], want["grads"][k], f"{what} grad {k}")
    for k in N.RUNNING_KEYS:
        _close(res["running"][k], want["running"][k], f"{what} {k}")


@pytest.mark.parametrize("name", TR.GOLDEN)
def test_numpy_step_reproduces_the_reference_in_float64(name):
    case = TR.golden_case(name)
    assert case["f64"]["grads"]["trunk.0.weight"].dtype == np.float64
    _check(N.step(case), case["f64"], name)


@pytest.mark.parametrize("name", TR.GOLDEN)
def test_torch_restatement_reproduces_the_reference_in_float64(name):
    import torch

    import _mlp_torch as MT

    case = TR.golden_case(name)
    _check(MT.step(case, torch.float64), case["f64"], name)


@pytest.mark.parametrize("name", TR.GOLDEN)
def test_golden_rows_are_the_boards_rows(name):
    """the device test uploads the board's games and sets the golden's order: the rows must be those"""
    case = TR.golden_case(name)
    again = TR.make_case(case["board"], case["sd"], case["order"], case["swap"])
    for k in ("observation", "policy_p1", "policy_p2", "value_p1", "value_p2"):
        assert np.asarray(again[k]).reshape(-1).tobytes() == np.asarray(case[k]).reshape(-1).tobytes(), k


# ---- the ReLU guard: a condition on the fixtures, not a tolerance ---------------------------------------------------------
@pytest.mark.parametrize("name", TR.GOLDEN)
def test_relu_guard_goldens(name):
    assert N.relu_margin(TR.golden_case(name)) >= TR.MARGIN


@pytest.mark.parametrize("shape", TR.SHAPES, ids=TR.SHAPE_IDS)
def test_relu_guard_shapes(shape):
    assert N.relu_margin(TR.shape_case(*shape)) >= TR.MARGIN


def test_relu_guard_value_family():
    case = TR.value_family_case()
    res = N.step(case)
    assert N.relu_margin(case, res) >= TR.MARGIN
    v = np.concatenate([res["value_p1"], res["value_p2"]])  # softplus(o) is o to 2e-9 from o = 20 on
    assert ((v > 19.5) & (v < 20)).any() and ((v > 20) & (v < 20.5)).any()  # both sides of softplus's threshold
    assert (v > 89).any() and (v < 1e-30).any() and ((v > 1e-3) & (v < 10)).any()


def test_relu_guard_windows_and_swaps():
    _, windows = TR.window_cases()
    for (first, n), case in zip(TR.WINDOWS, windows):
        assert len(case["observation"]) == n
        assert N.relu_margin(case) >= TR.MARGIN, (first, n)
    plain, swapped = TR.swap_cases()
    assert N.relu_margin(plain) >= TR.MARGIN and N.relu_margin(swapped) >= TR.MARGIN
    assert not np.array_equal(plain["observation"], swapped["observation"])


def test_relu_guard_trajectory():
    steps = TR.trajectory_cases_f64()
    assert len(steps) == TR.TRAJ_STEPS
    for i, s in enumerate(steps):
        assert len(s["case"]["observation"]) == TR.TRAJ_BATCH
        assert N.relu_margin(s["case"], s["result"]) >= TR.MARGIN, i
