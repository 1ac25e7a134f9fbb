"""CPU: the float64 restatements of the LocalValueMLP training step (tests/_train_lv_np.py in NumPy, tests/_lv_torch.py with
autograd) against the reference's own model, loss and backward (tests/golden/train_lv, tools/gen_train_lv_golden.py), the
ReLU guard of every fixture a gradient is compared on, here or on the device (tests/_train_lv.py), and what the third term
does and does not touch: with ``ownership_weight`` 0 the fourteen gradients are PyRatMLP's, and a window without an active
cell follows the reference's early return."""
import numpy as np
import pytest

import _train_lv as TL
import _train_lv_np as NL
import _train_np as N

REL = 1e-12


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max()
    assert err <= REL * max(1.0, np.abs(want).max()), (what, err)


def _check(res, want, what):
    for k in NL.LOSS_KEYS:
        _close(res["losses"][k], want["losses"][k], f"{what} {k}")
    for k in NL.OUT_KEYS:
        _close(res[k], want[k], f"{what} {k}")
    for k in NL.PARAM_KEYS:
        _close(res["grads"][k], want["grads"][k], f"{what} grad {k}")
    for k in NL.RUNNING_KEYS:
        _close(res["running"][k], want["running"][k], f"{what} {k}")


@pytest.mark.parametrize("name", TL.GOLDEN)
def test_numpy_step_reproduces_the_reference_in_float64(name):
    case = TL.golden_case(name)
    assert case["f64"]["grads"]["ownership_head.2.weight"].dtype == np.float64
    assert set(case["f64"]["grads"]) == set(NL.PARAM_KEYS) and len(NL.PARAM_KEYS) == 18 and len(NL.LOSS_KEYS) == 7
    assert (case["policy_weight"], case["value_weight"], case["ownership_weight"]) == (1.0, 0.5, 0.25)
    res = NL.step(case)
    assert 0 < res["cells"] < case["cheese_outcomes"].size  # active and inactive cells
    _check(res, case["f64"], name)


@pytest.mark.parametrize("name", TL.GOLDEN)
def test_torch_restatement_reproduces_the_reference_in_float64(name):
    import torch

    import _lv_torch as LT

    case = TL.golden_case(name)
    _check(LT.step(case, torch.float64), case["f64"], name)


@pytest.mark.parametrize("name", TL.GOLDEN)
def test_golden_rows_are_the_boards_rows(name):
    """the device test uploads the board's games and sets the golden's order: the rows must be those"""
    case = TL.golden_case(name)
    again = TL.make_case(case["board"], case["sd"], case["order"], case["swap"])
    for k in ("observation", "policy_p1", "policy_p2", "value_p1", "value_p2", "cheese_outcomes"):
        assert np.asarray(again[k]).reshape(-1).tobytes() == np.asarray(case[k]).reshape(-1).tobytes(), k


def test_the_goldens_logits_tell_classes_apart():
    for name in TL.GOLDEN:
        l = TL.golden_case(name)["f64"]["ownership_logits"]
        assert (l.max(axis=-1) - l.min(axis=-1)).mean() > 1.0, name


# ---- the ReLU guard: a condition on the fixtures, not a tolerance ---------------------------------------------------------
@pytest.mark.parametrize("name", TL.GOLDEN)
def test_relu_guard_goldens(name):
    assert NL.relu_margin(TL.golden_case(name)) >= TL.MARGIN


@pytest.mark.parametrize("shape", TL.SHAPES, ids=TL.SHAPE_IDS)
def test_relu_guard_shapes(shape):
    case = TL.shape_case(*shape)
    assert NL.relu_margin(case) >= TL.MARGIN
    assert N.relu_margin(TL.mlp_case(case)) >= TL.MARGIN  # the fourteen-gradient comparison at ownership_weight 0


def test_relu_guard_windows_and_swaps():
    _, windows = TL.window_cases()
    for (first, n), case in zip(TL.WINDOWS, windows):
        assert len(case["observation"]) == n
        assert NL.relu_margin(case) >= TL.MARGIN, (first, n)
    plain, swapped = TL.swap_cases()
    assert NL.relu_margin(plain) >= TL.MARGIN and NL.relu_margin(swapped) >= TL.MARGIN
    assert not np.array_equal(plain["observation"], swapped["observation"])


def test_relu_guard_trajectory():
    steps = TL.trajectory_cases_f64()
    assert len(steps) == TL.TRAJ_STEPS
    for i, s in enumerate(steps):
        assert len(s["case"]["observation"]) == TL.TRAJ_BATCH
        assert NL.relu_margin(s["case"], s["result"]) >= TL.MARGIN, i
    assert any(s["case"]["swap"].any() for s in steps) and not all(s["case"]["swap"].all() for s in steps)  # augmented


# ---- the third term ----------------------------------------------------------------------------------------------------------
def test_swapped_rows_exchange_the_outer_classes():
    plain, swapped = TL.swap_cases()
    a, b = plain["cheese_outcomes"].astype(int), swapped["cheese_outcomes"].astype(int)
    assert np.array_equal(a >= 0, b >= 0) and (a >= 0).any()
    assert np.array_equal(b, np.where(a == 0, 3, np.where(a == 3, 0, a)))
    assert (a == 0).any() or (a == 3).any()  # the exchange is not vacuous


def test_ownership_weight_zero_gives_the_mlps_gradients():
    case = TL.shape_case(*TL.SHAPES[2])
    zero = NL.step(dict(case, ownership_weight=0.0))
    mlp = N.step(TL.mlp_case(case))
    for k in N.PARAM_KEYS:
        _close(zero["grads"][k], mlp["grads"][k], k)
    for k in NL.OWN_KEYS:
        assert not zero["grads"][k].any(), k
    assert zero["losses"]["loss_ownership"] > 0 and abs(zero["losses"]["loss"] - mlp["losses"]["loss"]) <= 1e-12
    full = NL.step(case)
    assert np.abs(full["grads"]["trunk.0.weight"] - mlp["grads"]["trunk.0.weight"]).max() > 1e-6  # the head reaches the trunk


def test_a_window_without_an_active_cell():
    """the reference's early return (losses/ownership.py:35-37): loss_ownership 0, nothing flows back from the head"""
    import torch

    import _lv_torch as LT

    case = TL.shape_case(*TL.SHAPES[1])
    case = dict(case, cheese_outcomes=np.full_like(case["cheese_outcomes"], -1))
    res, ref = NL.step(case), LT.step(case, torch.float64)
    mlp = N.step(TL.mlp_case(case))
    assert res["cells"] == 0 and res["losses"]["loss_ownership"] == 0.0 and float(ref["losses"]["loss_ownership"]) == 0.0
    for k in NL.OWN_KEYS:
        assert not res["grads"][k].any() and not ref["grads"][k].any(), k
    for k in N.PARAM_KEYS:
        _close(res["grads"][k], mlp["grads"][k], k)
        _close(ref["grads"][k], mlp["grads"][k], k)


def test_rows_whose_cell_is_never_active_get_no_gradient():
    case = TL.shape_case(*TL.SHAPES[1])
    res = NL.step(case)
    never = ~res["active"].any(axis=0)  # (hw,)
    assert never.any() and not never.all()
    g = res["grads"]["ownership_head.2.weight"].reshape(len(never), 4, -1)
    assert not g[never].any() and not res["grads"]["ownership_head.2.bias"].reshape(-1, 4)[never].any()
    assert all(g[c].any() for c in np.flatnonzero(~never))
