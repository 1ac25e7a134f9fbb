"""CPU: the float64 restatements of the three training steps with dropout (tests/_train_dropout_np.py in NumPy,
tests/_train_dropout_torch.py with autograd) against the reference's own models, losses and backward with the same masks
hooked onto their ``nn.Dropout`` modules (tests/golden/train_dropout, tools/gen_train_dropout_golden.py); the stored masks
are those of tests/_dropout_np.py; the ReLU guard of every fixture a gradient is compared on, here or on the device
(tests/_train_dropout.py); and with no element dropped the restatements are the existing ones, bit for bit."""
import numpy as np
import pytest

import _dropout_np as D
import _train_dropout as TD
import _train_dropout_np as ND

REL = 1e-12


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max()
    assert err <= REL * max(1.0, np.abs(want).max()), (what, err)


def _check(arch, res, want, what):
    K = TD.KEYS[arch]
    for k in K.LOSS_KEYS:
        _close(res["losses"][k], want["losses"][k], f"{what} {k}")
    for k in K.OUT_KEYS:
        _close(res[k], want[k], f"{what} {k}")
    for k in K.PARAM_KEYS:
        _close(res["grads"][k], want["grads"][k], f"{what} grad {k}")
    for k in K.RUNNING_KEYS:
        _close(res["running"][k], want["running"][k], f"{what} {k}")


@pytest.mark.parametrize("name", TD.GOLDEN)
def test_numpy_step_reproduces_the_reference_in_float64(name):
    case = TD.golden_case(name)
    arch = case["arch"]
    assert case["f64"]["grads"]["trunk.0.weight"].dtype == np.float64
    assert any(not m.all() for m in case["masks"])  # something is dropped
    _check(arch, ND.STEPS[arch](case), case["f64"], name)


@pytest.mark.parametrize("name", TD.GOLDEN)
def test_torch_restatement_reproduces_the_reference_in_float64(name):
    import torch

    import _train_dropout_torch as DT

    case = TD.golden_case(name)
    _check(case["arch"], DT.step(case["arch"], case, torch.float64), case["f64"], name)


@pytest.mark.parametrize("name", TD.GOLDEN)
def test_stored_masks_are_the_generators(name):
    case = TD.golden_case(name)
    n, H = len(case["observation"]), case["hidden"]
    assert case["p"] == float(np.float32(0.5 if name.endswith("p50") else 0.1))
    assert len(case["masks"]) == TD.N_CALLS[case["arch"]]
    for call, m in enumerate(case["masks"]):
        want = D.mask(case["dropout_seed"], case["dropout_step"], call, n, H, case["p"])
        assert m.shape == (n, H) and m.tobytes() == want.tobytes(), call
        assert m.tobytes() == TD.sim_mask(case["dropout_seed"], case["dropout_step"], call, n, H, case["p"]).tobytes(), call


@pytest.mark.parametrize("name", TD.GOLDEN)
def test_golden_rows_are_the_boards_rows(name):
    """the device test uploads the board's games and sets the golden's order: the rows must be those"""
    case = TD.golden_case(name)
    again = TD.FIXTURES[case["arch"]].make_case(case["board"], case["sd"], case["order"], case["swap"])
    rows = ("observation", "policy_p1", "policy_p2", "value_p1", "value_p2") + (("cheese_outcomes",) if case["arch"] == "local_value" else ())
    for k in rows:
        assert np.asarray(again[k]).reshape(-1).tobytes() == np.asarray(case[k]).reshape(-1).tobytes(), k


# ---- the ReLU guard: a condition on the fixtures, not a tolerance ---------------------------------------------------------
@pytest.mark.parametrize("name", TD.GOLDEN)
def test_relu_guard_goldens(name):
    case = TD.golden_case(name)
    assert ND.relu_margin(case["arch"], case) >= TD.MARGIN


@pytest.mark.parametrize("shape", TD.SHAPES, ids=TD.SHAPE_IDS)
def test_relu_guard_shapes(shape):
    arch, index, seed = shape
    case = TD.shape_case(arch, index, seed)
    assert len(case["masks"]) == TD.N_CALLS[arch] and any(not m.all() for m in case["masks"])
    assert ND.relu_margin(arch, case) >= TD.MARGIN


def test_shapes_are_the_ones_asked_for():
    for arch in TD.ARCHS:
        got = {(s[2], s[1]) for s in (TD.FIXTURES[arch].SHAPES[i] for i in TD.SHAPE_INDEX[arch])}  # (n, H)
        assert {n for n, _ in got} >= {2, 33, 129, 300}, arch
        assert 256 in {H for _, H in got}, arch
    assert (300, 256) in {(s[2], s[1]) for s in (TD.FIXTURES["mlp"].SHAPES[i] for i in TD.SHAPE_INDEX["mlp"])}


@pytest.mark.parametrize("arch", TD.ARCHS)
def test_relu_guard_two_steps_of_one_order(arch):
    cases = TD.iter_cases(arch)
    assert [len(c["observation"]) for c in cases] == [TD.ITER_BATCH] * 2
    for step, c in enumerate(cases):
        masked = ND.with_masks(c, TD.ITER_DROPOUT_SEED[arch], step, TD.P, TD.N_CALLS[arch])
        assert ND.relu_margin(arch, masked) >= TD.MARGIN, step


# ---- nothing dropped: the existing restatements, exactly ------------------------------------------------------------------
@pytest.mark.parametrize("arch", TD.ARCHS)
def test_p_zero_is_the_existing_restatement_exactly(arch):
    plain = TD.plain_shape_case(arch, 1)
    case = ND.with_masks(plain, 5, 3, 0.0, TD.N_CALLS[arch])
    assert case["scale"] == 1.0 and all(m.all() for m in case["masks"])
    got, want = ND.STEPS[arch](case), ND.PLAIN[arch].step(plain)
    K = TD.KEYS[arch]
    for k in K.LOSS_KEYS:
        assert np.asarray(got["losses"][k]).tobytes() == np.asarray(want["losses"][k]).tobytes(), k
    for k in K.OUT_KEYS:
        assert got[k].tobytes() == want[k].tobytes(), k
    for k in K.PARAM_KEYS:
        assert got["grads"][k].tobytes() == want["grads"][k].tobytes(), k
    for k in K.RUNNING_KEYS:
        assert got["running"][k].tobytes() == want["running"][k].tobytes(), k


@pytest.mark.parametrize("arch", TD.ARCHS)
def test_a_dropped_element_is_zero_and_a_kept_one_scaled(arch):
    case = TD.shape_case(arch, 1, TD.SHAPE_DROPOUT_SEED[arch][1])
    res = ND.STEPS[arch](case)
    acts = res["acts"] if arch == "symmetric" else [res["a1"], res["a2"]]
    pre = res["bn_out"] if arch == "symmetric" else [res["y1"], res["y2"]]
    for a, y, m in zip(acts, pre, case["masks"]):
        assert (a[~m] == 0).all()
        np.testing.assert_array_equal(a[m], np.maximum(y, 0.0)[m] * case["scale"])
