"""CPU: alpharat_amd/csrc/dev_train_sym.h -- the text the SymmetricMLP training kernels add per row and per element --
through tests/hostsim_train_sym against the float64 restatement (tests/_train_sym_np.py): the three inputs as columns of the
flat row (exact: copies), the packed dOut rows of the heads, and every element of dh_1 and dh_2. The arithmetic inputs are the
float64 step's values rounded to float32; the expectation is the same formula in float64 on those rounded inputs, to 1e-6
relative to 1 + |value|, the bound of tests/test_train_logic_cpu.py."""
import numpy as np
import pytest

import _train_sym as TS
import _train_sym_np as NS

REL = 1e-6

CASES = [("golden", name) for name in TS.GOLDEN] + [("rows", s) for s in (TS.SHAPES[4], TS.SHAPES[5], TS.SHAPES[6])]


def _case(kind, arg):
    return TS.golden_case(arg) if kind == "golden" else TS.shape_case(*arg)


def _within(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want) / (1.0 + np.abs(want))
    assert err.max() <= REL, (what, float(err.max()))


@pytest.mark.parametrize("kind,arg", CASES, ids=[str(a) for _, a in CASES])
def test_inputs_are_the_rows_columns(kind, arg):
    case = _case(kind, arg)
    x = np.asarray(case["observation"], np.float32)
    xs, xp = TS.sim_split(x, case["width"], case["height"])
    want_s, want_p = NS.split_inputs(x, case["width"], case["height"])
    assert xs.tobytes() == np.ascontiguousarray(want_s).tobytes()
    assert xp.tobytes() == np.ascontiguousarray(np.concatenate(want_p, axis=0)).tobytes()
    assert not np.array_equal(want_p[0], want_p[1])


@pytest.mark.parametrize("kind,arg", CASES, ids=[str(a) for _, a in CASES])
def test_head_backward_of_every_element(kind, arg):
    case = _case(kind, arg)
    r = NS.step(case)
    n = len(case["observation"])
    dout32 = np.asarray(r["dout"], np.float32)
    d12 = TS.sim_pack(dout32)
    d = dout32.astype(np.float64)
    own = [np.concatenate([d[:, 5 * i:5 * i + 5], d[:, 10 + i:11 + i]], axis=1) for i in (0, 1)]
    for i in (0, 1):
        assert np.array_equal(d12[i * n:(i + 1) * n, :6], own[i].astype(np.float32))
        assert np.array_equal(d12[i * n:(i + 1) * n, 6:], (own[0].astype(np.float32) + own[1].astype(np.float32)))
    wh32 = np.asarray(r["wh"], np.float32)
    H = wh32.shape[1] // 2
    dy = TS.sim_head_dy(d12, wh32)
    p64, w64 = d12.astype(np.float64), wh32.astype(np.float64)
    _within(dy, p64[:, :6] @ w64[:, :H] + p64[:, 6:] @ w64[:, H:], "dh on the rounded inputs")
    # and the rounded chain stays at the float64 step's own dh
    want = np.concatenate(r["dh"], axis=0)
    assert np.abs(dy - want).max() <= 1e-5 * (1.0 + np.abs(want).max())
