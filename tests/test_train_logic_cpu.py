"""CPU: alpharat_amd/csrc/dev_train.h -- the text the training kernels run per row and per element -- through
tests/hostsim_train against the float64 restatement (tests/_train_np.py): the heads' loss terms and dOut of every row, the
BatchNorm forward and backward of every element given the float64 column statistics. Inputs are the float64 step's values
rounded to float32; the expectation is the same formula in float64 on those rounded inputs. Bound: 1e-6 relative to
1 + |value| (f32 expf / logf against float64, the bound the validation terms use). And the two partitions of a step
(train_cols, train_split), which fix the order of every sum over the batch, against a table of literals."""
import numpy as np
import pytest

import _train as TR
import _train_np as N

REL = 1e-6

CASES = [("golden", name) for name in TR.GOLDEN] + [("rows", (b, H)) for b in ("5x5 open", "7x5") for H in (32, 64)]


def _case(kind, arg):
    if kind == "golden":
        return TR.golden_case(arg)
    board, H = arg
    total = len(TR.board(board)[1]["value_p1"])
    return TR.shape_case(board, H, 2 * total, 3)  # every row once as P1 sees it and once as P2 does, or the reverse


def _within(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want) / (1.0 + np.abs(want))
    assert err.max() <= REL, (what, float(err.max()))


@pytest.mark.parametrize("kind,arg", CASES, ids=[str(a) for _, a in CASES])
def test_head_terms_of_every_row(kind, arg):
    case = _case(kind, arg)
    if kind == "rows":
        assert case["swap"].any() and not case["swap"].all()
    r = N.step(case)
    n = len(case["observation"])
    pw_n, vw_n = np.float32(case["policy_weight"]) / np.float32(n), np.float32(case["value_weight"]) / np.float32(n)
    out32 = np.asarray(r["head_out"], np.float32)
    terms = TR.sim_heads(out32, case["policy_p1"], case["policy_p2"], case["value_p1"], case["value_p2"], pw_n, vw_n)
    # the same formulas in float64 on the rounded inputs
    o = out32.astype(np.float64)
    t = [np.asarray(case["policy_p1"], np.float64), np.asarray(case["policy_p2"], np.float64)]
    y = np.stack([np.asarray(case["value_p1"], np.float64).reshape(-1), np.asarray(case["value_p2"], np.float64).reshape(-1)], 1)
    for p in (0, 1):
        ls = N._log_softmax(o[:, 5 * p:5 * p + 5])
        _within(terms["ce"][:, p], -(t[p] * ls).sum(axis=1), f"ce{p}")
        _within(terms["dout"][:, 5 * p:5 * p + 5], float(pw_n) * (np.exp(ls) * t[p].sum(axis=1, keepdims=True) - t[p]), f"dl{p}")
    v = N._softplus(o[:, 10:])
    _within(terms["v"], v, "v")
    _within(terms["sq"], (v - y) ** 2, "sq")
    _within(terms["dout"][:, 10:], float(vw_n) * (v - y) / (1.0 + np.exp(-o[:, 10:])), "do")


def test_softplus_threshold():
    """above 20 the value is the input and its derivative 1, as torch's softplus"""
    o = np.zeros((3, 12), np.float32)
    o[:, 10] = [19.5, 20.0, 25.0]
    o[:, 11] = [-30.0, 20.5, 0.0]
    t = np.full((3, 5), 0.2, np.float32)
    y = np.zeros(3, np.float32)
    terms = TR.sim_heads(o, t, t, y, y, 1.0, 1.0)
    assert terms["v"][2, 0] == np.float32(25.0) and terms["dout"][2, 10] == np.float32(25.0)
    assert terms["v"][1, 1] == np.float32(20.5) and terms["dout"][1, 11] == np.float32(20.5)
    o64 = o[:, 10:].astype(np.float64)
    _within(terms["v"], np.where(o64 > 20, o64, np.log1p(np.exp(o64))), "v")


@pytest.mark.parametrize("kind,arg", CASES, ids=[str(a) for _, a in CASES])
def test_batchnorm_of_every_element(kind, arg):
    case = _case(kind, arg)
    r = N.step(case)
    sd = case["sd"]
    for layer, bn in ((1, "trunk.1"), (2, "trunk.5")):
        z = np.asarray(r[f"z{layer}"], np.float32)
        rstd, mu, var = r[f"stats{layer}"]
        var32 = np.asarray(var, np.float32)
        gamma, beta = np.asarray(sd[f"{bn}.weight"], np.float32), np.asarray(sd[f"{bn}.bias"], np.float32)
        y, xhat = TR.sim_bn_forward(z, mu, var32, gamma, beta)
        rstd64 = 1.0 / np.sqrt(var32.astype(np.float64) + np.float64(np.float32(1e-5)))
        xhat64 = (z.astype(np.float64) - mu) * rstd64
        _within(xhat, xhat64, f"xhat{layer}")
        _within(y, gamma.astype(np.float64) * xhat64 + beta, f"y{layer}")
        dy = np.asarray(r[f"dy{layer}"], np.float32)
        mean_dy = np.asarray(r[f"dy{layer}"].mean(axis=0), np.float32)
        mean_dyx = np.asarray((r[f"dy{layer}"] * r[f"xhat{layer}"]).mean(axis=0), np.float32)
        dz = TR.sim_bn_backward(dy, xhat, var32, gamma, mean_dy, mean_dyx)
        g64, x64 = gamma.astype(np.float64), xhat.astype(np.float64)
        want = rstd64 * (dy.astype(np.float64) * g64 - g64 * mean_dy - x64 * (g64 * mean_dyx))
        _within(dz, want, f"dz{layer}")
        # and the rounded chain stays at the float64 step's own dz
        assert np.abs(dz - r[f"dz{layer}"]).max() <= 1e-5 * (1.0 + np.abs(r[f"dz{layer}"]).max())


# rows: (P, rpp, S, kps). The values the drivers computed inline before train_cols and train_split existed, printed from
# those statements; 2, 257, 2049, 4096, 65536 and the split of 131072 also worked out by hand. 131072 is the symmetric
# step's 2n at the row cap: a split only, no step has that many rows in a BatchNorm call.
PARTITIONS = {
    2: (1, 2, 1, 16),
    15: (1, 15, 1, 16),
    16: (1, 16, 1, 16),
    17: (1, 17, 1, 32),
    63: (1, 63, 1, 64),
    64: (1, 64, 1, 64),
    65: (2, 33, 1, 80),
    255: (4, 64, 1, 256),
    256: (4, 64, 1, 256),
    257: (5, 52, 2, 144),
    2047: (32, 64, 8, 256),
    2048: (32, 64, 8, 256),
    2049: (32, 65, 9, 240),
    4096: (32, 128, 16, 256),
    8191: (32, 256, 32, 256),
    8193: (32, 257, 31, 272),
    65535: (32, 2048, 32, 2048),
    65536: (32, 2048, 32, 2048),
    131072: (None, None, 32, 4096),
}


@pytest.mark.parametrize("rows", list(PARTITIONS))
def test_partitions_of_the_batch(rows):
    """every row in exactly one part and one split, within the caps the workspace is sized for, and the same partition as
    ever: another one would sum in another order and change the gradients' bytes"""
    want_P, want_rpp, want_S, want_kps = PARTITIONS[rows]
    S, kps = TR.sim_split(rows)
    assert S <= 32 and kps % 16 == 0 and (S - 1) * kps < rows <= S * kps
    assert (S, kps) == (want_S, want_kps)
    if want_P is not None:
        for H in (32, 256):  # the width is carried along, it decides nothing
            P, rpp = TR.sim_cols(rows, H)
            assert P <= 32 and (P - 1) * rpp < rows <= P * rpp
            assert (P, rpp) == (want_P, want_rpp)
