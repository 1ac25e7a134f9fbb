"""Validation on the CPU: the restatement of the reference's validation numbers (tests/_metrics_np.py) against fixtures the
reference's own functions wrote (tests/golden/metrics, tools/gen_metrics_golden.py); the per-row text of the device
(alpharat_amd/csrc/dev_validate.h, compiled for the CPU by tests/hostsim_validate) against the restatement; the C-ABI and
the Python mirror (alpharat_amd/validate.py) without a device; and the condition the GPU test's fixtures must meet."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import _metrics_np as M
import _validate as V

GOLDEN = sorted((Path(__file__).parent / "golden" / "metrics").glob("*.npz"))
KEYS = {"loss", "loss_p1", "loss_p2", "loss_value", "loss_value_p1", "loss_value_p2", "p1/top1_accuracy", "p1/top2_accuracy",
        "p1/entropy_pred", "p1/entropy_target", "p2/top1_accuracy", "p2/top2_accuracy", "p2/entropy_pred", "p2/entropy_target",
        "value/p1_explained_variance", "value/p1_correlation", "value/p2_explained_variance", "value/p2_correlation"}


def _golden(path):
    z = np.load(path)
    case = {k: z[k] for k in z.files}
    return case, float(z["policy_weight"]), float(z["value_weight"]), dict(zip(z["ref_keys"].tolist(), z["ref_values"].tolist()))


def _valsums(s: dict):
    from alpharat_amd.validate import ValSums

    return ValSums(**s)


# ---- 1. the restatement and the reference's numbers ---------------------------------------------------------------------
def test_the_fixtures_are_the_cases_they_are_there_for():
    names = {p.stem for p in GOLDEN}
    assert names == {"random", "target_ties", "constant_value", "worse_than_mean", "weights", "real_game_5x5"}
    for p in GOLDEN:
        case, pw, vw, ref = _golden(p)
        n = len(case["pred_v1"])
        assert 0 < n <= 256 and n % 3, p.stem  # (batches of 3 with a short last one)
        assert set(ref) == KEYS
        if p.stem == "target_ties":
            t = case["policy_p1"]
            assert ((t == t.max(axis=1, keepdims=True)).sum(axis=1) > 1).mean() > 0.5
        if p.stem == "constant_value":
            assert ref["value/p1_explained_variance"] == 0.0 and ref["value/p1_correlation"] == 0.0
            assert ref["value/p2_correlation"] == 0.0
        if p.stem == "worse_than_mean":
            assert ref["value/p1_explained_variance"] == -1.0 and ref["value/p2_explained_variance"] == -1.0
        if p.stem == "weights":
            assert (pw, vw) == (0.7, 2.5)


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: p.stem)
def test_restatement_equals_the_reference(path):
    """rtol 1e-5, atol 1e-6: the reference works in f32 over at most 256 rows, 256 * 2^-24 = 1.5e-5 is the worst relative
    error of its means. Accuracies are ratios of counts and match exactly (to the f32 the reference returns)."""
    case, pw, vw, ref = _golden(path)
    got = M.metrics(case, pw, vw)
    assert set(got) == KEYS
    for k in sorted(KEYS):
        if k.endswith("accuracy"):
            assert np.float32(got[k]) == np.float32(ref[k]), (k, got[k], ref[k])
        else:
            np.testing.assert_allclose(got[k], ref[k], rtol=1e-5, atol=1e-6, err_msg=k)
    # and ValSums.metrics from the restated sums: the same numbers from moments instead of centred rows
    mine = _valsums(M.sums(case)).metrics(pw, vw)
    assert set(mine) == KEYS
    for k in sorted(KEYS):
        if k.endswith("accuracy"):
            assert mine[k] == got[k], k
        else:
            np.testing.assert_allclose(mine[k], got[k], rtol=1e-9, atol=1e-9, err_msg=k)
            np.testing.assert_allclose(mine[k], ref[k], rtol=1e-5, atol=1e-6, err_msg=k)


def test_one_row_gives_nan_explained_variance():
    case, pw, vw, _ = _golden(GOLDEN[0])
    one = {k: v[:1] for k, v in case.items() if getattr(v, "ndim", 0) >= 1 and not k.startswith("ref_")}
    for m in (M.metrics(one), _valsums(M.sums(one)).metrics()):
        assert np.isnan(m["value/p1_explained_variance"]) and np.isnan(m["value/p2_explained_variance"])
        assert m["value/p1_correlation"] == 0.0 and np.isfinite(m["loss"])


# ---- 2. dev_validate.h on the CPU ---------------------------------------------------------------------------------------
def _seeded_outputs(rows, seed):
    """f32 logits and positive values for the rows; every seventh row gets exact logit ties around the target action"""
    n = len(rows["value_p1"])
    rng = np.random.default_rng(seed)
    out = dict(logits_p1=(2 * rng.standard_normal((n, 5))).astype(np.float32),
               logits_p2=(2 * rng.standard_normal((n, 5))).astype(np.float32),
               value_p1=np.abs(rows["value_p1"] + rng.standard_normal(n)).astype(np.float32),
               value_p2=np.abs(rows["value_p2"] + rng.standard_normal(n)).astype(np.float32))
    for lk, tk in (("logits_p1", "policy_p1"), ("logits_p2", "policy_p2")):
        a = rows[tk].argmax(axis=1)
        for i in range(0, n, 7):
            out[lk][i, (a[i] + 1 + i % 4) % 5] = out[lk][i, a[i]]  # a tie at a lower or a higher index
    return out


@pytest.mark.parametrize("name", list(V.BOARDS), ids=lambda b: b.replace(" ", "_"))
def test_device_text_equals_the_restatement(name):
    games, rows = V.board(name)
    _, w, h, *_ = V.BOARDS[name]
    out = _seeded_outputs(rows, 17)
    case = V.expected_case(rows, out)
    got, terms = V.sim_run(1 if w * h <= 64 else 4, *V.scores(games), rows["policy_p1"], rows["policy_p2"], out["logits_p1"],
                           out["logits_p2"], out["value_p1"], out["value_p2"])
    want = M.sums(case)
    V.assert_sums_close(got, want, 1e-6, name)  # counts exactly; f32 expf / logf against float64
    for p in (0, 1):
        rt = M.row_terms(case, p)
        assert np.array_equal(terms["top1"][:, p] != 0, rt["top1"]) and np.array_equal(terms["top2"][:, p] != 0, rt["top2"])
        assert terms["target"][:, p].tobytes() == rows[("value_p1", "value_p2")[p]].tobytes()  # the subtraction of rows_build_row
        assert terms["pred"][:, p].tobytes() == out[("value_p1", "value_p2")[p]].tobytes()
        np.testing.assert_allclose(terms["ce"][:, p], rt["ce"], rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(terms["ent_pred"][:, p], rt["ent_pred"], rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(terms["ent_target"][:, p], rt["ent_target"], rtol=2e-6, atol=2e-6)
    if name != "one position":  # the fixtures hold what the rule is about
        t = rows["policy_p1"]
        assert ((t == t.max(axis=1, keepdims=True)).sum(axis=1) > 1).any(), "no target tie"
        assert 0 < want["top1"][0] < want["top2"][0] < want["n"]


def test_rank_rule_on_ties():
    """a = first index of the largest target; rank = #{l_k > l_a} + #{k < a : l_k == l_a}"""
    rows = [  # (target, logits, top1, top2)
        ([0.4, 0.4, 0.2, 0, 0], [1, 5, 0, 0, 0], 0, 1),      # target tie: a = 0, not 1; one logit above
        ([0.2, 0.4, 0.4, 0, 0], [0, 5, 9, 0, 0], 0, 1),      # a = 1
        ([0, 0, 1, 0, 0], [3, 0, 3, 0, 0], 0, 1),            # logit tie at a lower index: it ranks first
        ([0, 0, 1, 0, 0], [0, 0, 3, 3, 3], 1, 1),            # ties at higher indices only: a ranks first
        ([0, 0, 1, 0, 0], [3, 3, 3, 0, 0], 0, 0),            # two equal logits in front
        ([0, 0, 0, 0, 1], [2, 2, 2, 2, 2], 0, 0),            # all equal, a last
        ([1, 0, 0, 0, 0], [2, 2, 2, 2, 2], 1, 1),            # all equal, a first
        ([0.2, 0.2, 0.2, 0.2, 0.2], [0, 1, 2, 3, 4], 0, 0),  # uniform target: a = 0
        ([0, 1, 0, 0, 0], [7, 6, 5, 5, 5], 0, 1),
    ]
    n = len(rows)
    t = np.array([r[0] for r in rows], np.float32)
    l = np.array([r[1] for r in rows], np.float32)
    z = np.zeros(n, np.float32)
    got, terms = V.sim_run(1, z, z, z, z, t, t[::-1].copy(), l, l[::-1].copy(), z + 1, z + 1)
    assert terms["top1"][:, 0].tolist() == [r[2] for r in rows] and terms["top2"][:, 0].tolist() == [r[3] for r in rows]
    assert terms["top1"][:, 1].tolist() == [r[2] for r in rows][::-1]
    r = M.ranks(l.astype(np.float64), t.astype(np.float64))
    assert (r < 1).astype(int).tolist() == [x[2] for x in rows] and (r < 2).astype(int).tolist() == [x[3] for x in rows]
    assert got["top1"] == (sum(x[2] for x in rows),) * 2 and got["top2"] == (sum(x[3] for x in rows),) * 2


# ---- 3. the C-ABI and the Python mirror, without a device -----------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from alpharat_amd import _lib

    return _lib.load()


def test_symbol_is_declared_and_exported(lib):
    from alpharat_amd import _lib

    header = (Path(__file__).resolve().parent.parent / "include" / "alpharat_hip.h").read_text()
    assert "int ar_rows_validate(ArRowSet* set, ArNet* net, const uint64_t* rows, uint64_t n, uint32_t chunk_rows" in header
    assert "ar_rows_validate" in _lib.EXPORTS and lib.ar_rows_validate is not None
    # the mirror has the header's layout: n, four pairs of doubles, two pairs of counts, five pairs of doubles
    assert C.sizeof(_lib.ArValSums) == 8 + 11 * 16 and _lib.ArValSums.top1.offset == 8 + 4 * 16
    assert C.sizeof(_lib.ArValRows) == 4 * C.sizeof(C.c_void_p)
    assert (Path(__file__).resolve().parent.parent / "alpharat_amd" / "csrc" / "dev_validate.h").exists()


def test_null_arguments_are_invalid_without_a_device(lib):
    from alpharat_amd import _lib

    sums = _lib.ArValSums()
    sums.n = 77
    fake = C.c_void_p(8)  # never dereferenced: the other argument is null
    assert lib.ar_rows_validate(None, None, None, 0, 0, C.byref(sums), None) == _lib.AR_E_INVALID
    assert lib.ar_rows_validate(None, fake, None, 0, 0, C.byref(sums), None) == _lib.AR_E_INVALID
    assert "null argument" in _lib.last_error()
    assert sums.n == 77  # untouched


def test_valsums_add_and_metrics():
    from alpharat_amd.validate import ValSums

    case, pw, vw, _ = _golden(GOLDEN[0])
    n = len(case["pred_v1"])
    cut = 77
    part = lambda lo, hi: {k: v[lo:hi] for k, v in case.items() if getattr(v, "ndim", 0) >= 1 and not k.startswith("ref_")}  # noqa: E731
    a, b, whole = _valsums(M.sums(part(0, cut))), _valsums(M.sums(part(cut, n))), _valsums(M.sums(case))
    both = a + b
    assert both.n == whole.n == n and both.top1 == whole.top1 and both.top2 == whole.top2
    for k in M.SUM_KEYS:
        np.testing.assert_allclose(getattr(both, k), getattr(whole, k), rtol=1e-12)
    assert (ValSums() + a) == a and ValSums().n == 0
    for k, x in both.metrics(pw, vw).items():
        np.testing.assert_allclose(x, whole.metrics(pw, vw)[k], rtol=1e-9, atol=1e-12, err_msg=k)
    with pytest.raises(ValueError, match="no rows"):
        ValSums().metrics()
    with pytest.raises(TypeError):
        a + 1


# ---- 4. the fixtures of tests/test_gpu_validate.py ------------------------------------------------------------------------
@pytest.mark.parametrize("board,net", V.CASES, ids=V.CASE_IDS)
def test_gpu_fixtures_have_no_ambiguous_rows(board, net):
    """A row is ambiguous when some logit is within 2 (1e-5 + 1e-5 max|l|) of the logit at the target's argmax: an evaluator
    within tolerance may then rank the target action differently. At most 1 % of a pair's rows may be."""
    games, rows = V.board(board)
    _, w, h, *_ = V.BOARDS[board]
    _, forward = V.network(net, w, h)
    want = forward(rows["observation"])
    n = len(rows["value_p1"])
    bad = int(V.ambiguous(want["logits_p1"], rows["policy_p1"]).sum() + V.ambiguous(want["logits_p2"], rows["policy_p2"]).sum())
    assert bad <= 0.01 * n, (board, net, bad, n)
