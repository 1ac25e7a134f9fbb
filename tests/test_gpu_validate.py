"""Validation on the device: ar_rows_validate (k_val_requests, the evaluators, k_val_terms, k_val_sum), RowSet.validate /
RowDataset.validate and alpharat_amd/validate.py, against the float64 restatement of the reference's validation numbers
(tests/_metrics_np.py, tied to the reference by tests/golden/metrics) over the expected forward of every network
(tests/_mlp_np.py, tests/_katago_np.py, the oracle's forward). The rows are the oracle games of tests/_rows.py BOARDS,
uploaded with add_games; tests/test_validate_cpu.py checks that no row of these fixtures has a logit within tolerance of
the logit at its target action."""
import numpy as np
import pytest
import torch  # before anything loads libalpharat_hip: a process brings up one HIP runtime, and torch ships its own

import _metrics_np as M
import _rows as T
import _rows_np as R
import _validate as V
from _random_nets import positions, pyrat

pytestmark = pytest.mark.gpu

OUT_KEYS = ("logits_p1", "logits_p2", "value_p1", "value_p2")


@pytest.fixture(scope="module")
def sets():
    """board name -> (an uploaded RowSet, the games, stack_rows(games)); stored position i is row i"""
    from alpharat_amd.shards import RowSet

    made = {}

    def get(name):
        if name not in made:
            games, rows = V.board(name)
            _, w, h, *_ = V.BOARDS[name]
            rs = RowSet(w, h, len(rows["value_p1"]))
            rs.add_games(games)
            made[name] = (rs, games, rows)
        return made[name]

    yield get
    for rs, _, _ in made.values():
        rs.close()


@pytest.fixture(scope="module")
def mlp55(tmp_path_factory):
    """random_mlp H = 64 on 5x5: (blob, expected forward)"""
    return V.network("random_mlp_h64", 5, 5, tmp_path_factory.mktemp("mlp55"))


def _net(blob):
    from alpharat_amd.nets import Net

    return Net(blob)


def _same(a, b, what=""):
    """two (ValSums, per-row outputs): the same bytes"""
    assert a[0] == b[0], (what, a[0], b[0])
    for k in OUT_KEYS:
        assert a[1][k].tobytes() == b[1][k].tobytes(), (what, k)


def _check_against_outputs(sums, out, rows, index=None, what=""):
    """the reduction on its own: the sums are the restatement's over the returned f32 outputs and the rows' targets --
    counts exactly, double sums to 1e-6 relative (f32 expf / logf against float64)"""
    case = V.expected_case(rows, out, index)
    V.assert_sums_close(V.sums_of(sums), M.sums(case), 1e-6, what)
    return case


@pytest.mark.parametrize("board,net", V.CASES, ids=V.CASE_IDS)
def test_outputs_sums_and_metrics(board, net, sets, tmp_path):
    rs, games, rows = sets(board)
    _, w, h, *_ = V.BOARDS[board]
    blob, forward = V.network(net, w, h, tmp_path)
    n = len(rows["value_p1"])
    assert rs.count() == (len(games), n)
    dev = _net(blob)
    sums, out = rs.validate(dev, np.arange(n), return_rows=True)
    assert sums.n == n and out["logits_p1"].shape == (n, 5) and out["value_p2"].shape == (n,)
    want = forward(rows["observation"])
    # 1. per-row outputs at the project's tolerance
    for k in OUT_KEYS:
        np.testing.assert_allclose(out[k], want[k], atol=1e-5, rtol=1e-5, err_msg=f"{board} {net} {k}")
    # 2. the reduction on its own
    case_out = _check_against_outputs(sums, out, rows, what=f"{board} {net}")
    # 3. end to end: metrics() against the restatement over the expected float64 forward. With d_l = 1e-5 (1 + max|l|) and
    # d_v = 1e-5 (1 + |v|) the outputs' tolerances, a row's cross-entropy moves by at most 2 d_l (|l_k - lse| is 1-Lipschitz in
    # each of l and lse), its predicted entropy by (2 + max|l|) d_l, its squared error by 2 |v - y| d_v + d_v^2; means move
    # by the mean of the rows' bounds. 1e-6 on top covers f32 expf / logf and the f32 terms.
    got, exp = sums.metrics(), M.metrics(V.expected_case(rows, want))
    bound = {}
    ambiguous = 0
    for p, name in enumerate(("p1", "p2")):
        l, v, y = want[f"logits_{name}"], want[f"value_{name}"], rows[f"value_{name}"].astype(np.float64)
        lmax = np.abs(l).max(axis=1)
        d_l, d_v = 1e-5 * (1 + lmax), 1e-5 * (1 + np.abs(v))
        bound[f"loss_{name}"] = (2 * d_l).mean() + 1e-6
        bound[f"{name}/entropy_target"] = (2 * d_l).mean() + 1e-6
        bound[f"{name}/entropy_pred"] = ((2 + lmax) * d_l).mean() + 1e-6
        bound[f"loss_value_{name}"] = (2 * np.abs(v - y) * d_v + d_v ** 2).mean() + 1e-6
        ambiguous += int(V.ambiguous(l, rows[f"policy_{name}"]).sum())
    bound["loss_value"] = 0.5 * (bound["loss_value_p1"] + bound["loss_value_p2"])
    bound["loss"] = bound["loss_p1"] + bound["loss_p2"] + bound["loss_value"]
    for k, b in bound.items():
        print(f"{board} {net} {k}: got {got[k]:.9g} want {exp[k]:.9g} diff {abs(got[k] - exp[k]):.3g} bound {b:.3g}")
        assert abs(got[k] - exp[k]) <= b, (board, net, k, got[k], exp[k], b)
    assert ambiguous <= 0.01 * n
    for name in ("p1", "p2"):
        for k in ("top1_accuracy", "top2_accuracy"):
            assert abs(round(got[f"{name}/{k}"] * n) - round(exp[f"{name}/{k}"] * n)) <= ambiguous, (board, net, name, k)
    # explained variance and correlation are ratios of centred moments, for which the issue's row-wise bounds do not compose:
    # they are compared with the restatement over the *returned* outputs, where both sides work in double on the same f32
    # numbers and differ only in the moment form (relative error n eps sum v^2 / centred sum, far below 1e-6 here)
    from_out = M.metrics(case_out)
    for k in ("value/p1_explained_variance", "value/p1_correlation", "value/p2_explained_variance", "value/p2_correlation"):
        if np.isnan(from_out[k]):
            assert n == 1 and np.isnan(got[k]), (board, net, k)
        else:
            assert abs(got[k] - from_out[k]) <= 1e-6, (board, net, k, got[k], from_out[k])
    dev.close()


@pytest.mark.parametrize("board", list(V.BOARDS), ids=lambda b: b.replace(" ", "_"))
def test_chunking_and_reproducibility(board, sets, tmp_path):
    rs, games, rows = sets(board)
    _, w, h, *_ = V.BOARDS[board]
    blob, _ = V.network("random_mlp_h64", w, h, tmp_path)
    dev = _net(blob)
    n = len(rows["value_p1"])
    idx = np.arange(n)
    base = rs.validate(dev, idx, chunk_rows=0, return_rows=True)
    _same(rs.validate(dev, idx, chunk_rows=0, return_rows=True), base, "the same call twice")
    assert rs.validate(dev, idx) == base[0]  # without the per-row outputs
    for chunk in (1, 32, 50):
        got = rs.validate(dev, idx, chunk_rows=chunk, return_rows=True)
        V.assert_sums_close(V.sums_of(got[0]), V.sums_of(base[0]), 1e-9, f"{board} chunk_rows={chunk}")
        for k in OUT_KEYS:
            np.testing.assert_allclose(got[1][k], base[1][k], atol=1e-5, rtol=1e-5, err_msg=f"chunk_rows={chunk} {k}")
        _same(rs.validate(dev, idx, chunk_rows=chunk, return_rows=True), got, f"chunk_rows={chunk} twice")
    dev.close()


def test_row_selection(sets, mlp55):
    from alpharat_amd.dataset import RowDataset

    rs, games, rows = sets("5x5 open")
    dev = _net(mlp55[0])
    n = len(rows["value_p1"])
    whole = rs.validate(dev, np.arange(n), return_rows=True)
    rng = np.random.default_rng(3)
    train, val = RowDataset(rs).split(0.25, 42)
    assert 0 < len(val) < n and len(train) + len(val) == n
    requests = dict(permuted=rng.permutation(n), repeated=rng.integers(0, n, size=2 * n + 3), subset=val.positions.astype(np.int64))
    for what, index in requests.items():
        sums, out = rs.validate(dev, index, return_rows=True)
        assert sums.n == len(index)
        for k in OUT_KEYS:  # a row's outputs do not depend on its neighbours in the request
            np.testing.assert_allclose(out[k], whole[1][k][index], atol=1e-5, rtol=1e-5, err_msg=f"{what} {k}")
        _check_against_outputs(sums, out, rows, index, what)
    assert val.validate(dev) == rs.validate(dev, val.positions)
    assert (train.validate(dev) + val.validate(dev)).n == n
    V.assert_sums_close(V.sums_of(train.validate(dev) + val.validate(dev)),
                        V.sums_of(rs.validate(dev, np.concatenate([train.positions, val.positions]))), 1e-9, "train + val")
    dev.close()


def test_attached_set_equals_uploaded_set(mlp55):
    """a SelfPlaySession appends its games on the device; validating that set is, byte for byte, validating a second set
    fed the sink's records -- both listed by game index"""
    from alpharat_amd.sampling import SelfPlaySession
    from alpharat_amd.shards import RowSet

    kw = dict(width=5, height=5, cheese_count=5, max_turns=30, num_games=24, simulations=40, concurrent_games=8)
    sink = []
    attached = RowSet(5, 5, kw["num_games"] * kw["max_turns"])
    with SelfPlaySession(output_dir=None, batch_size=8, seed=3, on_game=sink.append, **kw) as s:
        s.attach_rows(attached)
        s.run_to_end()
    sink.sort(key=lambda g: g["game_index"])
    n = sum(g["n"] for g in sink)
    uploaded = RowSet(5, 5, n)
    uploaded.add_games(sink)
    dev = _net(mlp55[0])

    def listed(rs):
        gi, fr, nr = rs.games()
        return np.concatenate([fr[g] + np.arange(nr[g], dtype=np.uint64) for g in np.argsort(gi, kind="stable")])

    a = attached.validate(dev, listed(attached), return_rows=True)
    u = uploaded.validate(dev, listed(uploaded), return_rows=True)
    assert a[0].n == n > 0
    _same(a, u, "attached against uploaded")
    _check_against_outputs(a[0], a[1], R.stack_rows(sink), what="attached")
    dev.close()
    attached.close()
    uploaded.close()


def test_net_state_survives(sets, mlp55, tmp_path):
    rs_a, _, rows_a = sets("5x5 open")
    rs_b, _, rows_b = sets("one position")  # other 5x5 games
    blob = mlp55[0]
    dev = _net(blob)
    three = [pyrat(og) for og in positions(5, 5, 3, seed=21)]
    before = dev.evaluate(three)
    ia, ib = np.arange(len(rows_a["value_p1"])), np.arange(len(rows_b["value_p1"]))
    got = [rs_a.validate(dev, ia, return_rows=True), rs_b.validate(dev, ib, return_rows=True)]
    after = dev.evaluate(three)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    got += [rs_a.validate(dev, ia, return_rows=True), rs_b.validate(dev, ib, return_rows=True)]
    for j, (rs, idx) in enumerate(((rs_a, ia), (rs_b, ib), (rs_a, ia), (rs_b, ib))):
        fresh = _net(blob)
        _same(got[j], rs.validate(fresh, idx, return_rows=True), f"call {j} against a fresh net")
        fresh.close()
    dev.close()


def test_cleared_and_refilled_set_binds_its_new_mazes(tmp_path):
    """the same pool, the same number of games, other mazes: the net's maze constants follow"""
    from alpharat_amd.shards import RowSet

    games, rows = V.board("15x11 maze")
    _, w, h, *_ = V.BOARDS["15x11 maze"]
    assert len(games) == 2 and games[0]["cost"].tobytes() != games[1]["cost"].tobytes()
    blob, _ = V.network("random_mlp_h64", w, h, tmp_path)
    dev = _net(blob)
    n = len(rows["value_p1"])
    with RowSet(w, h, n) as rs, RowSet(w, h, n) as other:
        rs.add_games(games)
        rs.validate(dev, np.arange(n))
        rs.clear()
        rs.add_games(games[::-1])
        other.add_games(games[::-1])
        fresh = _net(blob)
        _same(rs.validate(dev, np.arange(n), return_rows=True), other.validate(fresh, np.arange(n), return_rows=True), "refilled")
        fresh.close()
    dev.close()


def test_refusals(sets, mlp55, tmp_path):
    from alpharat_amd.validate import ValSums

    rs, _, rows = sets("5x5 open")
    n = len(rows["value_p1"])
    dev = _net(mlp55[0])
    base = rs.validate(dev, np.arange(n), return_rows=True)
    wrong = _net(V.network("random_mlp_h64", 7, 5, tmp_path)[0])
    with pytest.raises(RuntimeError, match="7x5 board"):
        rs.validate(wrong, np.arange(n))
    with pytest.raises(RuntimeError, match="position"):
        rs.validate(dev, np.array([0, n], np.uint64))
    _same(rs.validate(dev, np.arange(n), return_rows=True), base, "after refused calls")
    rs7, _, rows7 = sets("7x5")
    assert rs7.validate(wrong, np.arange(len(rows7["value_p1"]))).n == len(rows7["value_p1"])  # the refused net still works
    empty, out = rs.validate(dev, np.zeros(0, np.uint64), return_rows=True)
    assert empty == ValSums() and out["logits_p1"].shape == (0, 5)
    with pytest.raises(ValueError, match="no rows"):
        empty.metrics()
    wrong.close()
    dev.close()
