"""Validation of a local_value checkpoint with its ownership head on the device: ar_rows_validate_lv (k_mlp_mfma with
FEAT, k_own_mfma, k_own_sum), RowSet.validate_lv and alpharat_amd/validate.py OwnSums / local_value_metrics, against the float64
restatement of the head and its loss (tests/_ownership_np.py, tied to the reference by tests/golden/ownership).

The rows are the oracle games of tests/_rows.py BOARDS. Their recorded outcomes are lopsided (few SIMULTANEOUS, no P2_WIN
on some boards), so every board is also uploaded with doctored outcomes, drawn uniformly per game and cell:
ar_rows_add_games stores a record's outcomes as given. Shapes: 5x5 H = 32 (100 columns: a partial pass, a narrow hidden
layer), 7x7 H = 256 (the golden trunk, full width), 15x11 H = 64 (660 columns: a partial third pass, NW = 4), 16x16 H = 64
(1024 columns: four full passes, the first-layer variant for large boards), one position (a block with one row)."""
import numpy as np
import pytest
import torch  # before anything loads libalpharat_hip: a process brings up one HIP runtime, and torch ships its own

import _oracle as O
import _ownership_np as ON
import _rows_np as R
import _validate as V
from _random_nets import positions, pyrat, random_mlp

pytestmark = pytest.mark.gpu

SHAPES = {"5x5 open": 32, "7x7": 256, "15x11 maze": 64, "16x16": 64, "one position": 32}
IDS = [b.replace(" ", "_") for b in SHAPES]
VAL_KEYS = ("logits_p1", "logits_p2", "value_p1", "value_p2")
OWN_KEYS = ("own_ce", "own_cells", "own_value", "own_logits")


def tensors_of(board):
    """(all tensors, the trunk's and heads' alone) of the board's network: the golden mlp_7x7_h256 trunk on 7x7, else a
    seeded PyRatMLP; the ownership head is tests/_ownership_np.py random_ownership"""
    from alpharat_amd.weights import read_blob

    _, w, h, *_ = V.BOARDS[board]
    H = SHAPES[board]
    plain = read_blob(V.GOLD / "nets" / "mlp_7x7_h256.arnet")[3] if board == "7x7" else random_mlp(w, h, H, V.SEED)
    assert plain["trunk.0.weight"].shape[0] == H
    return {**plain, **ON.random_ownership(w, h, H, 17)}, plain


def doctored(games):
    """the games with outcomes drawn uniformly, the first seed under which every class holds at least 15 % of the rows'
    active cells (a single position has five of them)"""
    for seed in range(200):
        rng = np.random.default_rng(seed)
        out = [dict(g, cheese_outcomes=rng.integers(0, 4, g["width"] * g["height"]).astype(np.uint8).reshape(
            np.asarray(g["cheese_outcomes"]).shape)) for g in games]
        co = R.stack_rows(out)["cheese_outcomes"]
        share = np.array([(co == k).sum() for k in range(4)]) / max((co >= 0).sum(), 1)
        if share.min() >= 0.15:
            return out, share
    raise AssertionError("no seed gives every class 15 % of the active cells")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """board -> dict(sets: {"recorded", "doctored"} -> (RowSet, stack_rows), net, blob, plain_blob, tensors, want): `want`
    the float64 ownership logits (n, hw, 4) of every stored position"""
    from alpharat_amd.nets import Net
    from alpharat_amd.shards import RowSet
    from alpharat_amd.weights import write_blob

    tmp = tmp_path_factory.mktemp("lv")
    made = {}

    def get(board):
        if board not in made:
            games, rows = V.board(board)
            _, w, h, *_ = V.BOARDS[board]
            doc, share = doctored(games)
            assert share.min() >= 0.15, share
            sets = {}
            for name, gs in (("recorded", games), ("doctored", doc)):
                rs = RowSet(w, h, len(rows["value_p1"]))
                rs.add_games(gs)
                sets[name] = (rs, R.stack_rows(gs))
            t, plain = tensors_of(board)
            tag = board.replace(" ", "_")
            blob = write_blob(tmp / f"{tag}.lv.arnet", "mlp", w, h, t)
            plain_blob = write_blob(tmp / f"{tag}.arnet", "mlp", w, h, plain)
            made[board] = dict(sets=sets, net=Net(blob), blob=blob, plain_blob=plain_blob, tensors=t,
                               want=ON.forward(t, rows["observation"]), n=len(rows["value_p1"]), w=w, h=h)
        return made[board]

    yield get
    for m in made.values():
        m["net"].close()
        for rs, _ in m["sets"].values():
            rs.close()


def rel_close(got, want, rel, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    assert np.all(err <= rel * (1 + np.abs(want))), (what, float(err.max()))


def same(a, b, what=""):
    """two results of validate_lv with return_rows: the same bytes"""
    assert a[0] == b[0] and a[1] == b[1], (what, a[:2], b[:2])
    for k in VAL_KEYS + OWN_KEYS:
        assert a[2][k].tobytes() == b[2][k].tobytes(), (what, k)


@pytest.mark.parametrize("board", list(SHAPES), ids=IDS)
def test_logits_row_terms_sums_and_loss(board, world):
    m = world(board)
    n, hw = m["n"], m["w"] * m["h"]
    assert m["net"].has_ownership
    for which, (rs, rows) in m["sets"].items():
        what = f"{board} {which}"
        targets = rows["cheese_outcomes"].reshape(n, hw)
        sums, own, out = rs.validate_lv(m["net"], np.arange(n), return_rows=True)
        assert sums.n == n and own.n == n and own.batch_rows == 0 and own.batch_weighted == 0.0
        assert out["own_logits"].shape == (n, m["h"], m["w"], 4)
        got = out["own_logits"].reshape(n, hw, 4)
        # 1. the head's logits at the project's tolerance for network outputs
        np.testing.assert_allclose(got, m["want"], atol=1e-5, rtol=1e-5, err_msg=what)
        # 2. active cells exactly
        assert np.array_equal(out["own_cells"], (targets >= 0).sum(axis=1)), what
        assert own.cells == int((targets >= 0).sum())
        # 3. the row terms on their own: over the returned f32 logits (f32 expf / logf against float64)
        ce, cells, value = ON.row_terms(got, targets)
        rel_close(out["own_ce"], ce, 1e-6, what + " ce")
        rel_close(out["own_value"], value, 1e-6, what + " value")
        # 4. the reduction on its own: over the returned per-row terms
        rel_close(own.ce, out["own_ce"].sum(), 1e-9, what + " sum ce")
        # 5. end to end against the float64 forward. A cell's cross-entropy moves by at most 2 d_l with d_l = 1e-5 (1 + max|l|)
        # the logits' tolerance (|l_k - lse| is 1-Lipschitz in each of l and lse); the mean over active cells moves by the mean
        # of the cells' bounds. 1e-6 on top covers f32 expf / logf and the f32 terms.
        w_ce, w_cells, _ = ON.row_terms(m["want"], targets)
        exp = ON.loss_ownership(w_ce, w_cells)
        active = targets >= 0
        d_l = 1e-5 * (1 + np.abs(m["want"]).max(axis=-1))
        bound = (2 * d_l[active]).mean() + 1e-6
        got_loss = own.metrics()["loss_ownership"]
        print(f"{what} loss_ownership: got {got_loss:.9g} want {exp:.9g} diff {abs(got_loss - exp):.3g} bound {bound:.3g}")
        assert abs(got_loss - exp) <= bound, (what, got_loss, exp, bound)


def test_loss_batches(world):
    from alpharat_amd.validate import local_value_metrics

    m = world("5x5 open")
    rs, rows = m["sets"]["doctored"]
    idx = np.arange(130) % m["n"]  # 130 rows: two batches of 64 or 65, the last one short
    n = len(idx)
    base = rs.validate_lv(m["net"], idx, return_rows=True)
    for B in (1, 3, 64, 65, n):
        sums, own, out = rs.validate_lv(m["net"], idx, loss_batch_rows=B, return_rows=True)
        assert own.batch_rows == B and sums == base[0]
        assert out["own_ce"].tobytes() == base[2]["own_ce"].tobytes()
        want = ON.batch_weighted(out["own_ce"], out["own_cells"], B)
        rel_close(own.batch_weighted, want, 1e-9, f"batches of {B}")
        rel_close(own.metrics()["loss_ownership"], want / n, 1e-9)
        for chunk in (1, 64, 200):  # chunk_rows is rounded up to whole batches
            again = rs.validate_lv(m["net"], idx, chunk_rows=chunk, loss_batch_rows=B)[1]
            rel_close(again.batch_weighted, want, 1e-9, f"batches of {B}, chunk_rows={chunk}")
    rel_close(own.batch_weighted, own.ce / own.cells * n, 1e-12, "one batch over the request")
    got = local_value_metrics(sums, own, 1.0, 0.5, 0.25)
    assert got["loss"] == sums.metrics(1.0, 0.5)["loss"] + 0.25 * got["loss_ownership"]
    with pytest.raises(ValueError, match="do not add"):
        own + base[1]
    assert (base[1] + base[1]).cells == 2 * base[1].cells


def _golden_games(z):
    """one single-position game per stored observation: the position its planes and scalars encode, on the open maze"""
    w, h, mt = int(z["width"]), int(z["height"]), int(z["max_turns"])
    hw = w * h
    maze = O.Game(w, h, mt).maze()
    games = []
    for i, o in enumerate(z["observation"]):
        p1, p2 = int(o[hw * 4:hw * 5].argmax()), int(o[hw * 5:hw * 6].argmax())
        sc = o[hw * 7:]
        s1, s2 = np.float32(round(float(sc[4]) * 20) / 2), np.float32(round(float(sc[5]) * 20) / 2)
        mask = (o[hw * 6:hw * 7] > 0).astype(np.uint8)
        z5 = np.zeros((1, 5), np.float32)
        games.append(dict(
            width=w, height=h, n=1, max_turns=mt, game_index=i, result=0, maze=maze, initial_cheese=mask.reshape(h, w),
            final_p1_score=np.float32(s1 + z["value_p1"][i]), final_p2_score=np.float32(s2 + z["value_p2"][i]),
            cheese_outcomes=np.where(z["cheese_outcomes"][i] >= 0, z["cheese_outcomes"][i], 2).astype(np.uint8),
            p1_pos=np.array([[p1 % w, p1 // w]], np.int32), p2_pos=np.array([[p2 % w, p2 // w]], np.int32),
            p1_mud=np.array([round(float(sc[2]) * 10)], np.int32), p2_mud=np.array([round(float(sc[3]) * 10)], np.int32),
            turn=np.array([round(float(sc[1]) * mt)], np.int32), p1_score=np.array([s1]), p2_score=np.array([s2]),
            cheese_mask=mask[None], action_p1=np.zeros(1, np.int32), action_p2=np.zeros(1, np.int32),
            policy_p1=z["policy_p1"][i:i + 1], policy_p2=z["policy_p2"][i:i + 1], value_p1=np.zeros(1, np.float32),
            value_p2=np.zeros(1, np.float32), visit_counts_p1=z5, visit_counts_p2=z5, prior_p1=z5, prior_p2=z5))
    return games


@pytest.mark.parametrize("name", ["lv_5x5_h32", "lv_7x5_h64"])
def test_golden_checkpoint_against_the_reference(name, tmp_path):
    """the reference's own LocalValueMLP, rows and numbers (tools/gen_ownership_golden.py)"""
    from alpharat_amd.nets import Net
    from alpharat_amd.shards import RowSet
    from alpharat_amd.validate import local_value_metrics
    from alpharat_amd.weights import write_blob

    z = np.load(V.GOLD / "ownership" / f"{name}.npz")
    w, h, n, B = int(z["width"]), int(z["height"]), len(z["observation"]), int(z["batch_rows"])
    sd = {k[3:]: z[k] for k in z.files if k.startswith("sd/") and k != "sd/outcome_values"}
    net = Net(write_blob(tmp_path / f"{name}.lv.arnet", "mlp", w, h, sd))
    assert net.has_ownership
    games = _golden_games(z)
    assert np.array_equal(R.stack_rows(games)["observation"], z["observation"])  # the positions are the stored ones
    with RowSet(w, h, n) as rs:
        rs.add_games(games)
        sums, own, out = rs.validate_lv(net, np.arange(n), loss_batch_rows=B, return_rows=True)
    np.testing.assert_allclose(out["own_logits"], z["ownership_logits"], atol=1e-5, rtol=1e-5)
    np.testing.assert_allclose(out["own_value"], z["ownership_value"], atol=1e-4, rtol=1e-5)  # a sum over up to hw / 4 cells
    assert np.array_equal(out["own_cells"], (z["cheese_outcomes"].reshape(n, -1) >= 0).sum(axis=1))
    pw, vw, ow = (float(x) for x in z["weights"])
    got = local_value_metrics(sums, own, pw, vw, ow)
    lmax = np.abs(z["ownership_logits"]).max()
    bound_own = 2e-5 * (1 + lmax) + 1e-6
    print(f"{name}: loss_ownership got {got['loss_ownership']:.9g} want {float(z['loss_ownership']):.9g} bound {bound_own:.3g}")
    assert abs(got["loss_ownership"] - float(z["loss_ownership"])) <= bound_own
    # the other terms as test_gpu_validate.py bounds them: 2 d_l per policy, 2 |v - y| d_v + d_v^2 per value
    d_p = sum(2e-5 * (1 + np.abs(z[f"logits_p{p}"]).max()) for p in (1, 2))
    v_err = max(np.abs(z[f"pred_value_p{p}"] - z[f"value_p{p}"]).max() for p in (1, 2))
    d_v = 1e-5 * (1 + max(np.abs(z[f"pred_value_p{p}"]).max() for p in (1, 2)))
    bound = pw * (d_p + 2e-6) + vw * (2 * v_err * d_v + d_v ** 2 + 1e-6) + ow * bound_own
    print(f"{name}: loss got {got['loss']:.9g} want {float(z['loss']):.9g} bound {bound:.3g}")
    assert abs(got["loss"] - float(z["loss"])) <= bound
    with RowSet(w, h, n) as rs:
        rs.add_games(games)
        one = rs.validate_lv(net, np.arange(n))[1]  # a single batch over the request: the pooled mean
    assert abs(one.metrics()["loss_ownership"] - float(z["loss_ownership_one_batch"])) <= bound_own
    net.close()


@pytest.mark.parametrize("board", ["5x5 open", "16x16"], ids=["5x5_open", "16x16"])
def test_valsums_and_rows_are_validates(board, world):
    """sums and rows_out of validate_lv: the bytes of validate with the same net, and with the plain blob of the trunk"""
    from alpharat_amd.nets import Net

    m = world(board)
    rs, _ = m["sets"]["recorded"]
    idx = np.arange(m["n"])
    plain = Net(m["plain_blob"])
    assert not plain.has_ownership
    for chunk in (0, 50):
        lv = rs.validate_lv(m["net"], idx, chunk_rows=chunk, return_rows=True)
        for net in (m["net"], plain):
            sums, out = rs.validate(net, idx, chunk_rows=chunk, return_rows=True)
            assert sums == lv[0], (board, chunk)
            for k in VAL_KEYS:
                assert out[k].tobytes() == lv[2][k].tobytes(), (board, chunk, k)
    plain.close()


@pytest.mark.parametrize("board", ["5x5 open", "15x11 maze"], ids=["5x5_open", "15x11_maze"])
def test_chunking_and_reproducibility(board, world):
    m = world(board)
    rs, _ = m["sets"]["doctored"]
    idx = np.arange(m["n"])
    base = rs.validate_lv(m["net"], idx, chunk_rows=0, return_rows=True)
    same(rs.validate_lv(m["net"], idx, chunk_rows=0, return_rows=True), base, "the same call twice")
    assert rs.validate_lv(m["net"], idx)[1] == base[1]  # without the per-row outputs
    for chunk in (1, 64, 65):
        got = rs.validate_lv(m["net"], idx, chunk_rows=chunk, return_rows=True)
        for k in OWN_KEYS:  # a row's terms do not depend on its neighbours in the block
            assert got[2][k].tobytes() == base[2][k].tobytes(), (chunk, k)
        assert got[1].cells == base[1].cells
        rel_close(got[1].ce, base[1].ce, 1e-9, f"chunk_rows={chunk}")
        same(rs.validate_lv(m["net"], idx, chunk_rows=chunk, return_rows=True), got, f"chunk_rows={chunk} twice")


def test_row_selection(world):
    m = world("5x5 open")
    rs, rows = m["sets"]["doctored"]
    n = m["n"]
    whole = rs.validate_lv(m["net"], np.arange(n), return_rows=True)
    rng = np.random.default_rng(3)
    requests = dict(repeated=rng.integers(0, n, size=2 * n + 3), reversed=np.arange(n)[::-1].copy(),
                    sixty_five=rng.integers(0, n, size=65))
    for what, index in requests.items():
        sums, own, out = rs.validate_lv(m["net"], index, return_rows=True)
        assert sums.n == own.n == len(index)
        for k in OWN_KEYS:
            assert out[k].tobytes() == whole[2][k][index].tobytes(), (what, k)
        assert own.cells == int(whole[2]["own_cells"][index].sum())
        rel_close(own.ce, whole[2]["own_ce"][index].sum(), 1e-9, what)
    from alpharat_amd.dataset import RowDataset
    from alpharat_amd.validate import OwnSums, ValSums

    train, val = RowDataset(rs).split(0.25, 42)
    assert val.validate_lv(m["net"]) == rs.validate_lv(m["net"], val.positions)
    sums, own, out = rs.validate_lv(m["net"], np.zeros(0, np.uint64), loss_batch_rows=3, return_rows=True)
    assert sums == ValSums() and own == OwnSums(batch_rows=3) and out["own_logits"].shape == (0, 5, 5, 4)
    with pytest.raises(ValueError, match="no rows"):
        own.metrics()


def test_one_net_alternates(world):
    m = world("5x5 open")
    rs, _ = m["sets"]["doctored"]
    net, idx = m["net"], np.arange(m["n"])
    three = [pyrat(og) for og in positions(5, 5, 3, seed=21)]
    ev, va, lv = net.evaluate(three), rs.validate(net, idx, return_rows=True), rs.validate_lv(net, idx, return_rows=True)
    for _ in range(2):
        again = net.evaluate(three)
        for k in ev:
            assert ev[k].tobytes() == again[k].tobytes(), k
        same(rs.validate_lv(net, idx, return_rows=True), lv, "validate_lv after evaluate")
        sums, out = rs.validate(net, idx, return_rows=True)
        assert sums == va[0] and all(out[k].tobytes() == va[1][k].tobytes() for k in VAL_KEYS)


def test_refusals(world, tmp_path):
    from alpharat_amd.nets import Net
    from alpharat_amd.weights import write_blob

    m = world("5x5 open")
    rs, _ = m["sets"]["doctored"]
    n = m["n"]
    base = rs.validate_lv(m["net"], np.arange(n), return_rows=True)
    plain = Net(m["plain_blob"])
    with pytest.raises(RuntimeError, match="no ownership head"):
        rs.validate_lv(plain, np.arange(n))
    assert rs.validate(plain, np.arange(n)) == base[0]
    plain.close()
    # H = 40 runs on k_mlp: the blob loads, the head is not built
    t40 = {**random_mlp(5, 5, 40, V.SEED), **ON.random_ownership(5, 5, 40, 17)}
    n40 = Net(write_blob(tmp_path / "h40.lv.arnet", "mlp", 5, 5, t40))
    assert not n40.has_ownership
    with pytest.raises(RuntimeError, match="no ownership head"):
        rs.validate_lv(n40, np.arange(n))
    assert rs.validate(n40, np.arange(n)).n == n
    n40.close()
    # three of the four tensors, a wrong shape: refused at load
    t = dict(m["tensors"])
    del t["ownership_head.2.bias"]
    with pytest.raises(RuntimeError, match=r"ownership_head\.2\.bias must be \[100\]"):
        Net(write_blob(tmp_path / "three.arnet", "mlp", 5, 5, t))
    t = dict(m["tensors"], **{"ownership_head.2.weight": m["tensors"]["ownership_head.2.weight"][:96]})
    with pytest.raises(RuntimeError, match=r"ownership_head\.2\.weight must be \[100, 32\]"):
        Net(write_blob(tmp_path / "shape.arnet", "mlp", 5, 5, t))
    with pytest.raises(RuntimeError, match="position"):
        rs.validate_lv(m["net"], np.array([0, n], np.uint64))
    other = world("7x7")
    with pytest.raises(RuntimeError, match="7x7 board"):
        rs.validate_lv(other["net"], np.arange(n))
    same(rs.validate_lv(m["net"], np.arange(n), return_rows=True), base, "after refused calls")
