"""Training batches on the device: ar_rows_order_set / ar_rows_build_device (k_rows_batch), RowSet.set_order / build_into
and alpharat_amd/dataset.py RowDataset, against the NumPy restatements of the reference's rows (tests/_rows_np.py) and of its
player-swap augmentation (tests/_augment_np.py, tied to the reference by tests/golden/augment). Every comparison is equality
of bytes -- a swapped score difference of 0 is -0.0 -- and every output tensor has rows of 0x5A in front of and behind the
rows asked for, which must stay."""
from pathlib import Path

import numpy as np
import pytest
import torch  # before anything loads libalpharat_hip: a process brings up one HIP runtime, and torch ships its own

import _augment_np as A
import _rows as T
import _rows_np as R

pytestmark = pytest.mark.gpu

SEED = 42
GUARD = 3

# SmartUniform runs, at most 40 simulations and 24 games, more games than resident slots
BOARDS = [
    ("5x5", dict(width=5, height=5, cheese_count=5, max_turns=30, num_games=24, simulations=40, concurrent_games=8)),
    ("7x5", dict(width=7, height=5, cheese_count=7, max_turns=30, num_games=12, simulations=40, concurrent_games=8)),
    ("9x8", dict(width=9, height=8, cheese_count=12, max_turns=30, num_games=6, simulations=24, concurrent_games=4)),
    ("15x11 maze", dict(width=15, height=11, cheese_count=21, max_turns=40, num_games=6, simulations=24, concurrent_games=4,
                        maze_type="random", wall_density=0.5, mud_density=0.5)),
    ("16x16", dict(width=16, height=16, cheese_count=30, max_turns=16, num_games=4, simulations=16, concurrent_games=2)),
    ("one position", dict(width=5, height=5, cheese_count=5, max_turns=1, num_games=5, simulations=16, concurrent_games=2)),
]


def _attached_run(kw, seed=3):
    """(the sink's records sorted by game index, the attached row set) of one run; the session is closed."""
    from alpharat_amd.sampling import SelfPlaySession
    from alpharat_amd.shards import RowSet

    sink = []
    rs = RowSet(kw["width"], kw["height"], kw["num_games"] * kw["max_turns"])
    with SelfPlaySession(output_dir=None, batch_size=8, seed=seed, on_game=sink.append, **kw) as s:
        s.attach_rows(rs)
        s.run_to_end()
    sink.sort(key=lambda g: g["game_index"])
    assert rs.count() == (len(sink), sum(g["n"] for g in sink))
    return sink, rs


def _listed(rs) -> np.ndarray:
    """the stored position of every position, games in increasing game index (the order of the restatement's rows)"""
    gi, fr, nr = rs.games()
    return np.concatenate([fr[g] + np.arange(nr[g], dtype=np.uint64) for g in np.argsort(gi, kind="stable")])


def _guarded(rs, n):
    """output tensors of n + 2 * GUARD rows, every byte 0x5A, and the views build_into gets"""
    from alpharat_amd.shards import KEYS, row_shapes

    shapes = row_shapes(rs.width, rs.height)
    whole = {}
    for k in KEYS:
        dt = torch.int8 if k in ("action_p1", "action_p2", "cheese_outcomes") else torch.float32
        t = torch.empty((n + 2 * GUARD,) + shapes[k], dtype=dt, device="cuda")
        t.view(torch.uint8).fill_(0x5A)
        whole[k] = t
    return whole, {k: whole[k][GUARD:] for k in KEYS}


def _fetch(whole, n, what=""):
    """the n rows between the guards as NumPy arrays (a copy on the current stream), the guards checked"""
    got = {}
    for k in R.KEYS:
        a = whole[k].cpu().numpy()
        for part in (a[:GUARD], a[GUARD + n:]):
            assert (part.view(np.uint8) == 0x5A).all(), f"{what}: {k} written outside its {n} rows"
        got[k] = a[GUARD:GUARD + n]
    return got


def _build(rs, first, n, what="", stream=None):
    whole, out = _guarded(rs, n)
    if stream is not None:
        torch.cuda.synchronize()  # the fill ran on the current stream
    rs.build_into(first, n, out, stream=stream)
    if stream is not None:
        stream.synchronize()
    return _fetch(whole, n, what)


@pytest.fixture(scope="module", params=BOARDS, ids=lambda b: b[0])
def run(request):
    from alpharat_amd.shards import RowSet

    name, kw = request.param
    sink, attached = _attached_run(kw)
    uploaded = RowSet(kw["width"], kw["height"], sum(g["n"] for g in sink))
    uploaded.add_games(sink)
    yield name, kw, sink, dict(uploaded=uploaded, attached=attached), R.stack_rows(sink)
    attached.close()
    uploaded.close()


@pytest.mark.parametrize("kind", ["uploaded", "attached"])
def test_build_into_equals_the_swapped_restatement(run, kind):
    name, kw, sink, sets, plain = run
    rs, w, h = sets[kind], kw["width"], kw["height"]
    stored = _listed(rs)
    n_pos = len(stored)
    assert n_pos == len(plain["value_p1"]) > 0
    rng = np.random.default_rng(9)
    masks = dict(all=np.ones(n_pos, bool), none=np.zeros(n_pos, bool), random=rng.random(n_pos) < 0.5)
    orders = dict(identity=np.arange(n_pos), permutation=rng.permutation(n_pos), repeated=rng.integers(0, n_pos, size=300))
    for mname, mask in masks.items():
        want_all = A.swap_rows(plain, mask, w, h)
        for oname, rows in orders.items():
            what = f"{name} {kind} mask={mname} order={oname}"
            rs.set_order(stored[rows], mask[rows] if mname != "none" else None)  # (no mask: swap = NULL)
            windows = [(0, len(rows))]
            if oname == "repeated":  # one row, five, more than a block's worth of launches' tail; first and n no multiples of 4
                windows += [(0, 1), (299, 1), (7, 5), (37, 259), (3, 13)]
            for first, n in windows:
                got = _build(rs, first, n, what)
                T.assert_rows_equal(got, R.take(want_all, rows[first:first + n]), f"{what} rows {first}+{n}")
    if n_pos > 1:  # the swap is not a no-op on these games
        assert A.swap_rows(plain, masks["all"], w, h)["observation"].tobytes() != plain["observation"].tobytes()
    if name == "5x5":  # equal scores at the first position: -0.0 in the swapped row
        rs.set_order(stored[:1], np.ones(1, np.uint8))
        assert _build(rs, 0, 1)["observation"][0, w * h * 7].view(np.uint32) == 0x80000000
    if name == "15x11 maze":
        assert any((np.asarray(g["p1_mud"]) != np.asarray(g["p2_mud"])).any() for g in sink)
    if name == "9x8":
        assert any(np.asarray(g["cheese_mask"]).reshape(g["n"], -1)[:, 64:].any() for g in sink)


def test_empty_window_and_empty_order(run):
    name, kw, sink, sets, plain = run
    rs = sets["uploaded"]
    rs.set_order(_listed(rs)[:4] if len(plain["value_p1"]) >= 4 else _listed(rs)[:1])
    whole, out = _guarded(rs, 0)
    rs.build_into(1, 0, out)
    _fetch(whole, 0, "n = 0")
    rs.set_order(np.zeros(0, np.uint64))
    rs.build_into(0, 0, out)
    with pytest.raises(ValueError, match="beyond the order"):
        rs.build_into(0, 1, _guarded(rs, 1)[1])


def test_on_another_stream(run):
    name, kw, sink, sets, plain = run
    rs, w, h = sets["attached"], kw["width"], kw["height"]
    stored = _listed(rs)
    n_pos = len(stored)
    rng = np.random.default_rng(4)
    rows, mask = rng.integers(0, n_pos, size=131), rng.random(n_pos) < 0.5
    rs.set_order(stored[rows], mask[rows])
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != torch.cuda.current_stream().cuda_stream
    got = _build(rs, 2, 127, f"{name} on a stream", stream=stream)
    T.assert_rows_equal(got, R.take(A.swap_rows(plain, mask, w, h), rows[2:129]), f"{name} on a stream")
    # the next order waits for that stream before it replaces the one the kernel read
    rs.set_order(stored[:1])


def test_more_rows_than_one_launch_takes():
    """262 144 rows go into one launch: a request beyond that is cut, into the same tensors."""
    sink, rs = _attached_run(dict(BOARDS[5][1]))
    try:
        plain = R.stack_rows(sink)
        n_pos = len(plain["value_p1"])
        stored = _listed(rs)
        total = 262144 + 259
        rows = (np.arange(total) * 7) % n_pos
        swap = (np.arange(total) % 3 == 1)
        rs.set_order(stored[rows], swap)
        got = _build(rs, 0, total, "over the launch cut")
        both = {k: np.concatenate([plain[k], A.swap_rows(plain, np.ones(n_pos, bool), 5, 5)[k]]) for k in R.KEYS}
        T.assert_rows_equal(got, R.take(both, rows + n_pos * swap), "over the launch cut")
    finally:
        rs.close()


# ---- RowDataset ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def five():
    from alpharat_amd.shards import RowSet

    kw = dict(BOARDS[0][1])
    sink, attached = _attached_run(kw)
    uploaded = RowSet(5, 5, sum(g["n"] for g in sink))
    uploaded.add_games(sink)
    yield sink, dict(uploaded=uploaded, attached=attached), R.stack_rows(sink)
    attached.close()
    uploaded.close()


def _as_rows(batches):
    """the batches of an epoch behind each other, as NumPy arrays in the shapes of the restatement"""
    if not batches:
        return None
    cat = {k: np.concatenate([b[k].cpu().numpy() for b in batches]) for k in R.KEYS}
    for k in ("value_p1", "value_p2", "action_p1", "action_p2"):
        cat[k] = cat[k].reshape(-1)
    return cat


@pytest.mark.parametrize("kind", ["uploaded", "attached"])
def test_epoch_iter_equals_the_restatement(five, kind):
    from alpharat_amd.dataset import RowDataset, epoch_plan

    sink, sets, plain = five
    ds = RowDataset(sets[kind])
    n = len(ds)
    assert n == len(plain["value_p1"]) and (ds.width, ds.height) == (5, 5)
    bs = 64 if n % 64 else 60  # an epoch with a remainder
    assert n % bs and n > 3 * bs
    epochs = []
    for epoch in (0, 1):
        batches = list(ds.epoch_iter(bs, epoch=epoch, seed=SEED))
        assert len(batches) == n // bs
        for b in batches:
            assert set(b) == set(R.KEYS) and all(t.device.type == "cuda" and t.is_contiguous() for t in b.values())
            assert b["observation"].shape == (bs, 5 * 5 * 7 + 6) and b["observation"].dtype == torch.float32
            assert b["policy_p1"].shape == b["policy_p2"].shape == (bs, 5) and b["policy_p2"].dtype == torch.float32
            assert b["value_p1"].shape == b["value_p2"].shape == (bs, 1) and b["value_p1"].dtype == torch.float32
            assert b["action_p1"].shape == b["action_p2"].shape == (bs, 1) and b["action_p1"].dtype == torch.int8
            assert b["cheese_outcomes"].shape == (bs, 5, 5) and b["cheese_outcomes"].dtype == torch.int8
        assert len({b["observation"].data_ptr() for b in batches}) == len(batches)  # each batch owns its tensors
        order, mask = epoch_plan(n, SEED, epoch)
        assert mask.any() and not mask.all()
        want = R.take(A.swap_rows(plain, mask, 5, 5), order[: n // bs * bs])
        got = _as_rows(batches)
        T.assert_rows_equal(got, want, f"epoch {epoch}")
        epochs.append(got)
    assert epochs[0]["observation"].tobytes() != epochs[1]["observation"].tobytes()
    T.assert_rows_equal(_as_rows(list(ds.epoch_iter(bs, epoch=0, seed=SEED))), epochs[0], "the same seed and epoch again")
    # the remainder
    tail = list(ds.epoch_iter(bs, epoch=0, seed=SEED, drop_last=False))
    assert len(tail) == n // bs + 1 and tail[-1]["value_p1"].shape == (n % bs, 1)
    order, mask = epoch_plan(n, SEED, 0)
    T.assert_rows_equal(_as_rows(tail), R.take(A.swap_rows(plain, mask, 5, 5), order), "drop_last=False")
    # the switches
    T.assert_rows_equal(_as_rows(list(ds.epoch_iter(n, augment=False, shuffle=False))), plain, "no shuffle, no swap")
    T.assert_rows_equal(_as_rows(list(ds.epoch_iter(n, p_swap=1.0, shuffle=False))),
                        A.swap_rows(plain, np.ones(n, bool), 5, 5), "no shuffle, every row swapped")


def test_two_epochs_over_one_set_do_not_interleave(five):
    from alpharat_amd.dataset import RowDataset

    train, val = RowDataset(five[1]["uploaded"]).split(0.25, SEED)
    it = train.epoch_iter(16)
    next(it)
    next(val.epoch_iter(16))
    with pytest.raises(RuntimeError, match="another epoch"):
        next(it)


def _row_bytes(rows):
    n = len(rows["value_p1"])
    return sorted(b"".join(np.ascontiguousarray(rows[k][i]).tobytes() for k in R.KEYS) for i in range(n))


@pytest.mark.parametrize("kind", ["uploaded", "attached"])
def test_split_holds_the_rows_of_the_written_shards(five, kind, tmp_path):
    from alpharat_amd import shards
    from alpharat_amd.dataset import RowDataset

    sink, sets, plain = five
    rs = sets[kind]
    res = shards.prepare_training_set_with_split(None, tmp_path, val_ratio=0.25, positions_per_shard=64, seed=SEED, rowset=rs)
    train, val = RowDataset(rs).split(0.25, SEED)
    assert len(train) == res.train_positions and len(val) == res.val_positions > 0
    for name, ds in (("train", train), ("val", val)):
        files = sorted((Path(res.shard_dir) / name).glob("shard_*.npz"))
        written = {k: np.concatenate([np.load(f)[k] for f in files]) for k in R.KEYS}
        got = _as_rows(list(ds.epoch_iter(50, seed=SEED, augment=False, drop_last=False)))
        assert _row_bytes(got) == _row_bytes(written), name


def test_refusals(five):
    from alpharat_amd.shards import RowSet

    sink, _, plain = five
    n_pos = len(plain["value_p1"])
    with RowSet(5, 5, n_pos) as rs:
        rs.add_games(sink)
        whole, out = _guarded(rs, 4)
        with pytest.raises(ValueError, match="no order"):            # build_into before set_order
            rs.build_into(0, 4, out)
        rs.set_order(np.arange(10), np.arange(10) % 2)
        want = R.take(A.swap_rows(plain, np.arange(n_pos) % 2 == 1, 5, 5), np.arange(10))
        with pytest.raises(ValueError, match="beyond the order"):    # a window past the order
            rs.build_into(8, 4, out)
        with pytest.raises(ValueError, match="beyond the order"):
            rs.build_into(11, 0, out)
        with pytest.raises(ValueError, match="position"):            # an index beyond the set: the old order stays
            rs.set_order(np.array([0, n_pos], np.uint64))
        with pytest.raises(ValueError, match="swap has shape"):
            rs.set_order(np.arange(4), np.zeros(3, np.uint8))
        _fetch(whole, 0, "refused calls")                            # nothing was written: all 4 + 2 * GUARD rows are 0x5A
        T.assert_rows_equal(_build(rs, 6, 4), {k: want[k][6:10] for k in R.KEYS}, "the old order after a refused one")
        rs.clear()
        with pytest.raises(ValueError, match="no order"):            # clear() dropped the order
            rs.build_into(0, 1, out)
        rs.add_games(sink[:1])
        with pytest.raises(ValueError, match="no order"):
            rs.build_into(0, 1, out)
        _fetch(whole, 0, "refused calls")
