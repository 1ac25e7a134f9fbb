"""Training rows on the device: ar_rows_add_games / ar_rows_attach / ar_rows_build (k_rows_append, k_rows_build) and
alpharat_amd/shards.py against the NumPy restatement of the reference's sharding step (tests/_rows_np.py). Rows are copies,
casts and exactly rounded f32 operations: every comparison is equality of bytes."""
from pathlib import Path

import numpy as np
import pytest

import _rows as T
import _rows_np as R

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).parent / "golden" / "nets"
SEED = 42

# SmartUniform runs, at most 100 simulations and 64 games, more games than resident slots
BOARDS = [
    ("5x5 open", dict(width=5, height=5, cheese_count=5, max_turns=30, num_games=24, simulations=40, concurrent_games=8)),
    ("7x5", dict(width=7, height=5, cheese_count=7, max_turns=30, num_games=12, simulations=40, concurrent_games=8)),
    ("7x7", dict(width=7, height=7, cheese_count=9, max_turns=40, num_games=16, simulations=40, concurrent_games=8)),
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
        stats = s.run_to_end()
        assert s.finished and stats.total_games == kw["num_games"]
    sink.sort(key=lambda g: g["game_index"])
    assert rs.count() == (len(sink), sum(g["n"] for g in sink))
    return sink, rs


def _sorted_rows(rs):
    """stored rows of every position, games in increasing game index"""
    gi, fr, nr = rs.games()
    order = np.argsort(gi, kind="stable")
    return np.concatenate([fr[g] + np.arange(nr[g], dtype=np.uint64) for g in order])


@pytest.fixture(scope="module", params=BOARDS, ids=lambda b: b[0])
def run(request):
    from alpharat_amd.shards import RowSet

    name, kw = request.param
    sink, attached = _attached_run(kw)
    uploaded = RowSet(kw["width"], kw["height"], sum(g["n"] for g in sink))
    uploaded.add_games(sink)
    yield name, kw, sink, attached, uploaded, R.stack_rows(sink)
    attached.close()
    uploaded.close()


def test_uploaded_records_build_the_restatements_rows(run):
    name, kw, sink, _, rs, want = run
    n = len(want["value_p1"])
    assert rs.count() == (len(sink), n)
    gi, fr, nr = rs.games()
    assert list(gi) == [g["game_index"] for g in sink] and list(nr) == [g["n"] for g in sink]
    assert list(fr) == list(np.cumsum([0] + [g["n"] for g in sink])[:-1])
    rng = np.random.default_rng(9)
    orders = dict(identity=np.arange(n), reversed=np.arange(n)[::-1], permutation=rng.permutation(n),
                  repeated=rng.integers(0, n, size=259), one=np.array([n - 1]), five=rng.integers(0, n, size=5))
    for what, rows in orders.items():
        T.assert_rows_equal(rs.build(rows), R.take(want, rows), f"{name} {what}")
    empty = rs.build(np.zeros(0, np.uint64))
    assert all(len(empty[k]) == 0 for k in R.KEYS) and empty["cheese_outcomes"].shape == (0, kw["height"], kw["width"])
    if name == "15x11 maze":
        assert any((g["maze"] >= 2).any() for g in sink) and any((g["maze"] == -1).any() for g in sink)
        assert any((g["p1_mud"] > 0).any() or (g["p2_mud"] > 0).any() for g in sink)
    if name == "5x5 open":
        assert len({g["n"] for g in sink}) > 1


def test_attached_run_equals_its_sink_records(run):
    """The attached set got its games on the device, in the order they finished, with cheese outcomes computed there; the
    uploaded set got the same run's sink records. Listed by game index, they give the same bytes."""
    name, kw, sink, attached, uploaded, want = run
    assert kw["num_games"] > kw["concurrent_games"]
    gi, _, nr = attached.games()
    assert sorted(gi) == [g["game_index"] for g in sink]
    a = attached.build(_sorted_rows(attached))
    T.assert_rows_equal(a, uploaded.build(_sorted_rows(uploaded)), f"{name} attached against uploaded")
    T.assert_rows_equal(a, want, f"{name} attached against the restatement")
    assert attached.build_kernel_ms() > 0.0


def test_more_rows_than_one_launch_takes():
    """262 144 rows go into one launch: a request beyond that is cut, into the same output arrays."""
    from alpharat_amd.shards import RowSet

    sink, rs = _attached_run(dict(BOARDS[5][1]))
    try:
        want = R.stack_rows(sink)
        n = len(want["value_p1"])
        rows = (np.arange(262144 + 259, dtype=np.uint64) * 7) % n
        got = rs.build(rows)
        T.assert_rows_equal(got, R.take(want, rows), "over the launch cut")
    finally:
        rs.close()


def test_resident_count_does_not_change_the_training_set(tmp_path):
    from alpharat_amd import shards

    out = []
    for conc in (4, 16):
        kw = dict(BOARDS[0][1], concurrent_games=conc)
        sink, rs = _attached_run(kw)
        try:
            res = shards.prepare_training_set_with_split(None, tmp_path / str(conc), val_ratio=0.25, positions_per_shard=64,
                                                         seed=SEED, rowset=rs)
        finally:
            rs.close()
        d = Path(res.shard_dir)
        out.append({s: [dict(np.load(f)) for f in sorted((d / s).glob("shard_*.npz"))] for s in ("train", "val")})
        assert res.total_positions == sum(g["n"] for g in sink)
    for s in ("train", "val"):
        assert len(out[0][s]) == len(out[1][s]) > 0
        for x, y in zip(out[0][s], out[1][s]):
            T.assert_rows_equal(x, y, s)


def test_network_run_end_to_end_equals_the_restatements_shards(tmp_path):
    from alpharat_amd import shards

    kw = dict(width=7, height=7, cheese_count=9, max_turns=40, num_games=12, simulations=32, concurrent_games=8,
              weights_path=str(GOLD / "mlp_7x7_h256.arnet"))
    sink, rs = _attached_run(kw, seed=0)
    try:
        res = shards.prepare_training_set_with_split(None, tmp_path, val_ratio=0.25, positions_per_shard=50, seed=SEED, rowset=rs)
    finally:
        rs.close()
    assert len(np.unique(np.concatenate([g["policy_p1"] for g in sink]))) > 20  # a network's policies, not a handful of values
    want = R.training_set(sink, 0.25, 50, SEED)
    d = Path(res.shard_dir)
    for s in ("train", "val"):
        files = sorted((d / s).glob("shard_*.npz"))
        assert [f.name for f in files] == [f"shard_{i:04d}.npz" for i in range(len(want[s]))]
        for f, x in zip(files, want[s]):
            T.assert_rows_equal(dict(np.load(f)), x, f"{s}/{f.name}")
    assert res.train_positions == sum(len(x["value_p1"]) for x in want["train"])
    assert res.val_positions == sum(len(x["value_p1"]) for x in want["val"]) > 0


def test_uploaded_games_through_the_writer(tmp_path):
    """Record dicts in, no row set given: the writer opens one of their size, uploads them in the order given and closes it."""
    from alpharat_amd import shards

    games = T.board_games("7x5", 7, 5, 30, 7, None, 5, 24)
    res = shards.prepare_training_set_with_split(games, tmp_path, val_ratio=0.2, positions_per_shard=30, seed=SEED)
    want = R.training_set(games, 0.2, 30, SEED)
    d = Path(res.shard_dir)
    for s in ("train", "val"):
        for i, x in enumerate(want[s]):
            T.assert_rows_equal(dict(np.load(d / s / f"shard_{i:04d}.npz")), x, f"{s} {i}")


def test_refusals():
    from alpharat_amd.sampling import SelfPlaySession
    from alpharat_amd.shards import RowSet

    games = T.board_games("5x5 open", 5, 5, 30, 5, None, 3, 24)
    other = T.board_games("7x5", 7, 5, 10, 5, None, 1, 16)
    n = sum(g["n"] for g in games)
    with RowSet(5, 5, n) as rs:
        rs.add_games(games[:2])
        before = rs.count()
        with pytest.raises(ValueError, match="7x5"):           # wrong board size
            rs.add_games(other)
        with pytest.raises(ValueError, match="position"):      # row index out of range
            rs.build(np.array([0, before[1]], np.uint64))
        with pytest.raises(MemoryError, match="full"):         # beyond capacity: nothing changes
            rs.add_games(games)
        assert rs.count() == before
        rs.add_games(games[2:])                                # exactly full
        assert rs.count() == (3, n)
        T.assert_rows_equal(rs.build(np.arange(n)), R.stack_rows(games), "after the refusals")
        rs.clear()
        assert rs.count() == (0, 0)
    kw = dict(width=5, height=5, cheese_count=5, max_turns=30, num_games=4, simulations=16, batch_size=8, seed=0,
              concurrent_games=2, output_dir=None)
    with RowSet(7, 5, 100) as wrong, RowSet(5, 5, 120) as a, RowSet(5, 5, 120) as b:
        with SelfPlaySession(**kw) as s:
            with pytest.raises(ValueError, match="7x5"):       # wrong board size
                s.attach_rows(wrong)
            s.attach_rows(a)
            with pytest.raises(ValueError, match="already"):   # a second attach
                s.attach_rows(b)
            with pytest.raises(RuntimeError, match="session"):
                a.close()                                      # (the session may still append to it)
            s.run_to_end()
        assert a.count()[0] == 4
        first = a.build(np.arange(a.count()[1]))
        a.clear()
        with SelfPlaySession(**kw) as s:                       # a closed session has let go of the set: the next run takes it
            s.attach_rows(a)
            s.run_to_end()
        assert a.count()[0] == 4
        again = a.build(np.arange(a.count()[1]))  # the same seeded games, whatever order they finished in
        assert sorted(r.tobytes() for r in again["observation"]) == sorted(r.tobytes() for r in first["observation"])
        with SelfPlaySession(**kw) as s:
            s.step(1)
            with pytest.raises(ValueError, match="first step"):  # attach after a step
                s.attach_rows(b)
        assert b.count() == (0, 0)
