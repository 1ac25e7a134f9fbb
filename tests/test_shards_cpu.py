"""The shard writer without a device: alpharat_amd/shards.py with the NumPy restatement (tests/_rows_np.py) injected as the
row builder. File layout, split, shuffle, manifest and bundle reading are checked against the restatement of
alpharat/data/sharding.py, array by array and byte by byte."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

import _bundles as B
import _rows as T
import _rows_np as R
from alpharat_amd import _lib, shards

SEED = 42  # scripts/iterate.py:198


@pytest.fixture(scope="module")
def games():
    gs = T.board_games("5x5 open", 5, 5, 30, 5, None, 7, 24)
    assert len({g["n"] for g in gs}) > 1
    return gs


def _load(d: Path) -> list:
    files = sorted(p.name for p in d.glob("shard_*.npz"))
    assert files == [f"shard_{i:04d}.npz" for i in range(len(files))], files
    out = []
    for f in files:
        with np.load(d / f) as z:
            assert sorted(z.files) == sorted(R.KEYS)
            out.append({k: z[k] for k in R.KEYS})
    return out


def _assert_split(d: Path, want: list, pps: int, w: int, h: int, set_id: str, batches=()):
    got = _load(d)
    assert len(got) == len(want)
    for i, (g, x) in enumerate(zip(got, want)):
        n = len(x["value_p1"])
        assert n == pps or (i == len(want) - 1 and 0 < n <= pps)
        assert g["observation"].shape == (n, w * h * 7 + 6) and g["policy_p1"].shape == (n, 5) and g["policy_p2"].shape == (n, 5)
        assert g["value_p1"].shape == (n,) and g["action_p2"].shape == (n,) and g["cheese_outcomes"].shape == (n, h, w)
        for k in R.KEYS:
            assert g[k].dtype == R.DTYPES[k], k
        T.assert_rows_equal(g, x, f"{d.name} shard {i}")
    m = json.loads((d / "manifest.json").read_text())
    assert sorted(m) == sorted(["training_set_id", "created_at", "builder_version", "source_batches", "total_positions",
                                "shard_count", "positions_per_shard", "width", "height"])
    assert m["training_set_id"] == set_id and m["builder_version"] == "flat_v2" and m["source_batches"] == list(batches)
    assert m["total_positions"] == sum(len(x["value_p1"]) for x in want) and m["shard_count"] == len(want)
    assert (m["positions_per_shard"], m["width"], m["height"]) == (pps, w, h)
    assert isinstance(m["created_at"], str) and m["created_at"][:2] == "20"


def _shard_sizes(n_train):
    """not a multiple of the total, exactly a multiple (several shards), exactly one shard, smaller than one shard"""
    div = next((d for d in range(2, n_train) if n_train % d == 0), 1)
    odd = next(p for p in (7, 11, 13) if n_train % p)
    return [odd, div, n_train, n_train + 5]


def test_files_split_and_manifest_equal_the_restatement(games, tmp_path):
    lengths = [g["n"] for g in games]
    train, val, *_ = R.split_and_shuffle(lengths, 0.3, SEED)
    assert len(val) == 2 and len(train) == 5
    n_train = sum(lengths[g] for g in train)
    for pps in _shard_sizes(n_train):
        asked = []
        inner = R.builder(games)

        def build(index):
            asked.append(np.asarray(index).copy())
            return inner(index)

        res = shards.prepare_training_set_with_split(games, tmp_path / f"pps{pps}", val_ratio=0.3, positions_per_shard=pps,
                                                     seed=SEED, row_builder=build)
        want = R.training_set(games, 0.3, pps, SEED)
        d = Path(res.shard_dir)
        assert d.parent == tmp_path / f"pps{pps}" and d.name == res.shard_id
        assert sorted(p.name for p in d.iterdir()) == ["train", "val"]
        _assert_split(d / "train", want["train"], pps, 5, 5, f"{res.shard_id}_train")
        _assert_split(d / "val", want["val"], pps, 5, 5, f"{res.shard_id}_val")
        assert res.train_positions == n_train and res.val_positions == sum(lengths[g] for g in val)
        assert res.total_positions == sum(lengths)
        if pps == n_train:
            assert len(want["train"]) == 1
        if pps == n_train + 5:
            assert len(want["train"]) == 1 and len(want["train"][0]["value_p1"]) < pps
        # no game has positions on both sides: the positions asked for, mapped back to their games
        game_of = np.repeat(np.arange(len(games)), lengths)
        k = len(want["train"])
        in_train = set(game_of[np.concatenate(asked[:k])])
        in_val = set(game_of[np.concatenate(asked[k:])])
        assert in_train == set(train) and in_val == set(val) and not (in_train & in_val)
        assert sorted(np.concatenate(asked)) == list(range(sum(lengths)))  # every position once


def test_no_validation_games_writes_no_val_directory(games, tmp_path):
    res = shards.prepare_training_set_with_split(games, tmp_path, val_ratio=0.0, positions_per_shard=50, seed=SEED,
                                                 row_builder=R.builder(games))
    d = Path(res.shard_dir)
    assert sorted(p.name for p in d.iterdir()) == ["train"] and res.val_positions == 0
    _assert_split(d / "train", R.training_set(games, 0.0, 50, SEED)["train"], 50, 5, 5, f"{res.shard_id}_train")
    # a ratio too small for one validation game does the same
    res = shards.prepare_training_set_with_split(games, tmp_path, val_ratio=0.1, positions_per_shard=50, seed=SEED,
                                                 row_builder=R.builder(games))
    assert sorted(p.name for p in Path(res.shard_dir).iterdir()) == ["train"]


def test_refusals(games, tmp_path):
    b = R.builder(games)
    # a ratio that would leave no training game: only val_ratio >= 1 can (int(total * val_ratio) < total below 1), and
    # the range check refuses it; the reference's later "No games left for training" branch is unreachable
    with pytest.raises(ValueError, match="val_ratio"):
        shards.prepare_training_set_with_split(games, tmp_path, val_ratio=1.0, seed=SEED, row_builder=b)
    with pytest.raises(ValueError, match="val_ratio"):
        shards.prepare_training_set_with_split(games, tmp_path, val_ratio=-0.1, seed=SEED, row_builder=b)
    with pytest.raises(ValueError, match="empty"):
        shards.prepare_training_set_with_split([], tmp_path, seed=SEED, row_builder=b)
    with pytest.raises(ValueError, match="No games"):
        (tmp_path / "nothing").mkdir()
        shards.prepare_training_set_with_split([tmp_path / "nothing"], tmp_path, seed=SEED, row_builder=b)
    res = shards.prepare_training_set_with_split(games[:1], tmp_path / "one", val_ratio=0.99, seed=SEED, row_builder=b)
    assert res.val_positions == 0 and res.train_positions == games[0]["n"]  # one game, any ratio below 1: it trains
    import shutil

    shutil.rmtree(tmp_path / "one")
    np.savez(tmp_path / "nothing" / "single_game.npz", maze=np.zeros((5, 5, 4), np.int8))
    with pytest.raises(ValueError, match="not a bundle"):
        shards.prepare_training_set_with_split([tmp_path / "nothing"], tmp_path, seed=SEED, row_builder=b)
    other = T.board_games("7x5", 7, 5, 10, 5, None, 1, 16)
    with pytest.raises(ValueError, match="Dimension mismatch"):
        shards.prepare_training_set_with_split(games + other, tmp_path, seed=SEED, row_builder=b)
    assert not [p for p in tmp_path.iterdir() if p.name != "nothing"]  # a refused call leaves nothing behind


def test_same_seed_same_files_other_seed_other_order(games, tmp_path):
    def run(seed, sub):
        res = shards.prepare_training_set_with_split(games, tmp_path / sub, val_ratio=0.3, positions_per_shard=40, seed=seed,
                                                     row_builder=R.builder(games))
        return {s: _load(Path(res.shard_dir) / s) for s in ("train", "val")}

    a, b, c = run(SEED, "a"), run(SEED, "b"), run(SEED + 1, "c")
    for s in ("train", "val"):
        assert len(a[s]) == len(b[s])
        for x, y in zip(a[s], b[s]):
            T.assert_rows_equal(x, y, s)
    assert b"".join(x["observation"].tobytes() for x in a["train"]) != b"".join(x["observation"].tobytes() for x in c["train"])


def test_stored_and_compressed_shards_load_alike(games, tmp_path):
    import zipfile

    out = {}
    for compress in (False, True):
        res = shards.prepare_training_set_with_split(games, tmp_path / str(compress), val_ratio=0.3, positions_per_shard=40,
                                                     seed=SEED, compress=compress, row_builder=R.builder(games))
        d = Path(res.shard_dir)
        with zipfile.ZipFile(d / "train" / "shard_0000.npz") as z:
            kinds = {i.compress_type for i in z.infolist()}
        assert kinds == ({zipfile.ZIP_DEFLATED} if compress else {zipfile.ZIP_STORED})
        out[compress] = {s: _load(d / s) for s in ("train", "val")}
    for s in ("train", "val"):
        for x, y in zip(out[False][s], out[True][s]):
            T.assert_rows_equal(x, y, s)


def test_without_the_split(games, tmp_path):
    d = shards.prepare_training_set(games, tmp_path, positions_per_shard=33, seed=SEED, row_builder=R.builder(games))
    n = sum(g["n"] for g in games)
    want = R.shards(R.take(R.stack_rows(games), np.random.default_rng(SEED).permutation(n)), 33)  # sharding.py:143-153
    _assert_split(d, want, 33, 5, 5, d.name)


def test_bundles_round_trip_into_the_same_rows(games, tmp_path):
    batch = tmp_path / "group" / "batch0"
    (batch / "games").mkdir(parents=True)
    B.write_games(games[:4], batch / "games" / "bundle_a.npz")
    B.write_games(games[4:], batch / "games" / "bundle_b.npz")
    back = shards.read_bundle_dirs([batch])
    assert [g["n"] for g in back] == [g["n"] for g in games]
    T.assert_rows_equal(R.stack_rows(back), R.stack_rows(games), "bundle games")
    # and through the writer, which reads the directory itself: the listing is the bundles' games in file order
    res = shards.prepare_training_set_with_split([batch], tmp_path / "out", val_ratio=0.3, positions_per_shard=40, seed=SEED,
                                                 row_builder=R.builder(games))
    want = R.training_set(games, 0.3, 40, SEED)
    d = Path(res.shard_dir)
    _assert_split(d / "train", want["train"], 40, 5, 5, f"{res.shard_id}_train", batches=["group/batch0"])
    _assert_split(d / "val", want["val"], 40, 5, 5, f"{res.shard_id}_val", batches=["group/batch0"])
    # the views the uploads are made from carry the records unchanged
    keep: list = []
    v = shards._view_of(back[0], keep)
    n = back[0]["n"]
    assert (v.width, v.height, v.n_positions, v.max_turns) == (5, 5, n, games[0]["max_turns"])
    assert np.ctypeslib.as_array(v.policy_p1, shape=(n * 5,)).tobytes() == games[0]["policy_p1"].astype(np.float32).tobytes()
    assert np.array_equal(np.ctypeslib.as_array(v.cheese_outcomes, shape=(25,)).reshape(5, 5), games[0]["cheese_outcomes"])


def test_no_device_is_an_error():
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    h = C.c_void_p()
    assert _lib.load().ar_rows_open(5, 5, 100, 0, C.byref(h)) == _lib.AR_E_DEVICE and not h
    with pytest.raises(RuntimeError, match="no HIP device"):
        shards.RowSet(5, 5, 100)
    with pytest.raises(RuntimeError, match="no HIP device"):  # the default row builder is the device: there is no CPU path
        shards.prepare_training_set_with_split([dict(width=5, height=5, turn=np.zeros(3))], "/nonexistent", seed=0)
