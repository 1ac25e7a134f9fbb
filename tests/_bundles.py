"""Bundles back into games -- test infrastructure only.

One dict per game, with the keys and shapes of the sink's record dict (alpharat_amd/sampling.py record_to_dict), so
that games read from a `bundle_<uuid>.npz`, records handed to an `on_game` sink and games played by the oracle are
compared by one function. Bundles carry no game index: collections of games are compared as multisets of
`canonical(game)` bytes, which needs no matching heuristic and cannot pair a game with the wrong partner.
Every comparison is equality of bytes: the writer only copies and casts (u8 -> i8 / bool, u16 -> i16, f32 -> f32).
"""
from __future__ import annotations

import ctypes as C
import struct
import zipfile

import numpy as np

from alpharat_amd import _lib

# array name -> dtype on disk: the 26 names of the reference's recording.rs, no more, no fewer
DTYPES = dict(game_lengths=np.int32, maze=np.int8, initial_cheese=np.bool_, cheese_outcomes=np.int8,
              max_turns=np.int16, result=np.int8, final_p1_score=np.float32, final_p2_score=np.float32,
              p1_pos=np.int8, p2_pos=np.int8, p1_score=np.float32,
              p2_score=np.float32, p1_mud=np.int8, p2_mud=np.int8, cheese_mask=np.bool_, turn=np.int16,
              value_p1=np.float32, value_p2=np.float32, visit_counts_p1=np.float32, visit_counts_p2=np.float32,
              prior_p1=np.float32, prior_p2=np.float32, policy_p1=np.float32, policy_p2=np.float32,
              action_p1=np.int8, action_p2=np.int8)

# canonical(): field -> (dtype, shape with n = positions, h, w, hw). Integers are widened to one fixed dtype each,
# floats stay the 4 bytes they are.
_GAME_FIELDS = (("width", np.int32, ()), ("height", np.int32, ()), ("max_turns", np.int32, ()), ("n", np.int32, ()),
                ("result", np.int32, ()), ("final_p1_score", np.float32, ()), ("final_p2_score", np.float32, ()),
                ("maze", np.int16, ("h", "w", 4)), ("initial_cheese", np.int16, ("h", "w")),
                ("cheese_outcomes", np.int16, ("h", "w")))
_POS_FIELDS = (("p1_pos", np.int16, ("n", 2)), ("p2_pos", np.int16, ("n", 2)), ("p1_score", np.float32, ("n",)),
               ("p2_score", np.float32, ("n",)), ("p1_mud", np.int16, ("n",)), ("p2_mud", np.int16, ("n",)),
               ("cheese_mask", np.int16, ("n", "hw")), ("turn", np.int32, ("n",)), ("value_p1", np.float32, ("n",)),
               ("value_p2", np.float32, ("n",)), ("visit_counts_p1", np.float32, ("n", 5)),
               ("visit_counts_p2", np.float32, ("n", 5)), ("prior_p1", np.float32, ("n", 5)),
               ("prior_p2", np.float32, ("n", 5)), ("policy_p1", np.float32, ("n", 5)),
               ("policy_p2", np.float32, ("n", 5)), ("action_p1", np.int16, ("n",)), ("action_p2", np.int16, ("n",)))
FIELDS = tuple(k for k, _, _ in _GAME_FIELDS + _POS_FIELDS)


def check_container(path) -> None:
    """The container contract of recording.rs / npz_writer.rs: 26 deflated .npy members, format 1.0, headers padded
    to 256 bytes, C order, and the dtypes of DTYPES."""
    with zipfile.ZipFile(path) as z:
        infos = z.infolist()
        assert len(infos) == 26 and all(i.filename.endswith(".npy") for i in infos)
        assert all(i.compress_type == zipfile.ZIP_DEFLATED for i in infos)
        for i in infos:
            raw = z.read(i)
            assert raw[:6] == b"\x93NUMPY" and raw[6:8] == b"\x01\x00"            # npy format 1.0
            hlen = struct.unpack("<H", raw[8:10])[0]
            assert (10 + hlen) % 256 == 0 and raw[10 + hlen - 1:10 + hlen] == b"\n"  # header padded to 256 bytes
            assert b"'fortran_order':False" in raw[10:10 + hlen].replace(b" ", b"")
    z = np.load(path)
    got = {k: z[k].dtype for k in z.files}
    assert sorted(got) == sorted(DTYPES)  # the 26 names of recording.rs, no more, no fewer
    for k, dt in got.items():
        assert dt == np.dtype(DTYPES[k]), (k, dt)


def read_games(path) -> list[dict]:
    """The games of one bundle, in file order. Width and height come from the `maze` shape; every other array must
    have the shape that follows from them, the number of games and the sum of `game_lengths`."""
    z = np.load(path)
    a = {k: z[k] for k in z.files}
    assert sorted(a) == sorted(DTYPES), sorted(a)
    for k, v in a.items():
        assert v.dtype == np.dtype(DTYPES[k]), (k, v.dtype)
    lengths = a["game_lengths"]
    assert lengths.ndim == 1 and len(lengths) > 0 and (lengths > 0).all()
    k_games, n_pos = len(lengths), int(lengths.sum())
    assert a["maze"].ndim == 4 and a["maze"].shape[0] == k_games and a["maze"].shape[3] == 4, a["maze"].shape
    h, w = a["maze"].shape[1:3]
    want_shapes = dict(game_lengths=(k_games,), maze=(k_games, h, w, 4), initial_cheese=(k_games, h, w),
                       cheese_outcomes=(k_games, h, w), max_turns=(k_games,), result=(k_games,),
                       final_p1_score=(k_games,), final_p2_score=(k_games,), p1_pos=(n_pos, 2), p2_pos=(n_pos, 2),
                       p1_score=(n_pos,), p2_score=(n_pos,), p1_mud=(n_pos,), p2_mud=(n_pos,),
                       cheese_mask=(n_pos, h, w), turn=(n_pos,), value_p1=(n_pos,), value_p2=(n_pos,),
                       visit_counts_p1=(n_pos, 5), visit_counts_p2=(n_pos, 5), prior_p1=(n_pos, 5), prior_p2=(n_pos, 5),
                       policy_p1=(n_pos, 5), policy_p2=(n_pos, 5), action_p1=(n_pos,), action_p2=(n_pos,))
    for k, s in want_shapes.items():
        assert a[k].shape == s, (k, a[k].shape, s)
    ends = np.cumsum(lengths)
    games = []
    for i in range(k_games):
        lo, hi = int(ends[i] - lengths[i]), int(ends[i])
        g = dict(width=int(w), height=int(h), n=hi - lo, max_turns=int(a["max_turns"][i]), result=int(a["result"][i]),
                 final_p1_score=a["final_p1_score"][i], final_p2_score=a["final_p2_score"][i], maze=a["maze"][i],
                 initial_cheese=a["initial_cheese"][i], cheese_outcomes=a["cheese_outcomes"][i])
        for k, _, _ in _POS_FIELDS:
            g[k] = a[k][lo:hi]
        g["cheese_mask"] = g["cheese_mask"].reshape(hi - lo, h * w)  # the sink's shape; (n, h, w) was checked above
        games.append(g)
    return games


def from_sink(g: dict) -> dict:
    """A sink record dict without the fields a bundle does not carry (game_index, total_*, cheese_available)."""
    d = {k: g[k] for k in FIELDS}
    for k in ("final_p1_score", "final_p2_score"):  # Python floats made from the view's f32: back to the same 4 bytes
        d[k] = np.float32(g[k])
        assert float(d[k]) == g[k], (k, g[k])
    return d


def from_oracle(want: dict) -> dict:
    """An `_oracle.play_game` result as the same dict. Per-position ints: p1x p1y p2x p2y p1_mud p2_mud turn a1 a2;
    floats: p1_score p2_score value_p1 value_p2 visits_p1[5] visits_p2[5] prior_p1[5] prior_p2[5] policy_p1[5]
    policy_p2[5] (oracle/capi.cpp or_record_positions)."""
    i, f = want["ints"], want["floats"]
    g = dict(width=want["width"], height=want["height"], n=want["n"], max_turns=want["max_turns"], result=want["result"],
             final_p1_score=np.float32(want["final_p1_score"]), final_p2_score=np.float32(want["final_p2_score"]),
             maze=want["maze"], initial_cheese=want["initial_cheese"], cheese_outcomes=want["cheese_outcomes"],
             p1_pos=i[:, 0:2], p2_pos=i[:, 2:4], p1_mud=i[:, 4], p2_mud=i[:, 5], turn=i[:, 6], action_p1=i[:, 7],
             action_p2=i[:, 8], p1_score=f[:, 0], p2_score=f[:, 1], value_p1=f[:, 2], value_p2=f[:, 3],
             visit_counts_p1=f[:, 4:9], visit_counts_p2=f[:, 9:14], prior_p1=f[:, 14:19], prior_p2=f[:, 19:24],
             policy_p1=f[:, 24:29], policy_p2=f[:, 29:34], cheese_mask=want["masks"])
    assert float(g["final_p1_score"]) == want["final_p1_score"] and float(g["final_p2_score"]) == want["final_p2_score"]
    return g


def _field_bytes(game: dict, k: str, dt, shape) -> bytes:
    dims = dict(n=game["n"], h=game["height"], w=game["width"], hw=game["width"] * game["height"])
    shape = tuple(dims.get(s, s) for s in shape)
    v = np.asarray(game[k])
    assert v.shape == shape, (k, v.shape, shape)
    if dt is np.float32:
        assert v.dtype == np.float32, (k, v.dtype)  # raw bits: no float is ever converted
        out = v
    else:
        assert v.dtype.kind in "iub", (k, v.dtype)
        out = v.astype(dt)
        assert np.array_equal(out, v.astype(np.int64)), (k, "does not fit", dt)
    return np.ascontiguousarray(out).tobytes()


def canonical(game: dict) -> bytes:
    """Every field of a game that a bundle carries, in a fixed order and fixed dtypes."""
    return b"".join(_field_bytes(game, k, dt, shape) for k, dt, shape in _GAME_FIELDS + _POS_FIELDS)


def multiset(games) -> list[bytes]:
    return sorted(canonical(g) for g in games)


def first_difference(a: dict, b: dict):
    """Name of the first field in which two games differ (for assertion messages), or None."""
    for k, dt, shape in _GAME_FIELDS + _POS_FIELDS:
        if _field_bytes(a, k, dt, shape) != _field_bytes(b, k, dt, shape):
            return k
    return None


def assert_same_games(got, want, what="") -> None:
    """Multiset equality of two collections of games. On a mismatch the message names the fields that differ when
    the two collections are also compared in the order given."""
    got, want = list(got), list(want)
    assert len(got) == len(want), (what, len(got), len(want))
    if multiset(got) != multiset(want):
        diffs = sorted({str(first_difference(g, w)) for g, w in zip(got, want)} - {"None"})
        raise AssertionError(f"{what}: the two collections of {len(got)} games differ (fields differing in the given "
                             f"order: {diffs or 'none -- same games, other multiplicities'})")


def view_of(game: dict, keep: list) -> _lib.ArGameRecordView:
    """An ArGameRecordView over copies of a game dict's arrays; `keep` holds the copies alive. The fields a bundle
    does not carry (game_index, cheese_available, total_*) are taken from the dict when present, else 0."""
    v = _lib.ArGameRecordView()
    v.width, v.height, v.max_turns = game["width"], game["height"], game["max_turns"]
    v.game_index = game.get("game_index", 0)
    v.n_positions = len(np.asarray(game["turn"]))
    v.final_p1_score, v.final_p2_score = float(game["final_p1_score"]), float(game["final_p2_score"])
    v.result, v.cheese_available = game["result"], game.get("cheese_available", 0)
    v.total_simulations, v.total_nn_evals = game.get("total_simulations", 0), game.get("total_nn_evals", 0)
    v.total_terminals, v.total_collisions = game.get("total_terminals", 0), game.get("total_collisions", 0)

    def ptr(arr, dt, ct):
        src = np.asarray(arr)
        a = np.ascontiguousarray(src, dtype=dt)
        if dt is not np.float32:
            assert np.array_equal(a.astype(np.int64), src.astype(np.int64)), "value does not fit the view's type"
        if a is arr or np.shares_memory(a, src):
            a = a.copy()
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(ct))

    v.maze = ptr(game["maze"], np.int8, C.c_int8)
    v.initial_cheese = ptr(game["initial_cheese"], np.uint8, C.c_uint8)
    v.cheese_outcomes = ptr(game["cheese_outcomes"], np.uint8, C.c_uint8)
    for k in ("p1_pos", "p2_pos", "p1_mud", "p2_mud", "action_p1", "action_p2", "cheese_mask"):
        setattr(v, k, ptr(game[k], np.uint8, C.c_uint8))
    v.turn = ptr(game["turn"], np.uint16, C.c_uint16)
    for k in ("p1_score", "p2_score", "value_p1", "value_p2", "visit_counts_p1", "visit_counts_p2", "prior_p1", "prior_p2",
              "policy_p1", "policy_p2"):
        setattr(v, k, ptr(game[k], np.float32, C.c_float))
    return v


def write_games(games, path) -> None:
    """ar_write_bundle (host code: works without a device) on game dicts."""
    keep: list = []
    views = (_lib.ArGameRecordView * len(games))(*[view_of(g, keep) for g in games])
    _lib.check(_lib.load().ar_write_bundle(views, len(games), str(path).encode()))
