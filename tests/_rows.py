"""Games for the row tests and the driver of tests/hostsim_rows -- test infrastructure only.

A game is the record dict of tests/_bundles.py from_oracle (the sink's keys) plus `game_index` and, under `final`, the state
after the last move (cells of both players, cheese mask), which the cheese-outcome rule needs and a record does not carry.
"""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import _bundles as B
import _oracle as O
import _rows_np as R

HERE = Path(__file__).resolve().parent / "hostsim_rows"

# (name, width, height, max_turns, cheese, walls and mud densities or None = open, games, simulations)
BOARDS = [
    ("5x5 open", 5, 5, 30, 5, None, 4, 40),
    ("7x5", 7, 5, 30, 7, None, 3, 40),
    ("7x7", 7, 7, 40, 9, None, 3, 40),
    ("15x11 maze", 15, 11, 60, 21, (0.5, 0.5), 2, 24),
    ("16x16", 16, 16, 24, 30, None, 2, 16),
    ("one position", 5, 5, 1, 5, None, 1, 16),
]


def _final(og: O.Game, game: dict) -> dict:
    g = og.clone()
    for a1, a2 in zip(game["action_p1"], game["action_p2"]):
        g.make_move(int(a1), int(a2))
    st = g.state()
    return dict(p1=st["p1"], p2=st["p2"], mask=g.cheese_mask().copy())


def played(og: O.Game, index: int, sims: int, batch: int = 8) -> dict:
    """One oracle self-play game (SmartUniform) as a record dict."""
    want = O.play_game(og, O.make_config(), sims, batch, 0xA1FA0000 + index, game_index=index)
    game = B.from_oracle(want)
    game["game_index"] = index
    game["cost"] = np.ascontiguousarray(og.cost().reshape(-1).astype(np.uint8))
    game["final"] = _final(og, game)
    return game


def board_games(name, w, h, max_turns, cheese, maze, n_games, sims) -> list:
    games = []
    for i in range(n_games):
        og = O.Game(w, h, max_turns)
        if maze is not None:
            og.random_maze(maze[0], maze[1], True, 11 + i)
        og.random_cheese(cheese, True, 100 + i)
        games.append(played(og, i, sims))
    return games


def scripted(og: O.Game, moves, index: int = 0) -> dict:
    """A game with given moves (no search): positions from the oracle's engine, policies that differ from row to row, and the
    cheese outcomes of the restated rule."""
    g = og.clone()
    w, h = og.w, og.h
    rows = dict(p1_pos=[], p2_pos=[], p1_mud=[], p2_mud=[], turn=[], p1_score=[], p2_score=[], cheese_mask=[])
    for a1, a2 in moves:
        assert not g.over()
        st = g.state()
        for k in ("p1_mud", "p2_mud", "turn", "p1_score", "p2_score"):
            rows[k].append(st[k])
        rows["p1_pos"].append(st["p1"])
        rows["p2_pos"].append(st["p2"])
        rows["cheese_mask"].append(g.cheese_mask().copy())
        g.make_move(a1, a2)
    assert g.over()
    n = len(moves)
    st = g.state()
    pol = (np.arange(n * 10, dtype=np.float32).reshape(n, 10) + 1) / np.float32(64)
    game = dict(width=w, height=h, n=n, max_turns=len(moves), game_index=index,
                result=1 if st["p1_score"] > st["p2_score"] else 2 if st["p2_score"] > st["p1_score"] else 0,
                final_p1_score=np.float32(st["p1_score"]), final_p2_score=np.float32(st["p2_score"]), maze=og.maze(),
                initial_cheese=rows["cheese_mask"][0].reshape(h, w), p1_pos=np.array(rows["p1_pos"], np.int32),
                p2_pos=np.array(rows["p2_pos"], np.int32), p1_mud=np.array(rows["p1_mud"], np.int32),
                p2_mud=np.array(rows["p2_mud"], np.int32), turn=np.array(rows["turn"], np.int32),
                p1_score=np.array(rows["p1_score"], np.float32), p2_score=np.array(rows["p2_score"], np.float32),
                cheese_mask=np.array(rows["cheese_mask"], np.uint8), action_p1=np.array([m[0] for m in moves], np.int32),
                action_p2=np.array([m[1] for m in moves], np.int32), policy_p1=pol[:, :5].copy(), policy_p2=pol[:, 5:].copy())
    for k in ("value_p1", "value_p2"):
        game[k] = np.zeros(n, np.float32)
    for k in ("visit_counts_p1", "visit_counts_p2", "prior_p1", "prior_p2"):
        game[k] = np.zeros((n, 5), np.float32)
    game["cost"] = np.ascontiguousarray(og.cost().reshape(-1).astype(np.uint8))
    game["final"] = dict(p1=st["p1"], p2=st["p2"], mask=g.cheese_mask().copy())
    game["cheese_outcomes"] = R.cheese_outcomes_rule(game, st["p1"], st["p2"], game["final"]["mask"])
    return game


def simultaneous_game() -> dict:
    """5x5: both players step onto the cheese at (2, 2) in the first move (outcome 1); the cheese at (0, 0) and (4, 4) is
    never taken (outcome 2); P2 then takes (4, 2) alone (outcome 3). Ends at max_turns = 4 with cheese left."""
    og = O.Game(5, 5, 4, p1=(1, 2), p2=(3, 2), cheese=[(2, 2), (0, 0), (4, 4), (4, 2)])
    return scripted(og, [(1, 3), (4, 1), (4, 1), (4, 4)], index=7)


# ---- tests/hostsim_rows ------------------------------------------------------------------------------------------------
class RsGame(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("max_turns", C.c_uint32), ("n", C.c_uint32),
                ("final1", C.c_float), ("final2", C.c_float), ("final_p1", C.c_uint32), ("final_p2", C.c_uint32),
                ("cost", C.c_void_p), ("outcomes", C.c_void_p), ("final_mask", C.c_void_p), ("ints", C.c_void_p),
                ("floats", C.c_void_p), ("masks", C.c_void_p)]


_sim = None


def sim() -> C.CDLL:
    global _sim
    if _sim is None:
        subprocess.run(["make", "-s", "-C", str(HERE)], check=True)
        L = C.CDLL(str(HERE / "librowssim.so"))
        L.rs_build.restype = C.c_int
        L.rs_build.argtypes = [C.POINTER(RsGame), C.c_uint32, C.c_void_p, C.c_uint64, C.c_int, C.c_int] + [C.c_void_p] * 8
        L.rs_outcomes.restype = None
        L.rs_outcomes.argtypes = [C.POINTER(RsGame), C.c_uint32, C.c_int, C.c_void_p]
        _sim = L
    return _sim


def _rs_game(game: dict, keep: list) -> RsGame:
    w, h, n = game["width"], game["height"], int(game["n"])
    ints = np.zeros((max(n, 1), 9), np.int32)
    fl = np.zeros((max(n, 1), 34), np.float32)
    ints[:n, 0:2], ints[:n, 2:4] = game["p1_pos"], game["p2_pos"]
    ints[:n, 4], ints[:n, 5], ints[:n, 6] = game["p1_mud"], game["p2_mud"], game["turn"]
    ints[:n, 7], ints[:n, 8] = game["action_p1"], game["action_p2"]
    fl[:n, 0], fl[:n, 1] = game["p1_score"], game["p2_score"]
    fl[:n, 24:29], fl[:n, 29:34] = game["policy_p1"], game["policy_p2"]
    arrs = dict(cost=np.ascontiguousarray(game["cost"], np.uint8),
                outcomes=np.ascontiguousarray(np.asarray(game["cheese_outcomes"]).reshape(-1), np.uint8),
                final_mask=np.ascontiguousarray(game["final"]["mask"], np.uint8), ints=ints, floats=fl,
                masks=np.ascontiguousarray(np.asarray(game["cheese_mask"]).reshape(max(n, 0), w * h), np.uint8))
    keep.extend(arrs.values())
    f = game["final"]
    return RsGame(w, h, game["max_turns"], n, float(game["final_p1_score"]), float(game["final_p2_score"]),
                  f["p1"][1] * w + f["p1"][0], f["p2"][1] * w + f["p2"][0], *[arrs[k].ctypes.data for k in
                                                                             ("cost", "outcomes", "final_mask", "ints",
                                                                              "floats", "masks")])


def empty_rows(n: int, w: int, h: int, fill: int = 0x5A) -> dict:
    """Output arrays for n rows, every byte preset to `fill` (a row the builder skips stays visible)."""
    shapes = dict(observation=(n, w * h * 7 + 6), policy_p1=(n, 5), policy_p2=(n, 5), value_p1=(n,), value_p2=(n,),
                  action_p1=(n,), action_p2=(n,), cheese_outcomes=(n, h, w))
    out = {}
    for k in R.KEYS:
        a = np.empty(shapes[k], R.DTYPES[k])
        a.view(np.uint8).fill(fill)
        out[k] = a
    return out


def sim_build(games, rows, reverse=False, use_rule=False) -> dict:
    keep: list = []
    gs = (RsGame * len(games))(*[_rs_game(g, keep) for g in games])
    rows = np.ascontiguousarray(rows, np.uint64)
    out = empty_rows(len(rows), games[0]["width"], games[0]["height"])
    rc = sim().rs_build(gs, len(games), rows.ctypes.data, len(rows), int(reverse), int(use_rule),
                        *[out[k].ctypes.data for k in R.KEYS])
    assert rc == 0, rc
    return out


def sim_outcomes(game, lanes=128, reverse=False) -> np.ndarray:
    keep: list = []
    g = _rs_game(game, keep)
    out = np.full(game["width"] * game["height"], 0x5A, np.uint8)
    sim().rs_outcomes(C.byref(g), lanes, int(reverse), out.ctypes.data)
    return out.reshape(game["height"], game["width"])


def assert_rows_equal(got: dict, want: dict, what="") -> None:
    for k in R.KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        if got[k].tobytes() != want[k].tobytes():
            bad = np.nonzero(got[k].reshape(len(got[k]), -1).view(np.uint8) != want[k].reshape(len(want[k]), -1).view(np.uint8))
            raise AssertionError(f"{what}: {k} differs, first at row {bad[0][0]} byte {bad[1][0]} ({len(set(bad[0]))} rows)")
