"""Training rows on the CPU: the row of a position and the cheese outcomes of a game (alpharat_amd/csrc/dev_rows.h, compiled
for the CPU by tests/hostsim_rows) against the NumPy restatement of the reference's sharding step (tests/_rows_np.py), on
games played by the oracle. The restatement itself is tied to the reference by the encoder fixtures (1e-6, the tolerance of
the reference's parity test); everything else is equality of bytes."""
import json
from pathlib import Path

import numpy as np
import pytest

import _oracle as O
import _rows as T
import _rows_np as R

GOLDEN = Path(__file__).parent / "golden" / "encoder"


# ---- the restatement and the reference's fixtures -------------------------------------------------------------------
def _fixture_game(fx) -> O.Game:
    xy = lambda d: (d["x"], d["y"])  # noqa: E731
    g = O.Game(fx["width"], fx["height"], fx["max_turns"], p1=xy(fx["p1_pos"]), p2=xy(fx["p2_pos"]),
               cheese=[xy(c) for c in fx["cheese"]], walls=[(xy(w["pos1"]), xy(w["pos2"])) for w in fx["walls"]],
               mud=[(xy(m["pos1"]), xy(m["pos2"]), m["value"]) for m in fx["mud"]])
    for d1, d2 in fx.get("moves", []):
        g.make_move(d1, d2)
    return g


@pytest.mark.parametrize("path", sorted(GOLDEN.glob("*.json")), ids=lambda p: p.stem)
def test_restatement_reproduces_the_reference_fixtures(path):
    fx = json.loads(path.read_text())
    g = _fixture_game(fx)
    st = g.state()
    got = R.observation_from(fx["width"], fx["height"], fx["max_turns"], g.maze(), st["p1"], st["p2"], g.cheese_mask(),
                             st["p1_score"], st["p2_score"], st["turn"], st["p1_mud"], st["p2_mud"])
    want = np.asarray(fx["expected"], dtype=np.float32)
    assert got.dtype == np.float32 and got.shape == want.shape
    np.testing.assert_allclose(got, want, atol=1e-6, rtol=0)  # crates/alpharat-sampling/tests/parity.rs:16
    # and the oracle's encoder, which the same fixtures pin, gives the same bytes
    assert got.tobytes() == g.encode().tobytes()


# ---- rows ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=T.BOARDS, ids=lambda b: b[0])
def board(request):
    games = T.board_games(*request.param)
    return request.param, games, R.stack_rows(games)


def test_rows_equal_the_restatement_byte_for_byte(board):
    (name, w, h, *_), games, want = board
    n = len(want["value_p1"])
    assert n == sum(g["n"] for g in games) and n > 0
    rng = np.random.default_rng(5)
    orders = dict(identity=np.arange(n), reversed=np.arange(n)[::-1], permutation=rng.permutation(n),
                  repeated=rng.integers(0, n, size=n + 3))
    for what, rows in orders.items():
        for reverse in (False, True):  # (no lane may depend on the order the lanes run in)
            got = T.sim_build(games, rows, reverse=reverse)
            T.assert_rows_equal(got, R.take(want, rows), f"{name} {what} reverse={reverse}")
    # dtypes and shapes of the table in the header
    got = T.sim_build(games, np.arange(n))
    assert got["observation"].shape == (n, w * h * 7 + 6) and got["cheese_outcomes"].shape == (n, h, w)
    assert got["action_p1"].dtype == np.int8 and got["cheese_outcomes"].dtype == np.int8


def test_the_boards_cover_what_they_are_there_for(board):
    (name, w, h, max_turns, *_), games, want = board
    if name == "5x5 open":
        assert len({g["n"] for g in games}) > 1            # games of different lengths in one set
    if name == "15x11 maze":
        costs = np.concatenate([g["cost"] for g in games])
        assert (costs >= 2).any() and (costs == 0).any()    # mud and walls: observation values >= 0.2 and -1
        assert max(int(g["p1_mud"].max()) + int(g["p2_mud"].max()) for g in games) > 0  # non-zero mud timers
        assert w * h > 2 * 64                              # more than two strides per lane
    if name == "16x16":
        assert any((g["p2_pos"][:, 1] * w + g["p2_pos"][:, 0] == 255).any() for g in games)  # cell index 255
    if name == "one position":
        assert [g["n"] for g in games] == [1]
    if name == "7x5":
        assert w != h and any(len(set(g["p1_pos"][:, 0])) > 1 and len(set(g["p1_pos"][:, 1])) > 1 for g in games)


def test_outcome_rule_equals_the_records_of_the_oracle(board):
    (name, *_), games, _ = board
    for g in games:
        f = g["final"]
        want = np.asarray(g["cheese_outcomes"])
        assert np.array_equal(R.cheese_outcomes_rule(g, f["p1"], f["p2"], f["mask"]), want), name
        for lanes in (64, 128):
            for reverse in (False, True):
                assert np.array_equal(T.sim_outcomes(g, lanes, reverse), want), (name, lanes, reverse)
    # rows built with the outcomes of the rule (an attached run) are the rows built with the records' outcomes
    n = sum(g["n"] for g in games)
    T.assert_rows_equal(T.sim_build(games, np.arange(n), use_rule=True), T.sim_build(games, np.arange(n)), name)


def test_cheese_left_at_the_end_is_never_collected():
    games = T.board_games("short", 7, 7, 6, 9, None, 2, 24)
    for g in games:
        co = np.asarray(g["cheese_outcomes"])
        left = g["final"]["mask"].reshape(7, 7) == 1
        assert left.any() and (co[left] == 2).all()
        assert np.array_equal(T.sim_outcomes(g), co)
    want = R.stack_rows(games)
    n = len(want["value_p1"])
    T.assert_rows_equal(T.sim_build(games, np.arange(n), use_rule=True), want, "cheese left")
    # the last row of a game still shows the cheese that stays, with outcome 2
    last = games[0]["n"] - 1
    assert (want["cheese_outcomes"][last][left_of(games[0])] == 2).all()


def left_of(g):
    return g["final"]["mask"].reshape(g["height"], g["width"]) == 1


def test_both_players_on_one_cheese_in_the_same_move():
    g = T.simultaneous_game()
    co = np.asarray(g["cheese_outcomes"])
    assert co[2, 2] == 1 and co[2, 4] == 3 and co[0, 0] == 2 and co[4, 4] == 2
    for reverse in (False, True):
        assert np.array_equal(T.sim_outcomes(g, 128, reverse), co)
    want = R.game_rows(g)
    assert want["value_p1"][0] == np.float32(0.5) and want["value_p2"][0] == np.float32(1.5)
    assert want["cheese_outcomes"][0][2, 2] == 1 and want["cheese_outcomes"][1][2, 2] == -1
    for reverse in (False, True):
        T.assert_rows_equal(T.sim_build([g], np.arange(g["n"]), reverse=reverse, use_rule=True), want, "simultaneous")


def test_row_index_out_of_range_is_refused():
    g = T.simultaneous_game()
    keep: list = []
    gs = (T.RsGame * 1)(T._rs_game(g, keep))
    rows = np.array([g["n"]], np.uint64)
    out = T.empty_rows(1, 5, 5)
    assert T.sim().rs_build(gs, 1, rows.ctypes.data, 1, 0, 0, *[out[k].ctypes.data for k in R.KEYS]) == -1
