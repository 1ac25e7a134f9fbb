"""The supply of a run's games (alpharat_amd/csrc/host_games.h GameSupply), compiled for the CPU by tests/hostsim_games:
the one owner of "which game has index i" for self-play sessions and matches. Compared with the oracle's generators game by
game, its random start cells pinned against a self-play run of the commit before GameSupply existed, its error messages,
and a sweep of every board size under AddressSanitizer and UBSan (a stand-alone program, run as a child process)."""
import subprocess

import numpy as np
import pytest

import _games as G
import _oracle as O

COUNT = {(5, 5): 5, (7, 5): 6, (16, 16): 20}
GSEED = 77


def _xy(cell, w):
    return (cell % w, cell // w)


@pytest.mark.parametrize("first", [0, 1000])
@pytest.mark.parametrize("cheese_symmetric", [True, False])
@pytest.mark.parametrize("maze_type", ["open", "classic", "random"])
@pytest.mark.parametrize("w,h", sorted(COUNT))
def test_games_equal_the_oracles(w, h, maze_type, cheese_symmetric, first):
    wd, md, msym = 0.55, 0.25, False  # ("random" takes these, "classic" 0.7 / 0.1 / symmetric, "open" none)
    for nth in range(16):
        g = G.make_game(nth, width=w, height=h, cheese_count=COUNT[w, h], cheese_symmetric=cheese_symmetric,
                        maze_type=maze_type, wall_density=wd, mud_density=md, maze_symmetric=msym, seed=GSEED,
                        first_game_index=first)
        index = first + nth
        assert g["index"] == index and g["generated"] == (maze_type != "open")
        assert (g["p1"], g["p2"]) == (0, w * h - 1)
        og = O.Game(w, h, 30, p1=_xy(g["p1"], w), p2=_xy(g["p2"], w))
        if maze_type == "classic":
            og.random_maze(0.7, 0.1, True, GSEED + index)
        elif maze_type == "random":
            og.random_maze(wd, md, msym, GSEED + index)
        np.testing.assert_array_equal(g["cost"], og.cost(), err_msg=f"maze of game {index}")
        og.random_cheese(COUNT[w, h], cheese_symmetric, GSEED + index)
        np.testing.assert_array_equal(g["cheese"], og.cheese_mask(), err_msg=f"cheese of game {index}")


@pytest.mark.parametrize("cheese_symmetric", [True, False])
@pytest.mark.parametrize("w,h", sorted(COUNT))
def test_random_start_cells(w, h, cheese_symmetric):
    hw, count = w * h, COUNT[w, h] - COUNT[w, h] % 2  # (even: a symmetric start cell may be the centre)
    kw = dict(width=w, height=h, cheese_count=count, cheese_symmetric=cheese_symmetric, maze_type="classic",
              positions="random", seed=GSEED, first_game_index=5)
    starts = set()
    for nth in range(16):
        g = G.make_game(nth, **kw)
        assert 0 <= g["p1"] < hw and 0 <= g["p2"] < hw
        if cheese_symmetric:
            assert g["p2"] == hw - 1 - g["p1"]
        assert g["cheese"][g["p1"]] == 0 and g["cheese"][g["p2"]] == 0 and g["cheese"].sum() == count
        og = O.Game(w, h, 30, p1=_xy(g["p1"], w), p2=_xy(g["p2"], w)).random_cheese(count, cheese_symmetric, GSEED + g["index"])
        np.testing.assert_array_equal(g["cheese"], og.cheese_mask())
        again = G.make_game(nth, **kw)  # the same index gives the same game
        assert (again["p1"], again["p2"]) == (g["p1"], g["p2"])
        assert again["cheese"].tobytes() == g["cheese"].tobytes() and again["cost"].tobytes() == g["cost"].tobytes()
        starts.add((g["p1"], g["p2"]))
    assert len(starts) > 4  # (they are drawn, not fixed)


# (p1, p2) of games 0..7 of rust_self_play(width=5, height=5, cheese_count=4, positions="random", seed=1), read from the
# records of a sink run on the commit before GameSupply (SelfPlaySession::make_game), symmetric cheese and not
PINNED_5X5_SEED1 = {
    True: [(12, 12), (0, 24), (16, 8), (4, 20), (20, 4), (18, 6), (15, 9), (3, 21)],
    False: [(12, 15), (0, 0), (16, 22), (4, 19), (20, 1), (18, 8), (15, 4), (3, 5)],
}


@pytest.mark.parametrize("cheese_symmetric", [True, False])
def test_random_start_cells_are_those_of_the_earlier_self_play(cheese_symmetric):
    got = []
    for nth in range(8):
        g = G.make_game(nth, width=5, height=5, cheese_count=4, cheese_symmetric=cheese_symmetric, positions="random", seed=1)
        got.append((g["p1"], g["p2"]))
    assert got == PINNED_5X5_SEED1[cheese_symmetric]


def test_error_messages():
    kw = dict(width=4, height=4, cheese_count=4)
    with pytest.raises(ValueError, match="^odd symmetric cheese count needs a free centre cell$"):
        G.make_game(0, **{**kw, "cheese_count": 3})  # (16 cells: no centre)
    with pytest.raises(ValueError, match="^odd symmetric cheese count needs a free centre cell$"):
        G.make_game(0, width=5, height=5, cheese_count=5, positions="random", seed=1)  # (game 0 starts on the centre)
    with pytest.raises(ValueError, match="^cheese_count does not fit the board$"):
        G.make_game(0, **{**kw, "cheese_count": 16})
    with pytest.raises(ValueError, match="^cheese_count does not fit the board$"):
        G.make_game(0, **{**kw, "cheese_count": 15, "cheese_symmetric": False})
    with pytest.raises(ValueError, match="^unknown maze_type: hexagonal$"):
        G.make_game(0, **kw, maze_type="hexagonal")
    with pytest.raises(ValueError, match="^unknown positions: centre$"):
        G.make_game(0, **kw, positions="centre")
    for w, h in ((0, 4), (4, 0), (17, 16)):
        with pytest.raises(ValueError, match=r"^board must have 1\.\.256 cells$"):
            G.make_game(0, **{**kw, "width": w, "height": h})
    assert G.make_game(0, **kw, maze_type=None, positions=None)["generated"] is False  # (the defaults: open, corners)


def test_sweep_under_the_sanitizers():
    """tests/hostsim_games/games_sweep.cpp, a program of its own built with -fsanitize=address,undefined: boards 1x2 ..
    16x16, the three maze types, both start-cell modes, both symmetries, the error paths."""
    subprocess.run(["make", "-s", "-C", str(G.HERE), "games_sweep"], check=True)
    r = subprocess.run([str(G.HERE / "games_sweep")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: ") and r.stderr == "", r.stdout + r.stderr
