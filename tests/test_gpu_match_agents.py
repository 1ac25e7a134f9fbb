"""-m gpu: device-resident matches with agents that do not search (ar_match_run: k_match_greedy, the engine-less path,
k_match_move_agents) and with a sampling temperature, against the semantics restated on the CPU (tests/_agents.py
oracle_game) at record level: positions, both actions, both agents' search outputs and counters, results and scores.
Bar: bit-exact. Last: a match's games against self-play's and the CPU harness of the game supply (tests/hostsim_games)."""
from pathlib import Path

import numpy as np
import pytest

import _agents as A
import _match as M
import _oracle as O

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).parent / "golden" / "nets"
SEED_A, SEED_B = 0xA0000, 0xB0000
OPEN5 = dict(width=5, height=5, cheese_count=5, max_turns=30)
MAZE7 = dict(width=7, height=7, cheese_count=10, max_turns=40, maze_type="random", wall_density=0.5, mud_density=0.4)


def _by_index(res):
    d = {g["game_index"]: g for g in res.games}
    assert len(d) == len(res.games)
    return d


def _check_stats(res, games):
    n = len(games)
    assert res.total_games == n and res.wins_a + res.wins_b + res.draws == n
    wins_a = sum(1 for g in games if g["result"] != 0 and (g["result"] == 1) == g["a_is_p1"])
    assert (res.wins_a, res.draws) == (wins_a, sum(1 for g in games if g["result"] == 0))
    assert res.total_positions == sum(g["n"] for g in games)
    for x in ("a", "b"):
        for mine, theirs in (("simulations", "total_visits"), ("nn_evals", "nn_evals"), ("terminals", "terminals"),
                             ("collisions", "collisions")):
            assert getattr(res, f"{mine}_{x}") == sum(int(g[x][theirs].sum()) for g in games), (x, mine)


def _no_search_outputs(res, games, x):
    for k in ("simulations", "nn_evals", "terminals", "collisions"):
        assert getattr(res, f"{k}_{x}") == 0, (x, k)
    for g in games:
        assert not any(np.asarray(v).any() for v in g[x].values()), (g["game_index"], x)


def _compare(games, og_of, a, b, indices, swap=True):
    for i in indices:
        want = A.oracle_game(og_of(i), i, a, b, a_is_p1=(i % 2 == 0) or not swap)
        M.assert_same_game(M.from_play_match(games[i]), want, f"game {i}")
        s1, s2 = want["final"]
        assert games[i]["result"] == (1 if s1 > s2 else 2 if s2 > s1 else 0), i
        assert (games[i]["final_p1_score"], games[i]["final_p2_score"]) == (float(s1), float(s2)), i


def test_greedy_against_random_without_any_engine():
    from alpharat_amd.match import MatchAgent, play_match

    res = play_match(MatchAgent.greedy(), MatchAgent.random(seed=SEED_B), num_games=40, swap_sides=True, seed=0,
                     concurrent_games=16, keep_games=True, **OPEN5)
    games = _by_index(res)
    assert sorted(games) == list(range(40)) and (res.agent_a, res.agent_b) == ("greedy", "random")
    _compare(games, lambda i: O.Game(5, 5, 30).random_cheese(5, True, i), A.Agent(A.GREEDY), A.Agent(A.RANDOM, seed=SEED_B),
             range(40))
    _check_stats(res, list(games.values()))
    _no_search_outputs(res, list(games.values()), "a")
    _no_search_outputs(res, list(games.values()), "b")
    assert res.avg_cheese_a > res.avg_cheese_b


def _maze7_game(i):
    return O.Game(7, 7, 40).random_maze(0.5, 0.4, True, i).random_cheese(10, True, i)


def _play_greedy_against_search(concurrent):
    from alpharat_amd.match import MatchAgent, play_match

    return play_match(MatchAgent.greedy(), MatchAgent("uniform_40", simulations=40, batch_size=8, seed=SEED_B), num_games=24,
                      swap_sides=True, seed=0, concurrent_games=concurrent, keep_games=True, **MAZE7)


@pytest.fixture(scope="module")
def greedy_against_search():
    return _play_greedy_against_search(8)


def test_greedy_against_search_on_a_muddy_maze(greedy_against_search):
    res = greedy_against_search
    games = _by_index(res)
    assert sorted(games) == list(range(24))
    b = A.Agent(A.SEARCH, M.Agent(O.make_config(), 40, 8, SEED_B))
    _compare(games, _maze7_game, A.Agent(A.GREEDY), b, range(24))
    _check_stats(res, list(games.values()))
    _no_search_outputs(res, list(games.values()), "a")
    assert res.simulations_b > 0
    assert any(g["p1_mud"].any() or g["p2_mud"].any() for g in games.values())  # moves were recorded in mud


@pytest.mark.parametrize("concurrent", [4, 64])
def test_scheduling_does_not_matter(greedy_against_search, concurrent):
    want = _by_index(greedy_against_search)
    got = _by_index(_play_greedy_against_search(concurrent))
    assert sorted(got) == sorted(want)
    for i, g in want.items():
        M.assert_same_game(M.from_play_match(got[i]), M.from_play_match(g), f"game {i}")
        assert got[i]["result"] == g["result"]


def test_greedy_against_random_above_64_cells():
    from alpharat_amd.match import MatchAgent, play_match

    res = play_match(MatchAgent.greedy(), MatchAgent.random(seed=SEED_B), width=11, height=9, cheese_count=12, max_turns=40,
                     num_games=8, swap_sides=True, seed=5, concurrent_games=8, keep_games=True, maze_type="random",
                     wall_density=0.5, mud_density=0.4)
    games = _by_index(res)
    assert sorted(games) == list(range(8))
    _compare(games, lambda i: O.Game(11, 9, 40).random_maze(0.5, 0.4, True, 5 + i).random_cheese(12, True, 5 + i),
             A.Agent(A.GREEDY), A.Agent(A.RANDOM, seed=SEED_B), range(8))
    _check_stats(res, list(games.values()))


@pytest.mark.parametrize("temperature", [0.0, 1.0, 0.5])
def test_pure_network_agent_against_random(temperature):
    from alpharat_amd.match import MatchAgent, play_match
    from test_gpu_pipeline_parity import HipEvaluator

    blob = GOLD / "mlp_5x5_h32.arnet"
    res = play_match(MatchAgent.nn(blob, temperature=temperature, seed=SEED_A), MatchAgent.random(seed=SEED_B), num_games=12,
                     swap_sides=True, seed=0, concurrent_games=8, keep_games=True, **OPEN5)
    games = _by_index(res)
    assert sorted(games) == list(range(12))
    _check_stats(res, list(games.values()))
    for g in games.values():
        assert (g["a"]["nn_evals"] == 1).all() and (g["a"]["total_visits"] == 1).all(), g["game_index"]
        if temperature == 0.0:
            mine = g["a"]["policy_p1"] if g["a_is_p1"] else g["a"]["policy_p2"]
            played = g["action_p1"] if g["a_is_p1"] else g["action_p2"]
            assert mine.any(axis=1).all()
            np.testing.assert_array_equal(played, np.argmax(mine, axis=1))
    ev = HipEvaluator(blob, 5, 5, 30)
    a = A.Agent(A.SEARCH, M.Agent(O.make_config(), 1, 1, SEED_A, backend=4, net=ev.backend), temperature)
    _compare(games, lambda i: O.Game(5, 5, 30).random_cheese(5, True, i), a, A.Agent(A.RANDOM, seed=SEED_B), (0, 5, 11))


def test_a_match_plays_the_games_self_play_generates():
    """Generated mazes and random start cells: game i of a match is the game self-play generates for the same index, and
    both are the game of the one GameSupply (tests/hostsim_games, the same header on the CPU)."""
    import _games as G
    from alpharat_amd.match import MatchAgent, play_match
    from alpharat_amd.sampling import rust_self_play

    res = play_match(MatchAgent.random(seed=SEED_A), MatchAgent.greedy(), num_games=8, seed=3, positions="random",
                     keep_games=True, **MAZE7)
    match = _by_index(res)
    played = {}
    rust_self_play(num_games=8, seed=3, positions="random", simulations=8, batch_size=4, output_dir=None,
                   on_game=lambda g: played.__setitem__(g["game_index"], g), **MAZE7)
    assert sorted(match) == sorted(played) == list(range(8))
    starts = set()
    for i in range(8):
        want = G.make_game(i, seed=3, positions="random", **MAZE7)
        assert want["index"] == i and want["generated"]
        for rec, who in ((match[i], "match"), (played[i], "self-play")):
            for side in ("p1", "p2"):
                x, y = (int(v) for v in rec[f"{side}_pos"][0])
                assert y * 7 + x == want[side], (i, who, side)
            np.testing.assert_array_equal(rec["cheese_mask"][0], want["cheese"], err_msg=f"game {i}, {who}")
        np.testing.assert_array_equal(match[i]["p1_pos"][0], played[i]["p1_pos"][0])
        np.testing.assert_array_equal(match[i]["p2_pos"][0], played[i]["p2_pos"][0])
        np.testing.assert_array_equal(match[i]["cheese_mask"][0], played[i]["cheese_mask"][0])
        np.testing.assert_array_equal(np.where(played[i]["maze"] < 0, 0, played[i]["maze"]), want["cost"], err_msg=f"maze {i}")
        starts.add((want["p1"], want["p2"]))
    assert len(starts) > 2  # (drawn, not the corners)
