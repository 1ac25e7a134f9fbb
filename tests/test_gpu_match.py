"""-m gpu: device-resident head-to-head matches (ar_match_run: two engines' search pipelines, k_match_move, drains and
refills) against the match restated on the CPU oracle (tests/_match.py oracle_game) at record level: positions, both
actions, both agents' policies, values, visit counts, priors and counters, results and scores. Bar: bit-exact."""
from pathlib import Path

import numpy as np
import pytest

import _match as M
import _oracle as O

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).parent / "golden" / "nets"
SEED_A, SEED_B = 0xA0000, 0xB0000
GAME = dict(width=5, height=5, cheese_count=5, max_turns=30)


def _uniform_agents():
    from alpharat_amd.match import MatchAgent

    return (MatchAgent("uniform_40", simulations=40, batch_size=8, seed=SEED_A),
            MatchAgent("uniform_100", simulations=100, batch_size=16, seed=SEED_B))


def _play(concurrent, num_games=70):
    from alpharat_amd.match import play_match

    a, b = _uniform_agents()
    return play_match(a, b, num_games=num_games, swap_sides=True, seed=0, concurrent_games=concurrent, keep_games=True, **GAME)


@pytest.fixture(scope="module")
def uniform_match():
    return _play(32)


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
    cheese_a = sum(g["final_p1_score"] if g["a_is_p1"] else g["final_p2_score"] for g in games)
    cheese_b = sum(g["final_p2_score"] if g["a_is_p1"] else g["final_p1_score"] for g in games)
    assert res.avg_cheese_a == pytest.approx(cheese_a / n) and res.avg_cheese_b == pytest.approx(cheese_b / n)


def test_uniform_against_uniform_all_games_equal_the_oracle(uniform_match):
    games = _by_index(uniform_match)
    assert sorted(games) == list(range(70))
    a = M.Agent(O.make_config(), 40, 8, SEED_A)
    b = M.Agent(O.make_config(), 100, 16, SEED_B)
    for i in range(70):
        g = games[i]
        want = M.oracle_game(O.Game(5, 5, 30).random_cheese(5, True, i), i, a, b, a_is_p1=i % 2 == 0)
        M.assert_same_game(M.from_play_match(g), want, f"game {i}")
        s1, s2 = want["final"]
        assert g["result"] == (1 if s1 > s2 else 2 if s2 > s1 else 0), i
    _check_stats(uniform_match, list(games.values()))
    assert (uniform_match.agent_a, uniform_match.agent_b) == ("uniform_40", "uniform_100")


def test_two_networks_equal_the_oracle_driven_by_the_device_evaluators():
    from alpharat_amd.match import MatchAgent, play_match
    from test_gpu_pipeline_parity import HipEvaluator

    blobs = (GOLD / "mlp_5x5_h32.arnet", GOLD / "symmetric_5x5_h32.arnet")
    res = play_match(MatchAgent("mlp", checkpoint=blobs[0], simulations=64, batch_size=8, seed=SEED_A),
                     MatchAgent("symmetric", checkpoint=blobs[1], simulations=64, batch_size=8, seed=SEED_B),
                     num_games=24, swap_sides=True, seed=0, concurrent_games=16, keep_games=True, **GAME)
    games = _by_index(res)
    assert sorted(games) == list(range(24)) and res.nn_evals_a > 0 and res.nn_evals_b > 0
    _check_stats(res, list(games.values()))
    ev = [HipEvaluator(b, 5, 5, 30) for b in blobs]
    a = M.Agent(O.make_config(), 64, 8, SEED_A, backend=4, net=ev[0].backend)
    b = M.Agent(O.make_config(), 64, 8, SEED_B, backend=4, net=ev[1].backend)
    for i in (0, 23, 7, 10, 16, 17):  # first, last (a refilled slot), both orientations
        want = M.oracle_game(O.Game(5, 5, 30).random_cheese(5, True, i), i, a, b, a_is_p1=i % 2 == 0)
        M.assert_same_game(M.from_play_match(games[i]), want, f"game {i}")
        s1, s2 = want["final"]
        assert games[i]["result"] == (1 if s1 > s2 else 2 if s2 > s1 else 0), i
        assert (games[i]["final_p1_score"], games[i]["final_p2_score"]) == (float(s1), float(s2)), i


@pytest.mark.parametrize("concurrent", [4, 64])
def test_scheduling_does_not_matter(uniform_match, concurrent):
    want = _by_index(uniform_match)
    got = _by_index(_play(concurrent))
    assert sorted(got) == sorted(want)
    for i, g in want.items():
        M.assert_same_game(M.from_play_match(got[i]), M.from_play_match(g), f"game {i}")
        assert got[i]["result"] == g["result"]


def test_board_above_64_cells():
    from alpharat_amd.match import MatchAgent, play_match

    res = play_match(MatchAgent("a", simulations=32, batch_size=8, seed=SEED_A),
                     MatchAgent("b", simulations=32, batch_size=8, seed=SEED_B), width=11, height=9, cheese_count=10,
                     max_turns=20, num_games=8, swap_sides=True, seed=5, concurrent_games=8, keep_games=True)
    games = _by_index(res)
    assert sorted(games) == list(range(8))
    a = M.Agent(O.make_config(), 32, 8, SEED_A)
    b = M.Agent(O.make_config(), 32, 8, SEED_B)
    for i in range(8):
        want = M.oracle_game(O.Game(11, 9, 20).random_cheese(10, True, 5 + i), i, a, b, a_is_p1=i % 2 == 0)
        M.assert_same_game(M.from_play_match(games[i]), want, f"game {i}")
    _check_stats(res, list(games.values()))


def test_refusals_leave_the_library_usable():
    from alpharat_amd.match import MatchAgent, play_match

    a, b = _uniform_agents()
    with pytest.raises(ValueError, match="board"):
        play_match(MatchAgent("net", checkpoint=GOLD / "mlp_7x7_h256.arnet", simulations=16), b, num_games=2, seed=0, **GAME)
    with pytest.raises(ValueError, match="batch_size"):
        play_match(a, MatchAgent("b", simulations=16, batch_size=0), num_games=2, seed=0, **GAME)
    with pytest.raises(ValueError, match="maze_type"):
        play_match(a, b, num_games=2, seed=0, maze_type="hexagonal", **GAME)
    res = play_match(a, b, num_games=2, seed=0, **GAME)
    assert res.total_games == 2 and res.wins_a + res.wins_b + res.draws == 2 and res.simulations_a > 0
