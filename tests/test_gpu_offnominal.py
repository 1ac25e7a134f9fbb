"""-m gpu: search constants the kernels otherwise never see (tests/_constant_sets.py: c_puct 0 and 8, fpu_reduction 0 and 2,
force_k 0 and 50, noise that replaces the prior, the smallest legal gamma shape) through whole self-play runs, every game
against the oracle. Small shapes: 5x5, 30 turns, 120 simulations in batches of 8, 8 games in 4 resident slots, so that
slots are refilled, trees are reused from move to move and k_advance runs. SmartUniform on the open board goes through
k_gather8, k_uniform_eval and k_backup16; the network on generated mazes with mud through k_gatherw and the evaluator.
The same sets run through the CPU harness in test_kernel_logic_cpu.py, which tells a logic failure from a device one."""
from pathlib import Path

import numpy as np
import pytest

import _constant_sets as K
import _oracle as O
from test_gpu_parity import _check_game
from test_gpu_pipeline_parity import HipEvaluator

pytestmark = pytest.mark.gpu

MLP = Path(__file__).parent / "golden" / "nets" / "mlp_5x5_h32.arnet"
N_GAMES, RESIDENT = 8, 4


def _run_kwargs(board, s, games):
    extra = dict(weights_path=str(MLP), maze_type="random", wall_density=K.WALLS, mud_density=K.MUD,
                 maze_symmetric=True) if board == "maze" else {}
    return dict(width=K.W, height=K.H, cheese_count=K.CHEESE, max_turns=K.TURNS, num_games=N_GAMES, simulations=K.SIMS,
                batch_size=K.BATCH, output_dir=None, seed=0, concurrent_games=RESIDENT,
                on_game=lambda g: games.__setitem__(g["game_index"], g), **K.kwargs(s), **extra)


def _play(board, s):
    from alpharat_amd.sampling import rust_self_play

    games = {}
    stats = rust_self_play(**_run_kwargs(board, s, games))
    assert stats.total_games == N_GAMES and sorted(games) == list(range(N_GAMES))
    return games


_evaluator = []
_wanted = {}


def _want(board, s):
    """the oracle's records of the run's games, computed once per (board, set); on the maze board the oracle's leaves
    are evaluated by the device network on that game's own maze"""
    if (board, s) not in _wanted:
        cfg = O.make_config(**K.kwargs(s))
        out = []
        for i in range(N_GAMES):
            og = K.game(board, i)
            if board == "maze":
                if not _evaluator:
                    _evaluator.append(HipEvaluator(MLP, K.W, K.H, K.TURNS))
                ev = _evaluator[0]
                ev.cost = np.ascontiguousarray(og.cost(), dtype=np.uint8).reshape(-1)
                out.append(O.play_game(og, cfg, K.SIMS, K.BATCH, K.rng_seed(i), backend=4, net=ev.backend, game_index=i))
            else:
                out.append(O.play_game(og, cfg, K.SIMS, K.BATCH, K.rng_seed(i), game_index=i))
        _wanted[(board, s)] = out
    return _wanted[(board, s)]


def _check(games, want):
    for i, w in enumerate(want):
        _check_game(games[i], w)


@pytest.mark.parametrize("s", K.SETS, ids=K.IDS)
def test_uniform_selfplay_open_board(s):
    want = _want("open", s)
    _check(_play("open", s), want)
    assert sum(w["total_nn_evals"] for w in want) > 0


@pytest.mark.parametrize("s", K.SETS, ids=K.IDS)
def test_network_selfplay_generated_mazes_with_mud(s):
    want = _want("maze", s)
    games = _play("maze", s)
    _check(games, want)
    assert any((g["maze"] >= 2).any() for g in games.values()) and any((g["maze"][:-1, :-1, :2] == -1).any() for g in games.values())
    assert sum(w["total_nn_evals"] for w in want) > 0


@pytest.mark.parametrize("backup", ["lane", None], ids=["backup-lane", "backup-default"])
@pytest.mark.parametrize("gather,kind", [("wide", 2), ("octet3", 1), ("lane", 0)])
@pytest.mark.parametrize("low", [True, False], ids=["all-zero", "all-high"])
def test_extreme_sets_with_full_noise_on_every_gather_and_backup(low, gather, kind, backup, monkeypatch):
    """(0, 0, 0) and (8, 2, 50) with the prior replaced by noise of the smallest shape, on each gather kernel of the
    network path with each backup kernel."""
    from alpharat_amd.sampling import SelfPlaySession

    s = (*(K.LOW if low else K.HIGH), *K.NOISE[1])
    assert s in K.SETS
    monkeypatch.setenv("AR_GATHER", gather)
    if backup:
        monkeypatch.setenv("AR_BACKUP", backup)
    else:
        monkeypatch.delenv("AR_BACKUP", raising=False)
    games = {}
    with SelfPlaySession(**_run_kwargs("maze", s, games)) as session:
        assert session.info()["gather_kind"] == kind, session.info()
        session.run_to_end()
    assert sorted(games) == list(range(N_GAMES))
    _check(games, _want("maze", s))


def test_concentration_of_five_is_refused_with_noise_and_accepted_without():
    """concentration / 5 must exceed 1 (the Gamma sampler restated on both sides is the one for shapes above 1): with noise
    the product refuses the configuration up front, and the oracle stops at the first root with five outcomes."""
    from alpharat_amd.game import PyRat
    from alpharat_amd.mcts import rust_mcts_search
    from alpharat_amd.sampling import rust_self_play

    centre = PyRat.create_custom(5, 5, cheese=[(0, 0), (4, 4)], player1_pos=(2, 2), player2_pos=(2, 2), max_turns=30)
    og = O.Game(5, 5, 30, p1=(2, 2), p2=(2, 2), cheese=[(0, 0), (4, 4)])
    bad = dict(noise_epsilon=0.25, noise_concentration=5.0)
    with pytest.raises(ValueError, match="noise_concentration must exceed 5"):
        rust_mcts_search(centre, simulations=20, batch_size=4, seed=1, **bad)
    with pytest.raises(ValueError, match="noise_concentration must exceed 5"):
        rust_self_play(width=5, height=5, cheese_count=5, max_turns=30, num_games=2, simulations=20, batch_size=4,
                       output_dir=None, seed=0, **bad)
    with pytest.raises(RuntimeError, match="Dirichlet noise with concentration/n_outcomes <= 1"):
        O.search_once(og, O.make_config(**bad), 20, 4, seed=1)
    ok = dict(noise_epsilon=0.0, noise_concentration=5.0)
    from test_gpu_parity import _assert_result

    got = rust_mcts_search(centre, simulations=120, batch_size=8, seed=1, **ok)
    _assert_result(got, O.search_once(og, O.make_config(**ok), 120, 8, seed=1), "concentration 5 without noise")
