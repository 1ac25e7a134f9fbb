"""-m gpu: k_backup16 (dev_backup16.h: a touched node is read once, updated for all its entries in batch order, written
once) through whole games: 5x5, 64 resident games, PyRatMLP h32. Chunks of sixteen entries that are full (batch 16), full
plus a part (24), and small batches over many simulations (3 x 200: deep, narrow trees). No root noise, so every batch,
the root's first included, goes through k_backup16. Every record of every game against the oracle (its leaves evaluated
by the same device network) and against the same run with the lane-per-game backup, byte for byte. Short games keep the
oracle's per-batch callbacks within seconds; the last test makes the search greedy, so that paths run past the levels
kept in LDS."""
from pathlib import Path

import numpy as np
import pytest

import _oracle as O
from test_gpu_parity import _check_game
from test_gpu_pipeline_parity import HipEvaluator

pytestmark = pytest.mark.gpu

MLP = Path(__file__).parent / "golden" / "nets" / "mlp_5x5_h32.arnet"
N_GAMES = 64


def _run(batch, sims, max_turns, **search):
    from alpharat_amd.sampling import SelfPlaySession

    games = {}
    with SelfPlaySession(width=5, height=5, cheese_count=5, max_turns=max_turns, num_games=N_GAMES, simulations=sims,
                         batch_size=batch, seed=0, concurrent_games=N_GAMES, weights_path=str(MLP), noise_epsilon=0.0,
                         on_game=lambda g: games.__setitem__(g["game_index"], g), **search) as s:
        stats = s.run_to_end()
    assert sorted(games) == list(range(N_GAMES))
    return games, stats


def _same_records(a, b):
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == b[k].tobytes(), k
        else:
            assert v == b[k], k


@pytest.mark.parametrize("batch,sims,max_turns", [(16, 64, 12), (24, 64, 12), (3, 200, 10)], ids=["b16", "b24", "b3-s200"])
def test_records_equal_the_oracle_and_the_lane_backup(batch, sims, max_turns, monkeypatch):
    monkeypatch.delenv("AR_BACKUP", raising=False)
    got, stats = _run(batch, sims, max_turns)
    assert stats.total_nn_evals > 0
    ev = HipEvaluator(MLP, 5, 5, max_turns)
    cfg = O.make_config(noise_epsilon=0.0)
    for i in range(N_GAMES):
        want = O.play_game(O.Game(5, 5, max_turns).random_cheese(5, True, i), cfg, sims, batch, 0xA1FA0000 + i, backend=4,
                           net=ev.backend, game_index=i)
        _check_game(got[i], want)
    monkeypatch.setenv("AR_BACKUP", "lane")
    lane, lane_stats = _run(batch, sims, max_turns)
    for i in range(N_GAMES):
        _same_records(got[i], lane[i])
    assert stats.backup_node_visits == lane_stats.backup_node_visits


@pytest.mark.parametrize("batch", [3, 16], ids=["b3", "b16"])
def test_paths_past_the_lds_levels(batch, monkeypatch):
    """c_puct 0.05 makes the search greedy: the tree is a few chains down to the horizon of 40 turns, so paths are far
    longer than the PATH_LDS_STEPS = 12 levels k_backup16 keeps in LDS and their root-side levels, which all sixteen
    entries share, live in scratch. The depth is asserted on the oracle's tree of game 0's first search (same network,
    same constants); game 0 must equal the oracle's game and all games the lane backup's."""
    monkeypatch.delenv("AR_BACKUP", raising=False)
    kw = dict(c_puct=0.05)
    got, stats = _run(batch, 200, 40, **kw)
    ev = HipEvaluator(MLP, 5, 5, 40)
    cfg = O.make_config(noise_epsilon=0.0, **kw)
    game0 = O.Game(5, 5, 40).random_cheese(5, True, 0)
    tree = O.search_once(game0, cfg, 200, batch, seed=0xA1FA0000, backend=4, net=ev.backend)["tree"].dump()
    assert tree[:, 0].max() + 1 > 2 * 12, tree[:, 0].max()  # levels of the deepest path, root included
    _check_game(got[0], O.play_game(game0, cfg, 200, batch, 0xA1FA0000, backend=4, net=ev.backend, game_index=0))
    monkeypatch.setenv("AR_BACKUP", "lane")
    lane, lane_stats = _run(batch, 200, 40, **kw)
    for i in range(N_GAMES):
        _same_records(got[i], lane[i])
    assert stats.backup_node_visits == lane_stats.backup_node_visits
