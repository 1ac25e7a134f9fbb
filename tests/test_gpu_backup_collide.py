"""-m gpu: k_backup16's collision cancel (dev_backup16.h: a collision record's count goes to the lane whose entry has the
record's node as its leaf and is taken off each ancestor while phase 2 has it in registers; nothing walks up) through
whole games: 5x5, 64 resident games, PyRatMLP h32, no root noise, so every batch goes through k_backup16. Every record of
every game against the oracle (its leaves evaluated by the same device network) and against the same run with the
lane-per-game backup, which keeps the atomic-free walk of backup_machine, byte for byte; equal backup_node_visits.

The cases: batch 16 with a fixed collision budget of 48 (more than sixteen records in a batch: a lane folds two and
more, one full chunk), batch 24 with the same budget (a leaf and the records on it in different chunks), batch 3 over
200 simulations with a budget of 8 (one short chunk, many picks).

That the first two settings really give batches with more than sixteen collision records was checked on the CPU with
the oracle before this file was written: a scratch copy of oracle/mcts.hpp whose simulate_batch prints the length of
all_collisions, built as the oracle's library and driven through tests/_oracle.py's play_game with the oracle's own
PyRatMLP forward (backend 2), games 0 to 7 of each setting. Batch 16: 443 batches, 9.8 records a batch, 48 at most, 94
batches (21 %) with more than sixteen records and 30 with more than thirty-two. Batch 24: 345 batches, 14.3 records a
batch, 45 at most, 134 (39 %) with more than sixteen, 46 with more than thirty-two. Batch 3: 5037 batches, 0.14 records
a batch, 8 at most."""
from pathlib import Path

import pytest

import _oracle as O
from test_gpu_backup_merge import _run, _same_records
from test_gpu_parity import _check_game
from test_gpu_pipeline_parity import HipEvaluator

pytestmark = pytest.mark.gpu

MLP = Path(__file__).parent / "golden" / "nets" / "mlp_5x5_h32.arnet"
N_GAMES = 64
MAX_TURNS = 12


def _budget(n):
    return dict(collision_limit_min=n, collision_limit_max=n)


@pytest.mark.parametrize("batch,sims,budget", [(16, 64, 48), (24, 64, 48), (3, 200, 8)], ids=["b16-c48", "b24-c48", "b3-s200-c8"])
def test_records_equal_the_oracle_and_the_lane_backup(batch, sims, budget, monkeypatch):
    monkeypatch.delenv("AR_BACKUP", raising=False)
    coll = _budget(budget)
    got, stats = _run(batch, sims, MAX_TURNS, **coll)
    assert stats.total_nn_evals > 0 and stats.total_collisions > 0
    ev = HipEvaluator(MLP, 5, 5, MAX_TURNS)
    cfg = O.make_config(noise_epsilon=0.0, **coll)
    for i in range(N_GAMES):
        want = O.play_game(O.Game(5, 5, MAX_TURNS).random_cheese(5, True, i), cfg, sims, batch, 0xA1FA0000 + i, backend=4,
                           net=ev.backend, game_index=i)
        _check_game(got[i], want)
    monkeypatch.setenv("AR_BACKUP", "lane")
    lane, lane_stats = _run(batch, sims, MAX_TURNS, **coll)
    for i in range(N_GAMES):
        _same_records(got[i], lane[i])
    assert stats.backup_node_visits == lane_stats.backup_node_visits
    assert stats.total_collisions == lane_stats.total_collisions
