"""-m gpu: the configuration bench.py times -- BASELINE config 3 with as many resident games as the device holds
(131072 on an MI355X), the default groups of games, the work-queue gather with its pass limit (gathers parked and
resumed), trees moving between runs of pages, zones of the tree region filling up -- against the CPU oracle at record
level, plus the size-independent properties on everything that finished. The other parity tests run at <= 64 resident
games, where none of that machinery is under load (the reference's harness and its tests run the same code,
bench_selfplay.rs:215-270 -> run_self_play, selfplay.rs:515-598).

And the close -> reopen path at scale: a session of two groups, closed, then a session of one group and another size in
the same process (the cached tree region is handed over), a game of each against the oracle."""
import os
import time
from pathlib import Path

import numpy as np
import pytest

import _oracle as O
from test_gpu_pipeline_parity import GOLD, TUNED, HipEvaluator, _check_game, _note

pytestmark = pytest.mark.gpu
GAME = dict(width=7, height=7, cheese_count=10, max_turns=50)


def _oracle_game(ev, cfg, index):
    return O.play_game(O.Game(7, 7, 50).random_cheese(10, True, index), cfg, 1897, 16, 0xA1FA0000 + index, backend=4,
                       net=ev.backend, game_index=index)


class _Sink:
    """keeps the records of chosen games, checks the cheap properties on all of them"""

    def __init__(self, keep):
        self.keep = set(keep)
        self.games = {}
        self.seen = 0
        self.bad = dict(policy=0, action=0, cheese=0)
        self.positions = 0

    def __call__(self, g):
        self.seen += 1
        self.positions += g["n"]
        s1, s2 = g["policy_p1"].sum(axis=1), g["policy_p2"].sum(axis=1)
        self.bad["policy"] += int((np.abs(s1 - 1) > 1e-5).sum() + (np.abs(s2 - 1) > 1e-5).sum())
        idx = np.arange(g["n"])
        self.bad["action"] += int((g["policy_p1"][idx, g["action_p1"]] <= 0).sum() + (g["policy_p2"][idx, g["action_p2"]] <= 0).sum())
        collected = (g["cheese_outcomes"] != 2).sum()
        self.bad["cheese"] += int(abs(collected - (g["final_p1_score"] + g["final_p2_score"])) > 1e-6)
        if g["game_index"] in self.keep:
            self.games[g["game_index"]] = g


def test_selfplay_at_the_timed_configuration_vs_oracle():
    from alpharat_amd.sampling import UNBOUNDED, SelfPlaySession

    want_resident = 131072
    blob = GOLD / "mlp_7x7_h256.arnet"
    t0 = time.perf_counter()
    # the first generation's game indices run over the slots the library filled at once (zone by zone, as many per zone as
    # its admission rule allows): the first and the last of them, both sides of the middle (the group boundary), a few more
    sink = _Sink(())
    with SelfPlaySession(**GAME, num_games=UNBOUNDED, simulations=1897, batch_size=16, output_dir=None, weights_path=str(blob),
                         seed=0, concurrent_games=want_resident, on_game=sink, **TUNED) as s:
        info = s.info()
        S = info["resident_games"]
        n0 = S - info["idle_slots"]
        assert S >= 65536 and n0 >= 32768, info  # (an MI355X holds 131072 slots; anything smaller means the sizing went wrong)
        # the library's default: two groups when the process was given a hardware queue per stream, else one
        queues = int(os.environ.get("GPU_MAX_HW_QUEUES") or 0)  # (unset: the runtime's default, fewer than eight)
        default_groups = 2 if queues >= 8 else 1
        assert info["gather_kind"] == 2 and info["groups"] == default_groups and info["gather_pass_limit"] < 1000, info
        sink.keep = {0, 1, n0 // 3, n0 // 2 - 1, n0 // 2, 2 * n0 // 3, n0 - 2, n0 - 1}
        steps = 0
        while len(sink.games) < len(sink.keep) and steps < 12000:
            s.step(512)
            steps += 512
        end = s.info()
    _note(f"bench scale: {S} slots, {n0} filled at once, {end['idle_slots']} idle at the end, {end['tree_pages_per_game']:.1f} pages "
          f"per game, {steps} batch steps, {sink.seen} games finished, {time.perf_counter() - t0:.1f} s")
    assert len(sink.games) == len(sink.keep), (sorted(sink.games), sorted(sink.keep))
    assert sink.seen > n0 // 4 and sink.bad == dict(policy=0, action=0, cheese=0), (sink.seen, sink.bad)
    ev = HipEvaluator(blob, 7, 7, 50)
    cfg = O.make_config(**TUNED)
    for i in sorted(sink.keep):
        t1 = time.perf_counter()
        _check_game(sink.games[i], _oracle_game(ev, cfg, i))
        _note(f"bench scale: oracle game {i}: {time.perf_counter() - t1:.1f} s")


def test_two_sessions_of_different_shape_in_one_process(monkeypatch):
    """A two-group session, closed; then a one-group session of another resident size in the same process, which takes over
    the tree region the first one left cached: streams, events, group count, page bitmaps, the evaluator's maze binding are
    all set up a second time. One game of each session against the oracle."""
    from alpharat_amd.sampling import UNBOUNDED, SelfPlaySession

    blob = GOLD / "mlp_7x7_h256.arnet"
    ev = HipEvaluator(blob, 7, 7, 50)
    cfg = O.make_config(**TUNED)
    # (the group count is set: the library's default depends on the hardware queues the process was given)
    for resident, groups, first in ((16384, 2, 0), (12288, 1, 1 << 20), (20480, 2, 2 << 20)):
        monkeypatch.setenv("AR_GROUPS", str(groups))
        sink = _Sink({first, first + resident - 1})
        with SelfPlaySession(**GAME, num_games=UNBOUNDED, simulations=1897, batch_size=16, output_dir=None, weights_path=str(blob),
                             seed=0, first_game_index=first, concurrent_games=resident, on_game=sink, **TUNED) as s:
            info = s.info()
            assert info["resident_games"] == resident and info["idle_slots"] == 0 and info["groups"] == groups, info
            steps = 0
            while len(sink.games) < 2 and steps < 12000:
                s.step(512)
                steps += 512
        assert len(sink.games) == 2 and sink.bad == dict(policy=0, action=0, cheese=0)
        _check_game(sink.games[first], _oracle_game(ev, cfg, first))
    monkeypatch.delenv("AR_GROUPS", raising=False)
