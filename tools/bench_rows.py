#!/usr/bin/env python3
"""Speed of the training-row path on one set of 7x7 self-play games (recorded, not gated).

One attached SmartUniform run fills a row set with at least --positions positions. Reported, as medians of --repeats runs
after a warm-up each:
  build_rows_per_s       ar_rows_build of every position in shuffled order, with its copy to host arrays
  build_kernel_ms        the time inside k_rows_build of that call (HIP events around the launches)
  shards_rows_per_s      the whole prepare_training_set_with_split (stored shards, default sizes) into a scratch directory
  restatement_rows_per_s the per-position loop of tests/_rows_np.py over the same run's records on this host
The last figure stands in for the reference's procedure (alpharat/data/sharding.py:566-579 is a per-position Python loop of
the same shape); it is NOT the reference's own code, which needs a newer Python than this project runs on. It is timed on a
sample of the games (--loop-positions) and reported as a rate.
Prints one JSON line; --out also writes it to a file.
"""
from __future__ import annotations

import argparse
import json
import shutil
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=500_000)
    ap.add_argument("--simulations", type=int, default=64)
    ap.add_argument("--max-turns", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-positions", type=int, default=40_000)
    ap.add_argument("--scratch", default=None, help="directory for the shards (default: a temporary one)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import _rows_np as R
    from alpharat_amd import shards
    from alpharat_amd.sampling import SelfPlaySession

    # Runs are added until the set is large enough: each plays the games still needed at 12 positions per game (these
    # settings give ~17), with game indices that continue. Capacity covers the first run at max_turns positions per game.
    sample: list = []
    kept = [0]

    def on_game(g):
        sample.append(g)
        kept[0] += g["n"]

    rs = shards.RowSet(7, 7, (a.positions // 12 + 1) * a.max_turns + a.positions)
    t0 = time.perf_counter()
    games, n, next_index = 0, 0, 0
    while n < a.positions:
        num_games = (a.positions - n) // 12 + 1
        with SelfPlaySession(width=7, height=7, cheese_count=9, max_turns=a.max_turns, num_games=num_games,
                             simulations=a.simulations, batch_size=8, output_dir=None, seed=0, first_game_index=next_index,
                             concurrent_games=16384, on_game=on_game,
                             record_filter=lambda i: kept[0] < a.loop_positions) as s:
            s.attach_rows(rs)
            s.run_to_end()
        next_index += num_games
        games, n = rs.count()
    play_secs = time.perf_counter() - t0
    order = np.random.default_rng(0).permutation(n).astype(np.uint64)

    def median_of(fn):
        fn()  # warm-up
        times, extra = [], []
        for _ in range(a.repeats):
            t = time.perf_counter()
            extra.append(fn())
            times.append(time.perf_counter() - t)
        return statistics.median(times), extra

    def build():
        rs.build(order)
        return rs.build_kernel_ms()

    build_secs, kernel_ms = median_of(build)

    scratch = Path(a.scratch) if a.scratch else Path(tempfile.mkdtemp(prefix="bench_rows_"))
    scratch.mkdir(parents=True, exist_ok=True)

    def write():
        res = shards.prepare_training_set_with_split(None, scratch, val_ratio=0.1, positions_per_shard=10000, seed=42, rowset=rs)
        assert res.total_positions == n
        shutil.rmtree(res.shard_dir)

    try:
        shard_secs, _ = median_of(write)
    finally:
        if not a.scratch:
            shutil.rmtree(scratch, ignore_errors=True)

    loop_n = sum(g["n"] for g in sample)
    R.stack_rows(sample[:8])  # warm-up
    t = time.perf_counter()
    R.stack_rows(sample)
    loop_secs = time.perf_counter() - t
    rs.close()

    out = dict(board="7x7", games=games, positions=n, play_secs=round(play_secs, 3), repeats=a.repeats,
               build_secs=round(build_secs, 4), build_rows_per_s=round(n / build_secs),
               build_kernel_ms=round(statistics.median(kernel_ms), 3),
               build_kernel_rows_per_s=round(n / (statistics.median(kernel_ms) / 1000.0)),
               shards_secs=round(shard_secs, 3), shards_rows_per_s=round(n / shard_secs),
               restatement_positions=loop_n, restatement_secs=round(loop_secs, 3),
               restatement_rows_per_s=round(loop_n / loop_secs),
               note="restatement = tests/_rows_np.py per-position loop, a stand-in for the reference's sharding loop, not its code")
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
