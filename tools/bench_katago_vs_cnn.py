#!/usr/bin/env python3
"""KataGoCNN against PyRatCNN on bench.py's `cnn` workload, in one process, sessions alternating.

    python tools/bench_katago_vs_cnn.py [--rounds 3] [--warmup 512] [--steps 640] [--resident 16384]

Both nets are c64 res, res, gpool(32) with hidden 64 at 7x7 (tests/golden/nets/cnn_gpool_7x7_c64.arnet, the bench's
`cnn` network, and tests/golden/nets_katago/katago_7x7_c64.arnet, configs/train_cnn_pos_7x7.yaml). Each session is
the bench's steady state: 4096 simulations, batch 16, noise 0.25, an unbounded stream of games over `--resident`
slots; `--warmup` batch steps, then `--steps` timed ones. One JSON line per session, then a summary line with the
median NN evaluations/s of each net and their ratio. Per-launch kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this script (k_cnn_mfma<.., false> is PyRatCNN, <.., true> KataGoCNN)."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

GAME = dict(width=7, height=7, cheese_count=10, max_turns=50)
SEARCH = dict(c_puct=0.512, fpu_reduction=0.459, force_k=0.103, noise_epsilon=0.25, noise_concentration=10.83)
NETS = {"cnn": ROOT / "tests" / "golden" / "nets" / "cnn_gpool_7x7_c64.arnet",
        "katago": ROOT / "tests" / "golden" / "nets_katago" / "katago_7x7_c64.arnet"}


def session(blob: Path, resident: int, warmup: int, steps: int) -> dict:
    from alpharat_amd.sampling import UNBOUNDED, SelfPlaySession

    with SelfPlaySession(**GAME, num_games=UNBOUNDED, simulations=4096, batch_size=16, output_dir=None,
                         weights_path=str(blob), seed=0, concurrent_games=resident, **SEARCH) as s:
        s.step(warmup)
        t0 = time.perf_counter()
        w = s.step(steps)
        dt = time.perf_counter() - t0
    return {"nn_evals_per_sec": w.total_nn_evals / dt, "simulations_per_sec": w.total_simulations / dt,
            "batch_steps": w.steps, "secs": dt}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=3)
    # (a move is 256+ batch steps at 4096 simulations / batch 16, and a window counts the moves it finishes: the warm-up
    # lets the games drift out of step, the timed window spans several moves)
    ap.add_argument("--warmup", type=int, default=512)
    ap.add_argument("--steps", type=int, default=640)
    ap.add_argument("--resident", type=int, default=16384)
    a = ap.parse_args()
    rates = {k: [] for k in NETS}
    for r in range(a.rounds):
        for name in (("cnn", "katago") if r % 2 == 0 else ("katago", "cnn")):
            row = session(NETS[name], a.resident, a.warmup, a.steps)
            rates[name].append(row["nn_evals_per_sec"])
            print(json.dumps({"round": r, "net": name, **row}), flush=True)
    med = {k: statistics.median(v) for k, v in rates.items()}
    print(json.dumps({"summary": "median NN evaluations/s", **med,
                      "katago_over_cnn": med["katago"] / med["cnn"] if med["cnn"] > 0 else None,
                      "rounds": a.rounds, "warmup": a.warmup, "steps": a.steps, "resident": a.resident}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
