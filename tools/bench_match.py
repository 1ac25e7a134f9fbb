"""Device-resident match against the host loop it replaces, in one process: games/s of `play_match` and of a loop that
plays the same games with two `HipSearcher.search_batch` calls per move while the host samples the actions and steps
the games (what alpharat/eval/game.py:47-87 does around SearcherAgent.get_move, batched over the games).

Workload (defaults): 7x7 open, 21 cheese, the mlp_7x7_h256 golden network on both sides, 400 simulations, batch 16,
4096 games on 4096 resident. The two runs alternate, `--repeats` times after one untimed warm-up of each (the first
run pays for the one-time allocation of the tree region); medians are reported and written to `--out`.

    python tools/bench_match.py --out profiles/match_vs_host_loop.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def device_match(args, blob, seed):
    from alpharat_amd.match import MatchAgent, play_match

    kw = dict(checkpoint=blob, simulations=args.simulations, batch_size=args.batch_size)
    t0 = time.perf_counter()
    res = play_match(MatchAgent("a", seed=0xA0000 + seed, **kw), MatchAgent("b", seed=0xB0000 + seed, **kw),
                     width=args.width, height=args.height, cheese_count=args.cheese, max_turns=args.max_turns,
                     num_games=args.games, swap_sides=True, seed=seed, concurrent_games=args.games)
    dt = time.perf_counter() - t0
    return dict(secs=dt, games=res.total_games, positions=res.total_positions, games_per_s=res.total_games / dt)


def host_loop(args, blob, seed):
    """The same games: per move one search_batch per agent over the games still running, then the host samples and steps."""
    from alpharat_amd import _lib
    from alpharat_amd.game import PyRat
    from alpharat_amd.nets import Net
    from alpharat_amd.searcher import HipSearcher

    L = _lib.load()
    net = Net(blob)
    sa = HipSearcher(args.simulations, batch_size=args.batch_size, net=net)
    sb = HipSearcher(args.simulations, batch_size=args.batch_size, net=net)
    rng = np.random.default_rng(seed)
    hw = args.width * args.height
    t0 = time.perf_counter()
    games = []
    for i in range(args.games):
        cheese = np.zeros(hw, np.uint8)
        _lib.check(L.ar_generate_cheese(args.width, args.height, 0, hw - 1, args.cheese, 1, seed + i,
                                        cheese.ctypes.data_as(_lib.C.c_void_p)))
        cells = [(int(c) % args.width, int(c) // args.width) for c in np.flatnonzero(cheese)]
        games.append(PyRat.create_custom(args.width, args.height, cheese=cells, max_turns=args.max_turns))
    live = list(range(args.games))
    positions = 0
    while live:
        gs = [games[i] for i in live]
        ra = sa.search_batch(gs, seeds=[int(s) for s in rng.integers(0, 2**31, len(gs))])
        rb = sb.search_batch(gs, seeds=[int(s) for s in rng.integers(0, 2**31, len(gs))])
        nxt = []
        for k, i in enumerate(live):
            a_is_p1 = i % 2 == 0
            r1, r2 = (ra[k], rb[k]) if a_is_p1 else (rb[k], ra[k])
            games[i].make_move(int(rng.choice(5, p=r1.policy_p1)), int(rng.choice(5, p=r2.policy_p2)))
            positions += 1
            if not games[i].is_over():
                nxt.append(i)
        live = nxt
    dt = time.perf_counter() - t0
    net.close()
    return dict(secs=dt, games=args.games, positions=positions, games_per_s=args.games / dt)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=7)
    ap.add_argument("--height", type=int, default=7)
    ap.add_argument("--cheese", type=int, default=21)
    ap.add_argument("--max-turns", type=int, default=100)
    ap.add_argument("--simulations", type=int, default=400)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--net", default=str(ROOT / "tests" / "golden" / "nets" / "mlp_7x7_h256.arnet"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    device_match(args, args.net, 1000)  # warm-up of both, untimed: tree region, code objects, pinned buffers
    host_loop(args, args.net, 1000)
    runs = {"device_match": [], "host_loop": []}
    for r in range(args.repeats):  # alternate, so drift hits both alike
        runs["device_match"].append(device_match(args, args.net, r * args.games))
        runs["host_loop"].append(host_loop(args, args.net, r * args.games))
        print(json.dumps({k: v[-1] for k, v in runs.items()}), flush=True)
    med = {k: statistics.median(x["games_per_s"] for x in v) for k, v in runs.items()}
    out = dict(workload={k: getattr(args, k) for k in ("width", "height", "cheese", "max_turns", "simulations", "batch_size",
                                                       "games", "repeats")},
               net=Path(args.net).name, games_per_s_device_match=med["device_match"], games_per_s_host_loop=med["host_loop"],
               ratio=med["device_match"] / med["host_loop"], runs=runs)
    print(json.dumps({k: out[k] for k in ("games_per_s_device_match", "games_per_s_host_loop", "ratio")}))
    if args.out:
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
