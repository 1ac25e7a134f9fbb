#!/usr/bin/env python3
"""Speed of one training epoch of PyRatCNN over a device-resident set of 7x7 self-play games (recorded, not gated;
DESIGN.md section 7 "Training gradients of PyRatCNN"). tools/bench_train_sym.py for the fourth architecture: the same fill,
plan, windows and clock.

One attached SmartUniform run fills a row set with at least --positions positions. At batch 4096, with C = 64 channels and
B = 3 residual blocks (player_dim 32, hidden_dim 64; random initial weights, tests/_train_cnn_np.py random_cnn), one epoch is
timed two ways, on the same device, from the same initial weights and with the same plan of batches:
  grad_rows_per_s    RowDataset.grad_iter(CNNGradStep) + torch.optim.AdamW.step(): the forward, the losses and the
                     gradients from ar_rows_grad_cnn, straight from the stored records
  today_rows_per_s   what a trainer does without it: RowDataset.epoch_iter materialises the batch, PyRatCNN restated in
                     plain torch ops in training mode (tests/_cnn_train_torch.py; its convolutions are MIOpen's), the
                     losses, backward(), AdamW.step()
The epochs are planned with augment=False, the reference's setting for this architecture (NoAugmentation). --windows timed
windows (one epoch each) after a warm-up epoch, a host clock around a loop that ends in one torch.cuda.synchronize().
--steps N instead runs N steps of this library's side only and prints nothing: the process a kernel trace is taken of.
Prints one JSON line and appends it to --out (profiles/train_cnn_bench.jsonl).

--gpool-last G makes the last block a GPoolResBlock of G gpool_channels and --dropout P trains both sides with dropout P
(configs/train_cnn_7x7.yaml is --gpool-last 32 --dropout 0.1): this library's side is then GPoolCNNGradStep over
ar_rows_grad_cnn_gpool with its seeded masks, today's side tests/_gpool_train_torch.py with torch's own dropout, the line
carries ``gpool_last`` and ``dropout`` and --out defaults to profiles/train_gpool_bench.jsonl. Without either flag the run, the classes and the line are what they were.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch  # before anything loads libalpharat_hip

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=32_768)
    ap.add_argument("--simulations", type=int, default=16)
    ap.add_argument("--max-turns", type=int, default=50)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--steps", type=int, default=0, help="run this many steps of the library's side and stop (for a kernel trace)")
    ap.add_argument("--gpool-last", type=int, default=0, help="gpool_channels of the last block (0: a ResBlock)")
    ap.add_argument("--dropout", type=float, default=0.0)
    ap.add_argument("--out", default=None, help="the record the line is appended to: profiles/train_cnn_bench.jsonl, with "
                    "--gpool-last or --dropout profiles/train_gpool_bench.jsonl")
    a = ap.parse_args()
    if a.out is None:
        a.out = str(ROOT / "profiles" / ("train_gpool_bench.jsonl" if a.gpool_last or a.dropout else "train_cnn_bench.jsonl"))

    import _cnn_train_torch as CT
    import _train_cnn_np as NC
    from alpharat_amd import shards
    from alpharat_amd.dataset import CNNGradStep, RowDataset
    from alpharat_amd.sampling import SelfPlaySession

    w = h = 7
    Ch, PD, HD, B = a.channels, 32, 64, a.blocks
    tensors = NC.random_cnn(w, h, Ch, PD, HD, B, 0, decided=False)
    gpool = bool(a.gpool_last or a.dropout)
    if gpool:
        import _gpool_train_torch as GT
        import _train_gpool_np as NG
        from alpharat_amd.dataset import GPoolCNNGradStep

        trunk = (0,) * (B - 1) + (a.gpool_last,) if B else ()
        tensors = NG.random_gpool_cnn(w, h, Ch, PD, HD, trunk, 0, decided=False)
    rs = shards.RowSet(7, 7, (a.positions // 12 + 1) * a.max_turns + a.positions)
    n, next_index = 0, 0
    while n < a.positions:  # (as tools/bench_rows.py: runs are added until the set is large enough)
        num_games = (a.positions - n) // 12 + 1
        with SelfPlaySession(width=7, height=7, cheese_count=9, max_turns=a.max_turns, num_games=num_games,
                             simulations=a.simulations, batch_size=8, output_dir=None, seed=0, first_game_index=next_index,
                             concurrent_games=16384) as s:
            s.attach_rows(rs)
            s.run_to_end()
        next_index += num_games
        games, n = rs.count()
    ds = RowDataset(rs)
    device = torch.device("cuda", rs.device_index)
    batch = a.batch
    rows = n - n % batch

    if gpool:
        model = GT.GPoolCNN(w, h, Ch, PD, HD, trunk, dropout=a.dropout, sd=tensors).to(device).train()
        step = GPoolCNNGradStep(model, 1.0, 1.0, dropout_seed=0 if a.dropout else None)
    else:
        model = CT.CNN(w, h, Ch, PD, HD, B, sd=tensors).to(device).train()
        step = CNNGradStep(model, 1.0, 1.0)
    opt = torch.optim.AdamW(model.parameters(), lr=a.lr)

    def ours(epoch, limit=0):
        losses = []
        for _, l in ds.grad_iter(step, batch, epoch=epoch, seed=0, augment=False):
            opt.step()
            losses.append(l[5])
            if limit and len(losses) == limit:
                break
        return torch.stack(losses).mean()

    if a.steps:
        ours(0, a.steps)
        torch.cuda.synchronize()
        rs.close()
        return

    def timed(epoch_fn):
        """(seconds of every window, the last epoch's mean loss)"""
        epoch_fn(0)  # warm-up
        torch.cuda.synchronize()
        times, loss = [], None
        for e in range(1, a.windows + 1):
            t = time.perf_counter()
            loss = epoch_fn(e)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t)
        return times, float(loss)

    ours_times, ours_loss = timed(ours)
    # today's path
    p = {k: torch.tensor(np.asarray(tensors[k], np.float32), device=device, requires_grad=True) for k in step.params}
    running = {k: torch.tensor(np.asarray(tensors[k], np.float32), device=device) for k in step.running}
    opt2 = torch.optim.AdamW(list(p.values()), lr=a.lr)

    def today(epoch):
        losses = []
        for b in ds.epoch_iter(batch, epoch=epoch, seed=0, augment=False):
            opt2.zero_grad(set_to_none=True)
            logits = (GT.forward(p, b["observation"], w, h, running, dropout=a.dropout) if gpool
                      else CT.forward(p, b["observation"], w, h, running))
            ls = CT.losses(logits, b["policy_p1"], b["policy_p2"], b["value_p1"], b["value_p2"], 1.0, 1.0)
            ls["loss"].backward()
            opt2.step()
            losses.append(ls["loss"].detach())
        return torch.stack(losses).mean()

    today_times, today_loss = timed(today)
    rs.close()
    more = dict(gpool_last=a.gpool_last, dropout=a.dropout) if gpool else {}
    line = json.dumps(dict(board="7x7", channels=Ch, blocks=B, **more, player_dim=PD, hidden_dim=HD, games=games, positions=n, batch=batch,
                           rows=rows, windows=a.windows, optimizer=f"AdamW(lr={a.lr})", augment=False,
                           grad_secs=round(statistics.median(ours_times), 5),
                           grad_secs_min_max=[round(min(ours_times), 5), round(max(ours_times), 5)],
                           grad_rows_per_s=round(rows / statistics.median(ours_times)),
                           today_secs=round(statistics.median(today_times), 5),
                           today_secs_min_max=[round(min(today_times), 5), round(max(today_times), 5)],
                           today_rows_per_s=round(rows / statistics.median(today_times)),
                           last_epoch_loss=round(ours_loss, 6), today_last_epoch_loss=round(today_loss, 6)))
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
