#!/usr/bin/env python3
"""Speed of one training epoch of SymmetricMLP over a device-resident set of 7x7 self-play games (recorded, not gated;
DESIGN.md section 7 "Training gradients of SymmetricMLP"). tools/bench_train.py for the second architecture: the same fill,
plan, windows and clock.

One attached SmartUniform run fills a row set with at least --positions positions, as tools/bench_validate.py fills its
own. At batch sizes 256, 4096 and 65536 one epoch is timed two ways, on the same device, from the same initial weights
(the blob's) and with the same plan of batches:
  grad_rows_per_s    RowDataset.grad_iter(SymmetricGradStep) + torch.optim.AdamW.step(): the forward, the losses and the
                     gradients from ar_rows_grad_symmetric, straight from the stored records
  today_rows_per_s   what a trainer does without it: RowDataset.epoch_iter materialises the batch, SymmetricMLP restated
                     in plain torch ops in training mode (tests/_sym_torch.py), the losses, backward(), AdamW.step()
The epochs are planned with augment=False, the reference's setting for this architecture (NoAugmentation).
Five timed windows (one epoch each, epochs 1 .. 5) after a warm-up epoch, a host clock around a loop that ends in one
torch.cuda.synchronize(). The mean loss of the last epoch of both sides is printed as a sanity check, not as a test: the
two sides round differently, and AdamW amplifies that. --dropout P as in tools/bench_train.py: both sides train with
dropout, each with its own masks. Prints one JSON line and writes it to --out (profiles/train_sym_bench.json).
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

BATCHES = (256, 4096, 65536)
WINDOWS = 5


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=262_144)
    ap.add_argument("--simulations", type=int, default=16)
    ap.add_argument("--max-turns", type=int, default=50)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--blob", default=str(ROOT / "tests" / "golden" / "nets" / "symmetric_7x7_h256.arnet"))
    ap.add_argument("--out", default=str(ROOT / "profiles" / "train_sym_bench.json"))
    ap.add_argument("--dropout", type=float, default=0.0,
                    help="both sides train with dropout P: the step with dropout_seed 0, the torch side a model built with nn.Dropout(P)")
    a = ap.parse_args()

    import _sym_torch as ST
    from alpharat_amd import shards
    from alpharat_amd.dataset import RowDataset, SymmetricGradStep
    from alpharat_amd.sampling import SelfPlaySession
    from alpharat_amd.weights import read_blob

    arch, w, h, tensors = read_blob(a.blob)
    assert arch == "symmetric" and (w, h) == (7, 7), "this benchmark is SymmetricMLP on 7x7"
    H = tensors["trunk.4.weight"].shape[0]
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

    def timed(epoch_fn):
        """(seconds of every window, the last epoch's mean loss)"""
        epoch_fn(0)  # warm-up
        torch.cuda.synchronize()
        times, loss = [], None
        for e in range(1, WINDOWS + 1):
            t = time.perf_counter()
            loss = epoch_fn(e)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t)
        return times, float(loss)

    results = []
    for batch in BATCHES:
        if batch > n:
            continue
        rows = n - n % batch
        # this library
        model = ST.Symmetric(w, h, H, a.dropout, sd=tensors).to(device).train()
        step = SymmetricGradStep(model, 1.0, 1.0, dropout_seed=0 if a.dropout else None)
        opt = torch.optim.AdamW(model.parameters(), lr=a.lr)

        def ours(epoch):
            losses = []
            for _, l in ds.grad_iter(step, batch, epoch=epoch, seed=0, augment=False):
                opt.step()
                losses.append(l[5])
            return torch.stack(losses).mean()

        ours_times, ours_loss = timed(ours)
        # today's path
        p = {k: torch.tensor(np.asarray(tensors[k], np.float32), device=device, requires_grad=True) for k in step.params}
        running = {k: torch.tensor(np.asarray(tensors[k], np.float32), device=device) for k in step.running}
        opt2 = torch.optim.AdamW(list(p.values()), lr=a.lr)
        forward = lambda x: ST.forward(p, x, w, h, running)  # noqa: E731
        if a.dropout:  # the modules themselves, nn.Dropout(P) among them: torch's own masks
            tm = ST.Symmetric(w, h, H, a.dropout, sd=tensors).to(device).train()
            opt2 = torch.optim.AdamW(tm.parameters(), lr=a.lr)

            def forward(x):  # alpharat/nn/models/symmetric.py forward, module by module
                hw = w * h
                sc = x[:, 7 * hw:]
                shared = tm.shared_encoder(torch.cat([x[:, :4 * hw], x[:, 6 * hw:7 * hw], sc[:, 1:2]], dim=1))
                pe = [tm.player_encoder(torch.cat([x[:, (4 + i) * hw:(5 + i) * hw], sc[:, 2 + i:3 + i], sc[:, 4 + i:5 + i]], dim=1))
                      for i in (0, 1)]
                hs = [tm.trunk(torch.cat([shared, pe[i]], dim=1)) for i in (0, 1)]
                cat = [torch.cat([hs[i], hs[0] + hs[1]], dim=1) for i in (0, 1)]
                v = [torch.nn.functional.softplus(tm.value_head(c)).squeeze(-1) for c in cat]
                return tm.policy_head(cat[0]), tm.policy_head(cat[1]), v[0], v[1]

        def today(epoch):
            losses = []
            for b in ds.epoch_iter(batch, epoch=epoch, seed=0, augment=False):
                opt2.zero_grad(set_to_none=True)
                ls = ST.losses(forward(b["observation"]), b["policy_p1"], b["policy_p2"], b["value_p1"],
                               b["value_p2"], 1.0, 1.0)
                ls["loss"].backward()
                opt2.step()
                losses.append(ls["loss"].detach())
            return torch.stack(losses).mean()

        today_times, today_loss = timed(today)
        results.append(dict(batch=batch, rows=rows, grad_secs=round(statistics.median(ours_times), 5),
                            grad_secs_min_max=[round(min(ours_times), 5), round(max(ours_times), 5)],
                            grad_rows_per_s=round(rows / statistics.median(ours_times)),
                            today_secs=round(statistics.median(today_times), 5),
                            today_secs_min_max=[round(min(today_times), 5), round(max(today_times), 5)],
                            today_rows_per_s=round(rows / statistics.median(today_times)),
                            last_epoch_loss=round(ours_loss, 6), today_last_epoch_loss=round(today_loss, 6)))
        print(json.dumps(results[-1]), file=sys.stderr)
    rs.close()
    line = json.dumps(dict(board="7x7", net=Path(a.blob).name, hidden=int(H), games=games, positions=n, windows=WINDOWS,
                           optimizer=f"AdamW(lr={a.lr})", augment=False, dropout=a.dropout, results=results))
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
