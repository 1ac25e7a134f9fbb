#!/usr/bin/env python3
"""Speed of validating a checkpoint over one device-resident set of 7x7 self-play games (recorded, not gated; DESIGN.md
section 7).

One attached SmartUniform run fills a row set with at least --positions positions. Reported, as medians of --repeats runs
after a warm-up each, both over every position of the set and on the same device:
  validate_rows_per_s   RowDataset.validate(net): ar_rows_validate, from the stored records to the sums on the host
  today_rows_per_s      what a user of this library does without it: RowDataset.epoch_iter(4096, shuffle=False,
                        augment=False) materialises the observations and targets, an eval-mode PyRatMLP forward written with
                        plain torch ops from the blob's tensors (the formulas of tests/_mlp_np.py, in f32 on the device),
                        F.cross_entropy / F.mse_loss per batch averaged with batch-size weights, every batch's outputs kept
                        and concatenated, and the detailed metrics (top-k accuracy, entropies, explained variance,
                        correlation) over the concatenation
The two sides' losses are printed next to each other as a sanity check, not as a test. Prints one JSON line; --out also
writes it to a file.
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
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def torch_mlp(tensors: dict, device):
    """eval-mode PyRatMLP from the blob's tensors: (Linear, BatchNorm with running statistics, ReLU) twice, three heads"""
    t = {k: torch.from_numpy(np.asarray(v, np.float32)).to(device) for k, v in tensors.items()}

    def block(x, lin, bn):
        x = F.linear(x, t[lin + ".weight"], t[lin + ".bias"])
        x = (x - t[bn + ".running_mean"]) / torch.sqrt(t[bn + ".running_var"] + 1e-5) * t[bn + ".weight"] + t[bn + ".bias"]
        return torch.relu(x)

    def forward(obs):
        x = block(block(obs, "trunk.0", "trunk.1"), "trunk.4", "trunk.5")
        v = F.softplus(F.linear(x, t["value_head.weight"], t["value_head.bias"]))
        return (F.linear(x, t["policy_p1_head.weight"], t["policy_p1_head.bias"]),
                F.linear(x, t["policy_p2_head.weight"], t["policy_p2_head.bias"]), v[:, 0], v[:, 1])

    return forward


def detailed(logits, target, pred, y) -> dict:
    """top-k accuracy, entropies, explained variance and correlation of one player over all rows"""
    a = target.argmax(dim=-1, keepdim=True)
    top = logits.topk(2, dim=-1).indices
    logp = F.log_softmax(logits, dim=-1)
    var_y = y.var()
    vc, yc = pred - pred.mean(), y - y.mean()
    den = (vc.pow(2).sum() * yc.pow(2).sum()).sqrt()
    return dict(top1=(top[:, :1] == a).any(-1).float().mean().item(), top2=(top == a).any(-1).float().mean().item(),
                entropy_pred=-(logp.exp() * logp).sum(-1).mean().item(),
                entropy_target=-(target * target.clamp(min=1e-8).log()).sum(-1).mean().item(),
                explained_variance=0.0 if var_y < 1e-8 else max(-1.0, (1.0 - (y - pred).var() / var_y).item()),
                correlation=0.0 if den < 1e-8 else ((vc * yc).sum() / den).item())


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=1_000_000)
    ap.add_argument("--simulations", type=int, default=16)
    ap.add_argument("--max-turns", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--blob", default=str(ROOT / "tests" / "golden" / "nets" / "mlp_7x7_h256.arnet"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from alpharat_amd import shards
    from alpharat_amd.dataset import RowDataset
    from alpharat_amd.nets import Net
    from alpharat_amd.sampling import SelfPlaySession
    from alpharat_amd.weights import read_blob

    arch, w, h, tensors = read_blob(a.blob)
    assert arch == "mlp" and (w, h) == (7, 7), "the torch side of this benchmark is PyRatMLP on 7x7"
    rs = shards.RowSet(7, 7, (a.positions // 12 + 1) * a.max_turns + a.positions)
    t0 = time.perf_counter()
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
    play_secs = time.perf_counter() - t0
    ds = RowDataset(rs)
    net = Net(a.blob)
    device = torch.device("cuda", rs.device_index)
    forward = torch_mlp(tensors, device)

    def median_of(fn):
        """(median seconds per call, the spread (min, max), the last result): every timed window holds enough calls to last
        about half a second, after a warm-up call"""
        fn()  # warm-up
        t = time.perf_counter()
        last = fn()
        inner = max(1, int(0.5 / max(time.perf_counter() - t, 1e-6)) + 1)
        times = []
        for _ in range(a.repeats):
            t = time.perf_counter()
            for _ in range(inner):
                last = fn()
            times.append((time.perf_counter() - t) / inner)
        return statistics.median(times), (min(times), max(times)), last

    def ours():
        return ds.validate(net).metrics()

    def today():
        losses, weights, kept = [], [], []
        with torch.no_grad():
            for b in ds.epoch_iter(a.batch, shuffle=False, augment=False, drop_last=False):
                l1, l2, v1, v2 = forward(b["observation"])
                y1, y2 = b["value_p1"].squeeze(-1), b["value_p2"].squeeze(-1)
                losses.append(torch.stack([F.cross_entropy(l1, b["policy_p1"]), F.cross_entropy(l2, b["policy_p2"]),
                                           F.mse_loss(v1, y1), F.mse_loss(v2, y2)]))
                weights.append(len(y1))
                kept.append((l1, l2, v1, v2, b["policy_p1"], b["policy_p2"], y1, y2))
            wt = torch.tensor(weights, device=device, dtype=torch.float32)
            p1, p2, m1, m2 = ((torch.stack(losses) * wt[:, None]).sum(0) / wt.sum()).tolist()
            cat = [torch.cat([k[i] for k in kept]) for i in range(8)]
            d1, d2 = detailed(cat[0], cat[4], cat[2], cat[6]), detailed(cat[1], cat[5], cat[3], cat[7])
        torch.cuda.synchronize()
        return dict(loss=p1 + p2 + 0.5 * (m1 + m2), loss_p1=p1, loss_p2=p2, loss_value=0.5 * (m1 + m2), p1=d1, p2=d2)

    ours_secs, ours_spread, m = median_of(ours)
    today_secs, today_spread, ref = median_of(today)
    out = dict(board="7x7", net=Path(a.blob).name, games=games, positions=n, play_secs=round(play_secs, 3), repeats=a.repeats,
               validate_secs=round(ours_secs, 5), validate_secs_min_max=[round(x, 5) for x in ours_spread],
               validate_rows_per_s=round(n / ours_secs),
               today_secs=round(today_secs, 5), today_secs_min_max=[round(x, 5) for x in today_spread],
               today_rows_per_s=round(n / today_secs), today_batch=a.batch,
               loss=round(m["loss"], 6), today_loss=round(ref["loss"], 6),
               top1_p1=round(m["p1/top1_accuracy"], 6), today_top1_p1=round(ref["p1"]["top1"], 6),
               ev_p1=round(m["value/p1_explained_variance"], 6), today_ev_p1=round(ref["p1"]["explained_variance"], 6))
    net.close()
    rs.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
