#!/usr/bin/env python3
"""Speed of training batches built on the device (recorded, not gated).

One attached SmartUniform run fills a row set with at least --positions 7x7 positions. For each batch size, one epoch is
timed both ways on the same device, as medians of --repeats epochs after a warm-up epoch each, a host clock around work that
ends in a device synchronise:
  rows (this project)   RowDataset.epoch_iter: the epoch's order and swap mask uploaded once, one k_rows_batch per batch into
                        fresh tensors; `kernel_ms` is the HIP-event time around the launches of one whole-epoch request
                        into preallocated tensors (nothing but k_rows_batch runs between the two events)
  tensors (restated)    what the reference's trainer does (alpharat/nn/training/loop.py:165-260, nn/augmentation.py:86-184),
                        restated in torch: the eight row tensors resident, per batch an index gather with a slice of a
                        device randperm, `torch.rand(n) < p_swap`, a clone of the observation and a chain of torch.where.
                        It is NOT the reference's code, which is decorated with torch.compile; this runs eagerly.
Both produce every whole batch of the epoch and drop the remainder. Bytes resident per position are sizeof(PosRec) plus the
per-position share of the per-game arrays for the row set, and the row's tensor bytes for the other.
Prints one JSON line; --out also writes it to a file.
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

W = H = 7
# sizeof(PosRec<NW>) (alpharat_amd/csrc/dev_search.h) by cheese words: boards of up to 64 cells, larger ones
# (tests/test_batches_logic_cpu.py holds them against the header)
POSREC_BYTES = {1: 176, 4: 200}


def swap_batch_torch(batch: dict, mask, w: int, h: int) -> dict:
    """augmentation.py:86-184 restated: a clone of the observation with the swapped columns, then torch.where per array"""
    import torch

    hw = w * h
    m2, m3 = mask.unsqueeze(-1), mask.unsqueeze(-1).unsqueeze(-1)
    obs = batch["observation"]
    sw = obs.clone()
    sw[:, hw * 4:hw * 5] = obs[:, hw * 5:hw * 6]
    sw[:, hw * 5:hw * 6] = obs[:, hw * 4:hw * 5]
    s = hw * 7
    sw[:, s] = -obs[:, s]
    sw[:, s + 2], sw[:, s + 3] = obs[:, s + 3], obs[:, s + 2]
    sw[:, s + 4], sw[:, s + 5] = obs[:, s + 5], obs[:, s + 4]
    out = {"observation": torch.where(m2, sw, obs)}
    for k in ("policy", "action", "value"):
        a, b = batch[f"{k}_p1"], batch[f"{k}_p2"]
        out[f"{k}_p1"], out[f"{k}_p2"] = torch.where(m2, b, a), torch.where(m2, a, b)
    co = batch["cheese_outcomes"]
    sc = torch.where(co == 0, torch.tensor(3, device=co.device, dtype=co.dtype), co)
    sc = torch.where(co == 3, torch.tensor(0, device=co.device, dtype=co.dtype), sc)
    out["cheese_outcomes"] = torch.where(m3, sc, co)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=500_000)
    ap.add_argument("--simulations", type=int, default=64)
    ap.add_argument("--max-turns", type=int, default=50)
    ap.add_argument("--batch-sizes", default="256,4096,65536")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from alpharat_amd import shards
    from alpharat_amd.dataset import RowDataset
    from alpharat_amd.sampling import SelfPlaySession

    if not torch.cuda.is_available():
        raise SystemExit("bench_batches needs the GPU: nothing here is measured without one")

    rs = shards.RowSet(W, H, (a.positions // 12 + 1) * a.max_turns + a.positions)
    t0 = time.perf_counter()
    n, next_index = 0, 0
    while n < a.positions:  # as tools/bench_rows.py: runs are added until the set is large enough
        num_games = (a.positions - n) // 12 + 1
        with SelfPlaySession(width=W, height=H, cheese_count=9, max_turns=a.max_turns, num_games=num_games,
                             simulations=a.simulations, batch_size=8, output_dir=None, seed=0, first_game_index=next_index,
                             concurrent_games=16384) as s:
            s.attach_rows(rs)
            s.run_to_end()
        next_index += num_games
        games, n = rs.count()
    play_secs = time.perf_counter() - t0
    ds = RowDataset(rs)
    device = torch.device("cuda", rs.device_index)

    def median_epoch(epoch_fn):
        epoch_fn(0)  # warm-up: code objects, the caching allocator's blocks of this batch size
        torch.cuda.synchronize()
        times = []
        for e in range(1, a.repeats + 1):
            t = time.perf_counter()
            epoch_fn(e)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t)
        return statistics.median(times), min(times), max(times)

    # the other side: the rows as resident tensors, in GPUDataset's shapes
    plain = next(ds.epoch_iter(n, augment=False, shuffle=False, drop_last=False))
    torch.cuda.synchronize()
    tensor_bytes = sum(t.numel() * t.element_size() for t in plain.values()) / n

    # the kernel alone: one request for the whole epoch into preallocated tensors, HIP events around it
    order = np.random.default_rng(0).permutation(n)
    mask = np.random.default_rng(1).random(n) < 0.5
    rs.set_order(ds.positions[order], mask[order])
    out = {k: torch.empty_like(t) for k, t in plain.items()}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kernel_ms = []
    for i in range(a.repeats + 1):
        ev0.record()
        rs.build_into(0, n, out)
        ev1.record()
        ev1.synchronize()
        if i:
            kernel_ms.append(ev0.elapsed_time(ev1))
    del out
    row_bytes = int(tensor_bytes)

    results = []
    for bs in [int(x) for x in a.batch_sizes.split(",")]:
        n_batches = n // bs

        def ours(epoch):
            for batch in ds.epoch_iter(bs, epoch=epoch, seed=0):
                pass

        def restated(epoch):
            index = torch.randperm(n, device=device)
            for b in range(n_batches):
                idx = index[b * bs:(b + 1) * bs]
                batch = {k: t[idx] for k, t in plain.items()}
                batch = swap_batch_torch(batch, torch.rand(bs, device=device) < 0.5, W, H)

        o_med, o_min, o_max = median_epoch(ours)
        r_med, r_min, r_max = median_epoch(restated)
        rows = n_batches * bs
        results.append(dict(batch_size=bs, batches=n_batches, rows=rows,
                            rows_secs=round(o_med, 5), rows_secs_min_max=[round(o_min, 5), round(o_max, 5)],
                            rows_per_s=round(rows / o_med),
                            tensors_secs=round(r_med, 5), tensors_secs_min_max=[round(r_min, 5), round(r_max, 5)],
                            tensors_rows_per_s=round(rows / r_med)))

    gi, fr, nr = rs.games()
    per_game = 32 + W * H * 4 + W * H  # RowGame header, maze bytes, cheese outcomes
    set_bytes = POSREC_BYTES[1 if W * H <= 64 else 4] + 4 + per_game * len(gi) / n  # + the game number of every position
    k_ms = statistics.median(kernel_ms)
    rs.close()
    res = dict(board="7x7", games=int(games), positions=int(n), play_secs=round(play_secs, 3), repeats=a.repeats,
               kernel_ms_whole_epoch=round(k_ms, 3), kernel_ms_min_max=[round(min(kernel_ms), 3), round(max(kernel_ms), 3)],
               kernel_rows_per_s=round(n / (k_ms / 1000.0)), row_bytes=row_bytes,
               kernel_write_gb_per_s=round(n * row_bytes / (k_ms / 1000.0) / 1e9, 1),
               resident_bytes_per_position=dict(row_set=round(set_bytes, 1), row_tensors=round(tensor_bytes, 1)),
               epochs=results,
               note="tensors = the reference trainer's gather + clone + torch.where restated in eager torch on the same "
                    "device, not its code")
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
