#!/usr/bin/env python3
"""Generate the validation-metric fixtures under tests/golden/metrics/ by running the reference's own
`compute_mlp_losses`, `compute_policy_metrics`, `compute_value_metrics` and `GPUMetricsAccumulator` on the CPU (build
container only -- /root/reference does not travel to the GPU box; the files are committed).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_metrics_golden.py

Each file holds the inputs of at most 256 rows -- logits_p1, logits_p2 (n, 5), pred_v1, pred_v2 (n,), policy_p1, policy_p2
(n, 5), value_p1, value_p2 (n,), policy_weight, value_weight -- and what the reference makes of them: `ref_keys` and
`ref_values`, the numbers its loop logs under val/ (alpharat/nn/training/loop.py:306-361). The losses are accumulated as
the loop does, batch by batch with batches of 3, so that a short last batch is included; the detailed metrics are computed
over the concatenation of the batches (loop.py:51-86). The import shims are those of tools/gen_net_golden.py.
"""
from __future__ import annotations

import os
import sys
from pathlib import Path
from types import SimpleNamespace

os.environ["TORCHDYNAMO_DISABLE"] = "1"
sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference")
OUT = ROOT / "tests" / "golden" / "metrics"
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

BATCH = 3
INPUTS = ("logits_p1", "logits_p2", "pred_v1", "pred_v2", "policy_p1", "policy_p2", "value_p1", "value_p2")


def _policies(rng, n):
    import numpy as np

    return rng.dirichlet(np.full(5, 0.6), size=n).astype(np.float32)


def _tied_policies(rng, n):
    """visit-proportional policies from a handful of visits: most rows have two or more equal largest entries"""
    import numpy as np

    out = np.zeros((n, 5), np.float32)
    for i in range(n):
        top = rng.choice(5, size=int(rng.integers(2, 4)), replace=False)
        counts = np.zeros(5)
        counts[top] = 3
        rest = [k for k in range(5) if k not in top]
        counts[rng.choice(rest)] += int(rng.integers(0, 3))
        out[i] = (counts / counts.sum()).astype(np.float32)
    return out


def cases() -> dict:
    import numpy as np

    import _rows as T
    import _rows_np as R

    rng = np.random.default_rng(2025)
    out = {}

    def base(n, policies=_policies):
        y1 = (rng.integers(0, 12, size=n) * 0.5).astype(np.float32)
        y2 = (rng.integers(0, 12, size=n) * 0.5).astype(np.float32)
        return dict(logits_p1=(2 * rng.standard_normal((n, 5))).astype(np.float32),
                    logits_p2=(2 * rng.standard_normal((n, 5))).astype(np.float32),
                    pred_v1=np.abs(y1 + rng.standard_normal(n)).astype(np.float32),
                    pred_v2=np.abs(y2 + 0.5 * rng.standard_normal(n)).astype(np.float32),
                    policy_p1=policies(rng, n), policy_p2=policies(rng, n), value_p1=y1, value_p2=y2,
                    policy_weight=1.0, value_weight=1.0)

    out["random"] = base(200)
    out["target_ties"] = base(100, _tied_policies)
    c = base(64)  # P1: a constant target (explained variance and correlation 0.0); P2: a constant prediction (correlation 0.0)
    c["value_p1"][:] = 2.5
    c["pred_v2"][:] = 1.25
    out["constant_value"] = c
    c = base(50)  # predictions worse than the mean: the clamp at -1
    c["pred_v1"] = (20.0 - 3.0 * c["value_p1"] + rng.standard_normal(50)).astype(np.float32)
    c["pred_v2"] = (3.0 * c["value_p2"] + 4.0).astype(np.float32)
    out["worse_than_mean"] = c
    c = base(256)
    c["policy_weight"], c["value_weight"] = 0.7, 2.5
    out["weights"] = c
    rows = R.stack_rows(T.board_games(*T.BOARDS[0]))  # real games: the targets of a 5x5 oracle self-play
    n = len(rows["value_p1"])
    n -= n % BATCH == 0  # (a short last batch)
    c = base(n)
    for k in ("policy_p1", "policy_p2", "value_p1", "value_p2"):
        c[k] = rows[k][:n].copy()
    c["pred_v1"] = np.abs(c["value_p1"] + 0.7 * rng.standard_normal(n)).astype(np.float32)
    c["pred_v2"] = np.abs(c["value_p2"] + 0.7 * rng.standard_normal(n)).astype(np.float32)
    out["real_game_5x5"] = c
    return out


def reference_numbers(case: dict) -> dict:
    import torch

    from alpharat.nn.architectures.mlp.loss import compute_mlp_losses
    from alpharat.nn.metrics import GPUMetricsAccumulator, compute_policy_metrics, compute_value_metrics
    from alpharat.nn.training.keys import BatchKey, ModelOutput

    t = {k: torch.from_numpy(case[k]) for k in INPUTS}
    n = len(case["pred_v1"])
    config = SimpleNamespace(policy_weight=case["policy_weight"], value_weight=case["value_weight"])
    acc = GPUMetricsAccumulator(torch.device("cpu"))
    outputs = []
    with torch.no_grad():
        for lo in range(0, n, BATCH):  # loop.py:312-354
            hi = min(lo + BATCH, n)
            model_output = {ModelOutput.LOGITS_P1: t["logits_p1"][lo:hi], ModelOutput.LOGITS_P2: t["logits_p2"][lo:hi],
                            ModelOutput.VALUE_P1: t["pred_v1"][lo:hi], ModelOutput.VALUE_P2: t["pred_v2"][lo:hi]}
            batch = {BatchKey.POLICY_P1: t["policy_p1"][lo:hi], BatchKey.POLICY_P2: t["policy_p2"][lo:hi],
                     BatchKey.VALUE_P1: t["value_p1"][lo:hi].unsqueeze(-1), BatchKey.VALUE_P2: t["value_p2"][lo:hi].unsqueeze(-1)}
            losses = compute_mlp_losses(model_output, batch, config)
            acc.update({k: v for k, v in losses.items() if k.startswith("loss")}, batch_size=hi - lo)
            outputs.append((model_output, batch))
        numbers = {str(k): float(v) for k, v in acc.compute().items()}
        cat = lambda d, k: torch.cat([o[d][k] for o in outputs])  # noqa: E731  (loop.py:63-70)
        for name, lk, pk in (("p1", ModelOutput.LOGITS_P1, BatchKey.POLICY_P1), ("p2", ModelOutput.LOGITS_P2, BatchKey.POLICY_P2)):
            for k, v in compute_policy_metrics(cat(0, lk), cat(1, pk)).items():
                numbers[f"{name}/{k}"] = v.item()
        for k, v in compute_value_metrics(cat(0, ModelOutput.VALUE_P1), cat(0, ModelOutput.VALUE_P2), cat(1, BatchKey.VALUE_P1),
                                          cat(1, BatchKey.VALUE_P2)).items():
            numbers[f"value/{k}"] = v.item()
    return numbers


def main() -> None:
    import numpy as np

    from tools.gen_net_golden import _install_shims

    _install_shims()
    sys.path.insert(0, str(REF))
    OUT.mkdir(parents=True, exist_ok=True)
    for name, case in cases().items():
        n = len(case["pred_v1"])
        assert n <= 256 and n % BATCH, (name, n)
        numbers = reference_numbers(case)
        keys = sorted(numbers)
        np.savez_compressed(OUT / f"{name}.npz", **{k: case[k] for k in INPUTS}, policy_weight=np.float64(case["policy_weight"]),
                            value_weight=np.float64(case["value_weight"]), ref_keys=np.array(keys),
                            ref_values=np.array([numbers[k] for k in keys], np.float64))
        print(name, n, "rows,", (OUT / f"{name}.npz").stat().st_size, "bytes;",
              " ".join(f"{k}={numbers[k]:.4g}" for k in ("loss", "p1/top1_accuracy", "value/p1_explained_variance",
                                                           "value/p1_correlation")))


if __name__ == "__main__":
    main()
