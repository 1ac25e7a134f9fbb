#!/usr/bin/env python3
"""Generate tests/golden/ownership/*.npz: the reference's own LocalValueMLP and its loss on a few rows (build container
only -- the reference tree does not travel with the repository; the vectors are committed).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_ownership_golden.py

Per case: the reference's ``LocalValueMLP`` in eval mode with BatchNorm statistics randomised (tools/gen_net_golden.py) and
the ownership head redrawn so that its logits tell classes and cells apart (weights std 1/sqrt(H) and 2/sqrt(H), biases std
0.5; the reference's std 0.01 gives near-uniform logits). The model runs with ``cheese_mask = cheese_outcomes >= 0``;
``compute_local_value_losses`` gives the loss of one batch over all rows and of batches of three rows, which are
accumulated weighted by batch size as the training loop's validation pass does (the last batch is short). Stored: the
state dict's tensors (``sd/<name>``), the rows (observation, policy and value targets, cheese outcomes), and the reference's
``ownership_logits``, ``ownership_value``, ``loss_ownership`` and ``loss`` (``*_one_batch``: a single batch).
"""
from __future__ import annotations

import os
import sys
import types
from pathlib import Path

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

BATCH = 3
WEIGHTS = dict(policy_weight=1.0, value_weight=0.5, ownership_weight=0.25)
# name, (w, h), H, rows, the batch whose rows have no cheese (or None)
CASES = [("lv_5x5_h32", (5, 5), 32, 20, 1), ("lv_7x5_h64", (7, 5), 64, 17, None)]


def main() -> int:
    import gen_net_golden as G

    G._install_shims()
    sys.path.insert(0, str(G.REF))
    import numpy as np
    import torch

    from alpharat.nn.architectures.local_value.loss import compute_local_value_losses
    from alpharat.nn.models.local_value import LocalValueMLP
    from alpharat.nn.training.keys import BatchKey, LossKey, ModelOutput

    out_dir = ROOT / "tests" / "golden" / "ownership"
    out_dir.mkdir(parents=True, exist_ok=True)
    cfg = types.SimpleNamespace(**WEIGHTS)
    for idx, (name, (w, h), H, n, empty_batch) in enumerate(CASES):
        torch.manual_seed(5000 + idx)
        gen = torch.Generator().manual_seed(6000 + idx)
        hw = w * h
        model = LocalValueMLP(obs_dim=hw * 7 + 6, width=w, height=h, hidden_dim=H)
        G.randomise_bn(model, gen)
        with torch.no_grad():
            l0, l2 = model.ownership_head[0], model.ownership_head[2]
            l0.weight.copy_(torch.randn(l0.weight.shape, generator=gen) / H ** 0.5)
            l2.weight.copy_(torch.randn(l2.weight.shape, generator=gen) * 2.0 / H ** 0.5)
            l0.bias.copy_(torch.randn(l0.bias.shape, generator=gen) * 0.5)
            l2.bias.copy_(torch.randn(l2.bias.shape, generator=gen) * 0.5)
        model.eval()
        rng = np.random.default_rng(7000 + idx)
        obs = G.synth_obs(rng, w, h, n, max_turns=50)
        if empty_batch is not None:
            obs[empty_batch * BATCH:(empty_batch + 1) * BATCH, hw * 6:hw * 7] = 0.0
        cheese = obs[:, hw * 6:hw * 7] > 0
        co = np.where(cheese, rng.integers(0, 4, size=(n, hw)), -1).astype(np.int8).reshape(n, h, w)
        pol = [rng.dirichlet(np.ones(5), size=n).astype(np.float32) for _ in range(2)]
        val = [(rng.integers(0, 9, size=n) * 0.5).astype(np.float32) for _ in range(2)]
        batch = {BatchKey.OBSERVATION: torch.from_numpy(obs), BatchKey.POLICY_P1: torch.from_numpy(pol[0]),
                 BatchKey.POLICY_P2: torch.from_numpy(pol[1]), BatchKey.VALUE_P1: torch.from_numpy(val[0])[:, None],
                 BatchKey.VALUE_P2: torch.from_numpy(val[1])[:, None], BatchKey.CHEESE_OUTCOMES: torch.from_numpy(co)}

        def losses(lo, hi):
            b = {k: v[lo:hi] for k, v in batch.items()}
            with torch.no_grad():
                o = model(b[BatchKey.OBSERVATION], cheese_mask=b[BatchKey.CHEESE_OUTCOMES] >= 0)
                return o, compute_local_value_losses(o, b, cfg)

        whole, one = losses(0, n)
        acc = {LossKey.OWNERSHIP: 0.0, LossKey.TOTAL: 0.0}
        for lo in range(0, n, BATCH):
            hi = min(lo + BATCH, n)
            _, l = losses(lo, hi)
            for k in acc:
                acc[k] += float(l[k]) * (hi - lo)
        sd = {f"sd/{k}": v.detach().cpu().numpy() for k, v in model.state_dict().items()}
        np.savez_compressed(
            out_dir / f"{name}.npz", width=w, height=h, hidden=H, max_turns=50, batch_rows=BATCH,
            weights=np.array([WEIGHTS["policy_weight"], WEIGHTS["value_weight"], WEIGHTS["ownership_weight"]]),
            observation=obs, policy_p1=pol[0], policy_p2=pol[1], value_p1=val[0], value_p2=val[1], cheese_outcomes=co,
            ownership_logits=whole[ModelOutput.OWNERSHIP_LOGITS].numpy(), ownership_value=whole[ModelOutput.OWNERSHIP_VALUE].numpy(),
            logits_p1=whole[ModelOutput.LOGITS_P1].numpy(), logits_p2=whole[ModelOutput.LOGITS_P2].numpy(),
            pred_value_p1=whole[ModelOutput.VALUE_P1].numpy(), pred_value_p2=whole[ModelOutput.VALUE_P2].numpy(),
            loss_ownership=acc[LossKey.OWNERSHIP] / n, loss=acc[LossKey.TOTAL] / n,
            loss_ownership_one_batch=float(one[LossKey.OWNERSHIP]), loss_one_batch=float(one[LossKey.TOTAL]), **sd)
        size = (out_dir / f"{name}.npz").stat().st_size
        print(f"{name}: rows={n} loss_ownership={acc[LossKey.OWNERSHIP] / n:.6f} loss={acc[LossKey.TOTAL] / n:.6f} file={size} B")
    return 0


if __name__ == "__main__":
    os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
    sys.exit(main())
