#!/usr/bin/env python3
"""Generate tests/golden/train_lv/*.npz: one training step of the reference's own LocalValueMLP (build container only -- the
reference tree does not travel with the repository; the vectors are committed).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_train_lv_golden.py

Per case: the reference's ``LocalValueMLP`` in ``.train()``, ``compute_local_value_losses`` with ``policy_weight`` 1.0,
``value_weight`` 0.5 and ``ownership_weight`` 0.25 (three different weights: a forgotten or misplaced one shows), and
``loss.backward()``, once in float32 and once with ``model.double()`` on the same tensors. The BatchNorm affine parameters,
running statistics and the linear biases are randomised (tools/gen_net_golden.py), the three heads' weights are drawn at std
0.2 as tools/gen_train_golden.py does, and the ownership head is redrawn as tools/gen_ownership_golden.py does (weights std
1/sqrt(H) and 2/sqrt(H), biases std 0.5; the reference's std 0.01 gives near-uniform logits that tell nothing apart).

The rows are rows a row set can build, as in tools/gen_train_golden.py: the oracle games of a board of tests/_rows.py, stacked,
taken in ``order`` and seen by P2 where ``swap`` is set -- their cheese outcomes with them (classes 0 and 3 exchanged). The
weights' seed is the first for which both BatchNorm outputs and the ownership head's hidden pre-activation of the float64
restatement (tests/_train_lv_np.py) are at least 1e-4 away from zero (tests/test_train_lv_np.py asserts the margin).

Stored: ``sd/<name>`` (the state dict before the step), the rows (observation, policy and value targets, cheese outcomes),
``board``, ``order``, ``swap``, and under ``f32/`` and ``f64/`` the seven losses, the five outputs, ``grad/<name>`` of the
eighteen parameters and ``running/<name>`` of the four running statistics after the step. Only data.
"""
from __future__ import annotations

import copy
import os
import sys
import types
from pathlib import Path

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))

WEIGHTS = dict(policy_weight=1.0, value_weight=0.5, ownership_weight=0.25)
MARGIN = 1e-4
# name, board of tests/_rows.py, H, rows
CASES = [("lv_5x5_h32_n2", "5x5 open", 32, 2), ("lv_5x5_h32_n33", "5x5 open", 32, 33), ("lv_7x5_h64_n70", "7x5", 64, 70)]


def main() -> int:
    import gen_net_golden as G

    G._install_shims()
    sys.path.insert(0, str(G.REF))
    import numpy as np
    import torch

    import _augment_np as A
    import _rows as T
    import _rows_np as R
    import _train_lv_np as NL
    from alpharat.nn.architectures.local_value.loss import compute_local_value_losses
    from alpharat.nn.models.local_value import LocalValueMLP
    from alpharat.nn.training.keys import BatchKey, LossKey, ModelOutput

    out_dir = ROOT / "tests" / "golden" / "train_lv"
    out_dir.mkdir(parents=True, exist_ok=True)
    cfg = types.SimpleNamespace(**WEIGHTS)
    boards = {b[0]: b for b in T.BOARDS}
    loss_names = {LossKey.POLICY_P1: "loss_p1", LossKey.POLICY_P2: "loss_p2", LossKey.VALUE_P1: "loss_value_p1",
                  LossKey.VALUE_P2: "loss_value_p2", LossKey.VALUE: "loss_value", LossKey.TOTAL: "loss",
                  LossKey.OWNERSHIP: "loss_ownership"}
    for idx, (name, board, H, n) in enumerate(CASES):
        w, h = boards[board][1], boards[board][2]
        plain = R.stack_rows(T.board_games(*boards[board]))
        total = len(plain["value_p1"])
        rng = np.random.default_rng(8500 + idx)
        order = np.concatenate([rng.permutation(total) for _ in range(-(-n // total))])[:n]
        swap = rng.random(n) < 0.5
        rows = A.swap_rows(R.take(plain, order), swap, w, h)
        co = np.ascontiguousarray(rows["cheese_outcomes"], np.int8)

        def make(seed):
            torch.manual_seed(seed)
            gen = torch.Generator().manual_seed(seed + 1)
            model = LocalValueMLP(obs_dim=w * h * 7 + 6, width=w, height=h, hidden_dim=H)
            G.randomise_bn(model, gen)
            with torch.no_grad():
                for head in (model.policy_p1_head, model.policy_p2_head, model.value_head):
                    head.weight.copy_(torch.randn(head.weight.shape, generator=gen) * 0.2)
                l0, l2 = model.ownership_head[0], model.ownership_head[2]
                l0.weight.copy_(torch.randn(l0.weight.shape, generator=gen) / H ** 0.5)
                l2.weight.copy_(torch.randn(l2.weight.shape, generator=gen) * 2.0 / H ** 0.5)
                l0.bias.copy_(torch.randn(l0.bias.shape, generator=gen) * 0.5)
                l2.bias.copy_(torch.randn(l2.bias.shape, generator=gen) * 0.5)
            return model

        seed = 9500 + 100 * idx
        while True:
            model = make(seed)
            sd = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
            case = dict(sd=sd, observation=rows["observation"], policy_p1=rows["policy_p1"], policy_p2=rows["policy_p2"],
                        value_p1=rows["value_p1"], value_p2=rows["value_p2"], cheese_outcomes=co, **WEIGHTS)
            margin = NL.relu_margin(case)
            if margin >= MARGIN:
                break
            seed += 1

        def run(m, dtype):
            m.train()
            b = {BatchKey.OBSERVATION: torch.from_numpy(rows["observation"]).to(dtype),
                 BatchKey.POLICY_P1: torch.from_numpy(rows["policy_p1"]).to(dtype),
                 BatchKey.POLICY_P2: torch.from_numpy(rows["policy_p2"]).to(dtype),
                 BatchKey.VALUE_P1: torch.from_numpy(rows["value_p1"]).to(dtype).reshape(-1, 1),
                 BatchKey.VALUE_P2: torch.from_numpy(rows["value_p2"]).to(dtype).reshape(-1, 1),
                 BatchKey.CHEESE_OUTCOMES: torch.from_numpy(co)}
            o = m(b[BatchKey.OBSERVATION], cheese_mask=b[BatchKey.CHEESE_OUTCOMES] >= 0)
            losses = compute_local_value_losses(o, b, cfg)
            losses[LossKey.TOTAL].backward()
            res = {loss_names[k]: v.detach().numpy() for k, v in losses.items()}
            res.update(logits_p1=o[ModelOutput.LOGITS_P1].detach().numpy(), logits_p2=o[ModelOutput.LOGITS_P2].detach().numpy(),
                       value_p1=o[ModelOutput.VALUE_P1].detach().numpy(), value_p2=o[ModelOutput.VALUE_P2].detach().numpy(),
                       ownership_logits=o[ModelOutput.OWNERSHIP_LOGITS].detach().numpy())
            for k, p in m.named_parameters():
                res[f"grad/{k}"] = p.grad.detach().numpy()
            for k, v in m.named_buffers():
                if k.endswith(("running_mean", "running_var")):
                    res[f"running/{k}"] = v.detach().numpy()
            return res

        arrays = {}
        for tag, m, dtype in (("f32", copy.deepcopy(model), torch.float32), ("f64", copy.deepcopy(model).double(), torch.float64)):
            for k, v in run(m, dtype).items():
                assert v.dtype == (np.float32 if tag == "f32" else np.float64), (tag, k, v.dtype)
                arrays[f"{tag}/{k}"] = v
        assert len([k for k in arrays if k.startswith("f64/grad/")]) == 18 and "f64/loss_ownership" in arrays
        np.savez_compressed(out_dir / f"{name}.npz", width=w, height=h, hidden=H, board=board, order=order.astype(np.int64),
                            swap=swap, weights=np.array([WEIGHTS["policy_weight"], WEIGHTS["value_weight"],
                                                         WEIGHTS["ownership_weight"]]), seed=seed,
                            observation=rows["observation"], policy_p1=rows["policy_p1"], policy_p2=rows["policy_p2"],
                            value_p1=rows["value_p1"], value_p2=rows["value_p2"], cheese_outcomes=co,
                            **{f"sd/{k}": v for k, v in sd.items()}, **arrays)
        size = (out_dir / f"{name}.npz").stat().st_size
        print(f"{name}: rows={n} of {total} seed={seed} relu_margin={margin:.3e} active={int((co >= 0).sum())} "
              f"loss={float(arrays['f64/loss']):.6f} loss_ownership={float(arrays['f64/loss_ownership']):.6f} file={size} B")
    return 0


if __name__ == "__main__":
    os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
    sys.exit(main())
