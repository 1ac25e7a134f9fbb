#!/usr/bin/env python3
"""Generate tests/golden/train_dropout/*.npz: one training step of the reference's own PyRatMLP, SymmetricMLP and
LocalValueMLP built with ``dropout=p`` (build container only -- the reference tree does not travel with the repository; the
vectors are committed).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_train_dropout_golden.py

Per case: the reference's model in ``.train()`` with a forward hook on every ``nn.Dropout`` module that returns
``input * mask / (1 - p)`` in place of torch's own draw, the mask being that of tests/_dropout_np.py for the module's n-th
call in forward order (SymmetricMLP calls ``player_encoder`` for P1 and P2 and then ``trunk`` for P1 and P2: calls 1, 2 and
3, 5 / 4, 6); then the reference's own loss and ``loss.backward()``, once in float32 and once with ``model.double()``, as
tools/gen_train_golden.py, tools/gen_train_sym_golden.py and tools/gen_train_lv_golden.py do. Rows, orders, weights' draws
and loss weights are those generators'. The weights' seed is the first, from those generators' starting seed on, for which
every pre-ReLU value of the float64 restatement with the masks (tests/_train_dropout_np.py) is at least 1e-4 from zero.

Stored: everything those goldens store, and ``p`` (the float32 rate as a float64), ``dropout_seed``, ``dropout_step`` and
``mask/<call>`` (uint8, 1 kept). Only data.
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

MARGIN = 1e-4
GRID = 2.0 ** 10  # SymmetricMLP's Linear weights are multiples of 1 / GRID (tools/gen_train_sym_golden.py)
# name, architecture, board of tests/_rows.py, H, rows, p, dropout seed, dropout step, rows' seed, first weights' seed
CASES = [("mlp_5x5_h32_n33_p10", "mlp", "5x5 open", 32, 33, 0.1, 1, 0, 8001, 9100),
         ("mlp_7x5_h64_n70_p50", "mlp", "7x5", 64, 70, 0.5, 2 ** 63 + 5, 3, 8002, 9200),
         ("sym_5x5_h32_n2_p10", "symmetric", "5x5 open", 32, 2, 0.1, 0, 1, 8100, 9500),
         ("sym_5x5_h32_n33_p10", "symmetric", "5x5 open", 32, 33, 0.1, 7, 2 ** 32 + 1, 8101, 9600),
         ("lv_5x5_h32_n33_p10", "local_value", "5x5 open", 32, 33, 0.1, 11, 2, 8501, 9600)]
LOSS_WEIGHTS = dict(mlp=dict(policy_weight=1.0, value_weight=0.5), symmetric=dict(policy_weight=1.0, value_weight=0.5),
                    local_value=dict(policy_weight=1.0, value_weight=0.5, ownership_weight=0.25))
# the BatchNorm call index of a Dropout module's n-th call in forward order
CALLS = dict(mlp={"trunk.3": [0], "trunk.7": [1]}, local_value={"trunk.3": [0], "trunk.7": [1]},
             symmetric={"shared_encoder.3": [0], "player_encoder.3": [1, 2], "trunk.3": [3, 4], "trunk.7": [5, 6]})


def main() -> int:
    import gen_net_golden as G

    G._install_shims()
    sys.path.insert(0, str(G.REF))
    import numpy as np
    import torch

    import _augment_np as A
    import _dropout_np as D
    import _rows as T
    import _rows_np as R
    import _train_dropout_np as ND
    from alpharat.nn.architectures.local_value.loss import compute_local_value_losses
    from alpharat.nn.architectures.mlp.loss import compute_mlp_losses
    from alpharat.nn.architectures.symmetric.loss import compute_symmetric_losses
    from alpharat.nn.models.local_value import LocalValueMLP
    from alpharat.nn.models.mlp import PyRatMLP
    from alpharat.nn.models.symmetric import SymmetricMLP
    from alpharat.nn.training.keys import BatchKey, LossKey, ModelOutput

    out_dir = ROOT / "tests" / "golden" / "train_dropout"
    out_dir.mkdir(parents=True, exist_ok=True)
    boards = {b[0]: b for b in T.BOARDS}
    loss_names = {LossKey.POLICY_P1: "loss_p1", LossKey.POLICY_P2: "loss_p2", LossKey.VALUE_P1: "loss_value_p1",
                  LossKey.VALUE_P2: "loss_value_p2", LossKey.VALUE: "loss_value", LossKey.TOTAL: "loss",
                  LossKey.OWNERSHIP: "loss_ownership"}
    loss_fns = dict(mlp=compute_mlp_losses, symmetric=compute_symmetric_losses, local_value=compute_local_value_losses)
    for name, arch, board, H, n, p, dseed, dstep, rows_seed, seed in CASES:
        w, h = boards[board][1], boards[board][2]
        weights = LOSS_WEIGHTS[arch]
        cfg = types.SimpleNamespace(**weights)
        plain = R.stack_rows(T.board_games(*boards[board]))
        total = len(plain["value_p1"])
        rng = np.random.default_rng(rows_seed)
        order = np.concatenate([rng.permutation(total) for _ in range(-(-n // total))])[:n]
        swap = rng.random(n) < 0.5
        rows = A.swap_rows(R.take(plain, order), swap, w, h)
        co = np.ascontiguousarray(rows["cheese_outcomes"], np.int8)
        p32 = float(np.float32(p))
        n_calls = sum(len(v) for v in CALLS[arch].values())
        masks = D.masks(dseed, dstep, n_calls, n, H, p)

        def make(seed):
            torch.manual_seed(seed)
            gen = torch.Generator().manual_seed(seed + 1)
            if arch == "mlp":
                model = PyRatMLP(obs_dim=w * h * 7 + 6, hidden_dim=H, dropout=p32)
                heads = (model.policy_p1_head, model.policy_p2_head, model.value_head)
            elif arch == "symmetric":
                model = SymmetricMLP(width=w, height=h, hidden_dim=H, dropout=p32)
                heads = (model.policy_head, model.value_head)
            else:
                model = LocalValueMLP(obs_dim=w * h * 7 + 6, width=w, height=h, hidden_dim=H, dropout=p32)
                heads = (model.policy_p1_head, model.policy_p2_head, model.value_head)
            G.randomise_bn(model, gen)
            with torch.no_grad():
                for head in heads:
                    head.weight.copy_(torch.randn(head.weight.shape, generator=gen) * 0.2)
                if arch == "symmetric":
                    for m in model.modules():
                        if isinstance(m, torch.nn.Linear):
                            m.weight.copy_(torch.round(m.weight * GRID) / GRID)
                if arch == "local_value":
                    l0, l2 = model.ownership_head[0], model.ownership_head[2]
                    l0.weight.copy_(torch.randn(l0.weight.shape, generator=gen) / H ** 0.5)
                    l2.weight.copy_(torch.randn(l2.weight.shape, generator=gen) * 2.0 / H ** 0.5)
                    l0.bias.copy_(torch.randn(l0.bias.shape, generator=gen) * 0.5)
                    l2.bias.copy_(torch.randn(l2.bias.shape, generator=gen) * 0.5)
            return model

        while True:
            model = make(seed)
            sd = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
            case = dict(sd=sd, width=w, height=h, observation=rows["observation"], policy_p1=rows["policy_p1"],
                        policy_p2=rows["policy_p2"], value_p1=rows["value_p1"], value_p2=rows["value_p2"], cheese_outcomes=co,
                        masks=masks, scale=1.0 / (1.0 - p32), **weights)
            margin = ND.relu_margin(arch, case)
            if margin >= MARGIN:
                break
            seed += 1
        dropouts = {k: m for k, m in model.named_modules() if isinstance(m, torch.nn.Dropout)}
        assert set(dropouts) == set(CALLS[arch]) and all(m.p == p32 for m in dropouts.values()), list(dropouts)

        def run(m, dtype):
            m.train()
            seen = {k: 0 for k in CALLS[arch]}

            def hook_for(key):
                def hook(module, inputs, output):
                    call = CALLS[arch][key][seen[key]]
                    seen[key] += 1
                    return inputs[0] * torch.from_numpy(masks[call]).to(dtype) / (1 - p32)
                return hook

            for k, mod in m.named_modules():
                if isinstance(mod, torch.nn.Dropout):
                    mod.register_forward_hook(hook_for(k))
            b = {BatchKey.OBSERVATION: torch.from_numpy(rows["observation"]).to(dtype),
                 BatchKey.POLICY_P1: torch.from_numpy(rows["policy_p1"]).to(dtype),
                 BatchKey.POLICY_P2: torch.from_numpy(rows["policy_p2"]).to(dtype),
                 BatchKey.VALUE_P1: torch.from_numpy(rows["value_p1"]).to(dtype).reshape(-1, 1),
                 BatchKey.VALUE_P2: torch.from_numpy(rows["value_p2"]).to(dtype).reshape(-1, 1),
                 BatchKey.CHEESE_OUTCOMES: torch.from_numpy(co)}
            if arch == "local_value":
                o = m(b[BatchKey.OBSERVATION], cheese_mask=b[BatchKey.CHEESE_OUTCOMES] >= 0)
            else:
                o = m(b[BatchKey.OBSERVATION])
            assert all(seen[k] == len(v) for k, v in CALLS[arch].items()), seen
            losses = loss_fns[arch](o, b, cfg)
            losses[LossKey.TOTAL].backward()
            res = {loss_names[k]: v.detach().numpy() for k, v in losses.items()}
            res.update(logits_p1=o[ModelOutput.LOGITS_P1].detach().numpy(), logits_p2=o[ModelOutput.LOGITS_P2].detach().numpy(),
                       value_p1=o[ModelOutput.VALUE_P1].detach().numpy(), value_p2=o[ModelOutput.VALUE_P2].detach().numpy())
            if arch == "local_value":
                res["ownership_logits"] = o[ModelOutput.OWNERSHIP_LOGITS].detach().numpy()
            for k, q in m.named_parameters():
                res[f"grad/{k}"] = q.grad.detach().numpy()
            for k, v in m.named_buffers():
                if k.endswith(("running_mean", "running_var")):
                    res[f"running/{k}"] = v.detach().numpy()
            return res

        arrays = {}
        for tag, m, dtype in (("f32", copy.deepcopy(model), torch.float32), ("f64", copy.deepcopy(model).double(), torch.float64)):
            for k, v in run(m, dtype).items():
                assert v.dtype == (np.float32 if tag == "f32" else np.float64), (tag, k, v.dtype)
                arrays[f"{tag}/{k}"] = v
        more = dict(cheese_outcomes=co) if arch == "local_value" else {}
        np.savez_compressed(out_dir / f"{name}.npz", architecture=arch, width=w, height=h, hidden=H, board=board,
                            order=order.astype(np.int64), swap=swap, weights=np.array(list(weights.values())), seed=seed,
                            p=np.float64(p32), dropout_seed=np.uint64(dseed), dropout_step=np.uint64(dstep),
                            observation=rows["observation"], policy_p1=rows["policy_p1"], policy_p2=rows["policy_p2"],
                            value_p1=rows["value_p1"], value_p2=rows["value_p2"], **more,
                            **{f"mask/{c}": masks[c].astype(np.uint8) for c in range(n_calls)},
                            **{f"sd/{k}": v for k, v in sd.items()}, **arrays)
        size = (out_dir / f"{name}.npz").stat().st_size
        kept = np.mean([m.mean() for m in masks])
        print(f"{name}: rows={n} of {total} seed={seed} relu_margin={margin:.3e} kept={kept:.3f} "
              f"loss={float(arrays['f64/loss']):.6f} file={size} B")
    return 0


if __name__ == "__main__":
    os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
    sys.exit(main())
