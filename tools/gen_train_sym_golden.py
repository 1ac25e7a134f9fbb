#!/usr/bin/env python3
"""Generate tests/golden/train_sym/*.npz: one training step of the reference's own SymmetricMLP (build container only -- the
reference tree does not travel with the repository; the vectors are committed).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_train_sym_golden.py

Per case: the reference's ``SymmetricMLP`` in ``.train()``, ``compute_symmetric_losses`` with ``policy_weight`` 1.0 and
``value_weight`` 0.5, and ``loss.backward()``, once in float32 and once with ``model.double()`` on the same tensors. As in
tools/gen_train_golden.py the BatchNorm affine parameters, running statistics and the linear biases are randomised, the head
weights are drawn at std 0.2, the rows are rows a row set can build (a board of tests/_rows.py, stacked, taken in ``order``
and seen by P2 where ``swap`` is set), and the weights' seed is the first for which every one of the seven BatchNorm
outputs of the float64 restatement (tests/_train_sym_np.py) is at least 1e-4 away from zero.

Stored, under the names of tools/gen_train_golden.py: ``sd/<name>``, the rows, ``board``, ``order``, ``swap``, and under
``f32/`` and ``f64/`` the six losses, the four outputs, ``grad/<name>`` of the twenty parameters and ``running/<name>`` of
the eight running statistics after the step. Only data.

Every Linear weight is rounded to a multiple of 2^-10 before the step (a network as good as any other for the comparison):
the state dict then compresses to a third, which keeps the largest file under 300 KB. No result is rounded.
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

WEIGHTS = dict(policy_weight=1.0, value_weight=0.5)
MARGIN = 1e-4
GRID = 2.0 ** 10  # the Linear weights are multiples of 1 / GRID
# name, board of tests/_rows.py, H, rows
CASES = [("sym_5x5_h32_n2", "5x5 open", 32, 2), ("sym_5x5_h32_n33", "5x5 open", 32, 33), ("sym_7x5_h64_n70", "7x5", 64, 70)]


def main() -> int:
    import gen_net_golden as G

    G._install_shims()
    sys.path.insert(0, str(G.REF))
    import numpy as np
    import torch

    import _augment_np as A
    import _rows as T
    import _rows_np as R
    import _train_sym_np as N
    from alpharat.nn.architectures.symmetric.loss import compute_symmetric_losses
    from alpharat.nn.models.symmetric import SymmetricMLP
    from alpharat.nn.training.keys import BatchKey, LossKey, ModelOutput

    out_dir = ROOT / "tests" / "golden" / "train_sym"
    out_dir.mkdir(parents=True, exist_ok=True)
    cfg = types.SimpleNamespace(**WEIGHTS)
    boards = {b[0]: b for b in T.BOARDS}
    for idx, (name, board, H, n) in enumerate(CASES):
        w, h = boards[board][1], boards[board][2]
        plain = R.stack_rows(T.board_games(*boards[board]))
        total = len(plain["value_p1"])
        rng = np.random.default_rng(8100 + idx)
        order = np.concatenate([rng.permutation(total) for _ in range(-(-n // total))])[:n]
        swap = rng.random(n) < 0.5
        rows = A.swap_rows(R.take(plain, order), swap, w, h)

        def make(seed):
            torch.manual_seed(seed)
            gen = torch.Generator().manual_seed(seed + 1)
            model = SymmetricMLP(width=w, height=h, hidden_dim=H)
            G.randomise_bn(model, gen)
            with torch.no_grad():
                for head in (model.policy_head, model.value_head):
                    head.weight.copy_(torch.randn(head.weight.shape, generator=gen) * 0.2)
                for m in model.modules():
                    if isinstance(m, torch.nn.Linear):
                        m.weight.copy_(torch.round(m.weight * GRID) / GRID)
            return model

        seed = 9500 + 100 * idx
        while True:
            model = make(seed)
            sd = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
            case = dict(sd=sd, width=w, height=h, observation=rows["observation"], policy_p1=rows["policy_p1"],
                        policy_p2=rows["policy_p2"], value_p1=rows["value_p1"], value_p2=rows["value_p2"], **WEIGHTS)
            margin = N.relu_margin(case)
            if margin >= MARGIN:
                break
            seed += 1

        def run(m, dtype):
            m.train()
            b = {BatchKey.OBSERVATION: torch.from_numpy(rows["observation"]).to(dtype),
                 BatchKey.POLICY_P1: torch.from_numpy(rows["policy_p1"]).to(dtype),
                 BatchKey.POLICY_P2: torch.from_numpy(rows["policy_p2"]).to(dtype),
                 BatchKey.VALUE_P1: torch.from_numpy(rows["value_p1"]).to(dtype)[:, None],
                 BatchKey.VALUE_P2: torch.from_numpy(rows["value_p2"]).to(dtype)[:, None]}
            o = m(b[BatchKey.OBSERVATION])
            losses = compute_symmetric_losses(o, b, cfg)
            losses[LossKey.TOTAL].backward()
            res = {str(k.value if hasattr(k, "value") else k): v.detach().numpy() for k, v in losses.items()}
            res.update(logits_p1=o[ModelOutput.LOGITS_P1].detach().numpy(), logits_p2=o[ModelOutput.LOGITS_P2].detach().numpy(),
                       value_p1=o[ModelOutput.VALUE_P1].detach().numpy(), value_p2=o[ModelOutput.VALUE_P2].detach().numpy())
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
        assert [k for k, _ in model.named_parameters()] == list(N.PARAM_KEYS)
        np.savez_compressed(out_dir / f"{name}.npz", width=w, height=h, hidden=H, board=board, order=order.astype(np.int64),
                            swap=swap, weights=np.array([WEIGHTS["policy_weight"], WEIGHTS["value_weight"]]), seed=seed,
                            observation=rows["observation"], policy_p1=rows["policy_p1"], policy_p2=rows["policy_p2"],
                            value_p1=rows["value_p1"], value_p2=rows["value_p2"], **{f"sd/{k}": v for k, v in sd.items()},
                            **arrays)
        size = (out_dir / f"{name}.npz").stat().st_size
        print(f"{name}: rows={n} of {total} seed={seed} relu_margin={margin:.3e} loss={float(arrays['f64/loss']):.6f} file={size} B")
    return 0


if __name__ == "__main__":
    os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
    sys.exit(main())
