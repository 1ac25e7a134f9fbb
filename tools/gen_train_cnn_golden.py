#!/usr/bin/env python3
"""Generate tests/golden/train_cnn/*.npz: one training step of the reference's own PyRatCNN (build container only -- the
reference tree does not travel with the repository; the vectors are committed).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_train_cnn_golden.py

Per case: the model ``CNNModelConfig(trunk=TrunkConfig(channels=C, blocks=[ResBlockConfig()] * B))`` builds (``player_dim``
32, ``hidden_dim`` 64, ``MLPPolicyHead``, ``PointValueHead``) in ``.train()``, ``compute_cnn_losses`` with
``policy_weight`` 1.0 and ``value_weight`` 0.5, and ``loss.backward()``, once in float32 and once with ``model.double()`` on
the same tensors. As in tools/gen_train_sym_golden.py the BatchNorm affine parameters, running statistics and the linear
biases are randomised, the head weights are drawn at std 0.2, and the rows are rows a row set can build (a board of
tests/_rows.py, stacked, taken in ``order`` and seen by P2 where ``swap`` is set).

The ReLU guard. A convolutional BatchNorm has n hw C outputs, so the MLP fixtures' margin of 1e-4 cannot be kept; what
matters is that no ReLU's sign differs between a float32 and a float64 evaluation. Hooks on every BatchNorm2d and on
``player_encoder.0`` and ``combiner.0`` record each pre-ReLU array of both runs; ``pre_err`` is the largest
``|pre32 - pre64|`` over all of them, ``pre_min`` the smallest ``|pre64|``, and the weights' seed is the first with
``pre_min >= 8 * pre_err``. Both numbers are stored and tests/test_train_cnn_np.py asserts the inequality.

Stored, under the names of tools/gen_train_golden.py: ``sd/<name>``, the rows, ``board``, ``order``, ``swap``, ``pre_err``,
``pre_min``, and under ``f32/`` and ``f64/`` the six losses, the four outputs, ``grad/<name>`` of the parameters and
``running/<name>`` of the running statistics after the step. Only data.

Every Conv2d and Linear weight is rounded to a multiple of 2^-10 before the step (a network as good as any other for the
comparison): the state dict then compresses well. No result is rounded; the gradients do not compress, so a case is two
files, ``<name>.npz`` with the case and the ``f32/`` results and ``<name>.f64.npz`` with the ``f64/`` results, the largest
about 0.7 MB.
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
GRID = 2.0 ** 10  # the Conv2d and Linear weights are multiples of 1 / GRID


def main() -> int:
    import gen_net_golden as G

    G._install_shims()
    sys.path.insert(0, str(G.REF))
    import numpy as np
    import torch

    import _augment_np as A
    import _rows as T
    import _rows_np as R
    import _train_cnn as TC
    import _train_cnn_np as N
    from alpharat.nn.architectures.cnn.blocks import ResBlockConfig, TrunkConfig
    from alpharat.nn.architectures.cnn.config import CNNModelConfig
    from alpharat.nn.architectures.cnn.loss import compute_cnn_losses
    from alpharat.nn.training.keys import BatchKey, LossKey, ModelOutput

    out_dir = ROOT / "tests" / "golden" / "train_cnn"
    out_dir.mkdir(parents=True, exist_ok=True)
    cfg = types.SimpleNamespace(**WEIGHTS)
    boards = {b[0]: b for b in T.BOARDS}
    for idx, (name, board, Ch, B, n) in enumerate(TC.GOLDEN_CASES):
        w, h = boards[board][1], boards[board][2]
        plain = R.stack_rows(T.board_games(*boards[board]))
        total = len(plain["value_p1"])
        rng = np.random.default_rng(8300 + idx)
        order = np.concatenate([rng.permutation(total) for _ in range(-(-n // total))])[:n]
        swap = rng.random(n) < 0.5
        rows = A.swap_rows(R.take(plain, order), swap, w, h)

        def make(seed):
            torch.manual_seed(seed)
            gen = torch.Generator().manual_seed(seed + 1)
            mc = CNNModelConfig(trunk=TrunkConfig(channels=Ch, blocks=[ResBlockConfig() for _ in range(B)]))
            mc.set_data_dimensions(w, h)
            model = mc.build_model()
            G.randomise_bn(model, gen)
            with torch.no_grad():
                for head in (model.policy_head.linear, model.value_head.linear):
                    head.weight.copy_(torch.randn(head.weight.shape, generator=gen) * 0.2)
                for m in model.modules():
                    if isinstance(m, (torch.nn.Linear, torch.nn.Conv2d)):
                        m.weight.copy_(torch.round(m.weight * GRID) / GRID)
            return model

        def run(m, dtype):
            m.train()
            pre = []
            hooks = [mod.register_forward_hook(lambda _m, _i, o: pre.append(o.detach().numpy().copy())) for mod in m.modules()
                     if isinstance(mod, torch.nn.BatchNorm2d) or mod is m.player_encoder[0] or mod is m.combiner[0]]
            b = {BatchKey.OBSERVATION: torch.from_numpy(rows["observation"]).to(dtype),
                 BatchKey.POLICY_P1: torch.from_numpy(rows["policy_p1"]).to(dtype),
                 BatchKey.POLICY_P2: torch.from_numpy(rows["policy_p2"]).to(dtype),
                 BatchKey.VALUE_P1: torch.from_numpy(rows["value_p1"]).to(dtype)[:, None],
                 BatchKey.VALUE_P2: torch.from_numpy(rows["value_p2"]).to(dtype)[:, None]}
            o = m(b[BatchKey.OBSERVATION])
            for hk in hooks:
                hk.remove()
            losses = compute_cnn_losses(o, b, cfg)
            losses[LossKey.TOTAL].backward()
            res = {str(k.value if hasattr(k, "value") else k): v.detach().numpy() for k, v in losses.items()}
            res.update(logits_p1=o[ModelOutput.LOGITS_P1].detach().numpy(), logits_p2=o[ModelOutput.LOGITS_P2].detach().numpy(),
                       value_p1=o[ModelOutput.VALUE_P1].detach().numpy(), value_p2=o[ModelOutput.VALUE_P2].detach().numpy())
            for k, p in m.named_parameters():
                res[f"grad/{k}"] = p.grad.detach().numpy()
            for k, v in m.named_buffers():
                if k.endswith(("running_mean", "running_var")):
                    res[f"running/{k}"] = v.detach().numpy()
            return res, pre

        seed = 9700 + 100 * idx
        while True:
            model = make(seed)
            r32, pre32 = run(copy.deepcopy(model), torch.float32)
            r64, pre64 = run(copy.deepcopy(model).double(), torch.float64)
            assert len(pre32) == len(pre64) == 1 + 2 * B + 4
            pre_err = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(pre32, pre64))
            pre_min = min(float(np.abs(b).min()) for b in pre64)
            if pre_min >= TC.GUARD_FACTOR * pre_err:
                break
            seed += 1
            assert seed < 9700 + 100 * idx + 50, "no seed passes the guard"
        sd = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
        arrays = {}
        for tag, res, dt in (("f32", r32, np.float32), ("f64", r64, np.float64)):
            for k, v in res.items():
                assert v.dtype == dt, (tag, k, v.dtype)
                arrays[f"{tag}/{k}"] = v
        assert [k for k, _ in model.named_parameters()] == list(N.param_keys(B))
        np.savez_compressed(out_dir / f"{name}.npz", width=w, height=h, channels=Ch, n_blocks=B, board=board,
                            order=order.astype(np.int64), swap=swap, weights=np.array([WEIGHTS["policy_weight"], WEIGHTS["value_weight"]]),
                            seed=seed, pre_err=pre_err, pre_min=pre_min, observation=rows["observation"], policy_p1=rows["policy_p1"],
                            policy_p2=rows["policy_p2"], value_p1=rows["value_p1"], value_p2=rows["value_p2"],
                            **{f"sd/{k}": v for k, v in sd.items()}, **{k: v for k, v in arrays.items() if k.startswith("f32/")})
        # the float64 results in a file of their own: gradients do not compress, and C = 64 would pass 1 MiB in one file
        np.savez_compressed(out_dir / f"{name}.f64.npz", **{k: v for k, v in arrays.items() if k.startswith("f64/")})
        size = (out_dir / f"{name}.npz").stat().st_size, (out_dir / f"{name}.f64.npz").stat().st_size
        n_pre = sum(a.size for a in pre64)
        print(f"{name}: rows={n} of {total} seed={seed} pre-ReLU values={n_pre} pre_min={pre_min:.3e} pre_err={pre_err:.3e} "
              f"loss={float(arrays['f64/loss']):.6f} file={size} B")
    return 0


if __name__ == "__main__":
    os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
    sys.exit(main())
