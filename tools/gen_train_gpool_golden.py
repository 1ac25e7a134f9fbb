#!/usr/bin/env python3
"""Generate tests/golden/train_gpool/*.npz: one training step of the reference's own PyRatCNN with GPoolResBlocks in its
trunk, one case with dropout (build container only -- the reference tree does not travel with the repository; the vectors
are committed).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_train_gpool_golden.py

Per case (tests/_train_gpool.py GOLDEN_CASES): the model ``CNNModelConfig(trunk=TrunkConfig(channels=C, blocks=[...]),
dropout=p)`` builds, a ``GPoolBlockConfig(gpool_channels=G)`` where the case names a G and a ``ResBlockConfig`` where it
names 0, in ``.train()``; ``compute_cnn_losses`` with ``policy_weight`` 1.0 and ``value_weight`` 0.5, and
``loss.backward()``, once in float32 and once with ``model.double()``. Everything else as tools/gen_train_cnn_golden.py:
randomised BatchNorm parameters, statistics and biases, head weights at std 0.2, every Conv2d and Linear weight on the
2^-10 grid, rows a row set can build. For the dropout case a forward hook on the model's two ``nn.Dropout`` modules returns
``input * mask / (1 - p)`` with the library's masks (tests/_dropout_np.py): ``player_encoder.2`` is called for P1 and then
P2 (calls 0, 1), ``combiner.2`` likewise (calls 2, 3), as tools/gen_train_dropout_golden.py does for the MLPs.

Two guards, both stored and asserted by tests/test_train_gpool_np.py. The ReLU guard of tools/gen_train_cnn_golden.py over
every BatchNorm2d (``pool_bn`` included), ``player_encoder.0`` and ``combiner.0``: ``pre_min >= 8 * pre_err``. Its twin for
the maximum, over the output ``pz`` of every ``pool_conv``: per (row, channel) the gap between the largest and the second
largest value over the cells in float64, ``max_gap`` the smallest of them, and ``pz_err = max|pz32 - pz64|``: ``max_gap >= 8 *
pz_err``. The weights' seed is the first that satisfies both.

A gpool block as block 0 reads x_0, which is equal at two cells whose 3x3 input neighbourhoods are equal; such cells tie
exactly and no weight seed separates them. The rows of a case whose first block is a gpool block are therefore drawn from
the positions that have no such pair of cells (tests/_train_gpool.py ``distinct_neighbourhoods``: all 61 of the 5x5 board,
11 of the 74 of the 7x5 board).

Stored as tools/gen_train_cnn_golden.py stores it, in two files a case, plus ``blocks``, ``pz_err``, ``max_gap``, ``p`` and,
with dropout, ``dropout_seed``, ``dropout_step`` and ``mask/<call>``. Only data.
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
GRID = 2.0 ** 10
CALLS = {"player_encoder.2": [0, 1], "combiner.2": [2, 3]}


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
    import _train_gpool as TG
    import _train_gpool_np as NG
    from alpharat.nn.architectures.cnn.blocks import GPoolBlockConfig, ResBlockConfig, TrunkConfig
    from alpharat.nn.architectures.cnn.config import CNNModelConfig
    from alpharat.nn.architectures.cnn.loss import compute_cnn_losses
    from alpharat.nn.training.keys import BatchKey, LossKey, ModelOutput

    out_dir = ROOT / "tests" / "golden" / "train_gpool"
    out_dir.mkdir(parents=True, exist_ok=True)
    cfg = types.SimpleNamespace(**WEIGHTS)
    boards = {b[0]: b for b in T.BOARDS}
    dseed, dstep = TG.GOLDEN_DROPOUT
    for idx, (name, board, Ch, blocks, n, p) in enumerate(TG.GOLDEN_CASES):
        w, h = boards[board][1], boards[board][2]
        plain = R.stack_rows(T.board_games(*boards[board]))
        total = len(plain["value_p1"])
        # a gpool block first: only the positions all of whose cells see an input neighbourhood of their own (see above)
        pool = np.arange(total)
        if blocks[0]:
            pool = np.array([i for i in range(total) if TG.distinct_neighbourhoods(plain["observation"][i:i + 1], w, h)])
            assert len(pool) >= n, f"{board} has {len(pool)} positions without equal neighbourhoods, {n} are asked for"
        rng = np.random.default_rng(8400 + idx)
        order = np.concatenate([pool[rng.permutation(len(pool))] for _ in range(-(-n // len(pool)))])[:n]
        swap = rng.random(n) < 0.5
        rows = A.swap_rows(R.take(plain, order), swap, w, h)
        assert not blocks[0] or TG.distinct_neighbourhoods(rows["observation"], w, h)
        p32 = float(np.float32(p))
        PD, HD = 32, 64
        masks = [D.mask(dseed, dstep, c, n, PD if c < 2 else HD, p) for c in range(4)] if p else None

        def make(seed):
            torch.manual_seed(seed)
            gen = torch.Generator().manual_seed(seed + 1)
            mc = CNNModelConfig(trunk=TrunkConfig(channels=Ch, blocks=[GPoolBlockConfig(gpool_channels=g) if g else ResBlockConfig()
                                                                       for g in blocks]), dropout=p32)
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
            pre, pz = [], []
            hooks = [mod.register_forward_hook(lambda _m, _i, o: pre.append(o.detach().numpy().copy())) for mod in m.modules()
                     if isinstance(mod, torch.nn.BatchNorm2d) or mod is m.player_encoder[0] or mod is m.combiner[0]]
            hooks += [mod.register_forward_hook(lambda _m, _i, o: pz.append(o.detach().numpy().copy())) for k, mod in m.named_modules()
                      if k.endswith(".pool_conv")]
            seen = {k: 0 for k in CALLS}

            def hook_for(key):
                def hook(module, inputs, output):
                    call = CALLS[key][seen[key]]
                    seen[key] += 1
                    return inputs[0] * torch.from_numpy(masks[call]).to(dtype) / (1 - p32)
                return hook

            dropouts = {k: mod for k, mod in m.named_modules() if isinstance(mod, torch.nn.Dropout)}
            assert set(dropouts) == set(CALLS) and all(mod.p == p32 for mod in dropouts.values()), list(dropouts)
            if masks is not None:
                hooks += [mod.register_forward_hook(hook_for(k)) for k, mod in dropouts.items()]
            b = {BatchKey.OBSERVATION: torch.from_numpy(rows["observation"]).to(dtype),
                 BatchKey.POLICY_P1: torch.from_numpy(rows["policy_p1"]).to(dtype),
                 BatchKey.POLICY_P2: torch.from_numpy(rows["policy_p2"]).to(dtype),
                 BatchKey.VALUE_P1: torch.from_numpy(rows["value_p1"]).to(dtype)[:, None],
                 BatchKey.VALUE_P2: torch.from_numpy(rows["value_p2"]).to(dtype)[:, None]}
            o = m(b[BatchKey.OBSERVATION])
            for hk in hooks:
                hk.remove()
            assert masks is None or all(seen[k] == 2 for k in CALLS), seen
            losses = compute_cnn_losses(o, b, cfg)
            losses[LossKey.TOTAL].backward()
            res = {str(k.value if hasattr(k, "value") else k): v.detach().numpy() for k, v in losses.items()}
            res.update(logits_p1=o[ModelOutput.LOGITS_P1].detach().numpy(), logits_p2=o[ModelOutput.LOGITS_P2].detach().numpy(),
                       value_p1=o[ModelOutput.VALUE_P1].detach().numpy(), value_p2=o[ModelOutput.VALUE_P2].detach().numpy())
            for k, q in m.named_parameters():
                res[f"grad/{k}"] = q.grad.detach().numpy()
            for k, v in m.named_buffers():
                if k.endswith(("running_mean", "running_var")):
                    res[f"running/{k}"] = v.detach().numpy()
            return res, pre, pz

        seed = 9800 + 100 * idx
        while True:
            model = make(seed)
            r32, pre32, pz32 = run(copy.deepcopy(model), torch.float32)
            r64, pre64, pz64 = run(copy.deepcopy(model).double(), torch.float64)
            n_pool = sum(1 for g in blocks if g)
            assert len(pre32) == len(pre64) == 1 + 2 * len(blocks) + n_pool + 4 and len(pz32) == len(pz64) == n_pool
            pre_err = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(pre32, pre64))
            pre_min = min(float(np.abs(b).min()) for b in pre64)
            pz_err = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(pz32, pz64))
            max_gap = NG.max_gap([np.transpose(a, (0, 2, 3, 1)).reshape(n, w * h, -1) for a in pz64])
            if pre_min >= TG.GUARD_FACTOR * pre_err and max_gap >= TG.GUARD_FACTOR * pz_err:
                break
            seed += 1
            assert seed < 9800 + 100 * idx + 100, "no seed passes both guards"
        sd = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
        arrays = {}
        for tag, res, dt in (("f32", r32, np.float32), ("f64", r64, np.float64)):
            for k, v in res.items():
                assert v.dtype == dt, (tag, k, v.dtype)
                arrays[f"{tag}/{k}"] = v
        assert [k for k, _ in model.named_parameters()] == list(NG.param_keys(blocks))
        more = {}
        if masks is not None:
            more = dict(dropout_seed=np.uint64(dseed), dropout_step=np.uint64(dstep), **{f"mask/{c}": masks[c].astype(np.uint8) for c in range(4)})
        np.savez_compressed(out_dir / f"{name}.npz", width=w, height=h, channels=Ch, blocks=np.asarray(blocks, np.int64), board=board,
                            order=order.astype(np.int64), swap=swap, weights=np.array([WEIGHTS["policy_weight"], WEIGHTS["value_weight"]]),
                            seed=seed, pre_err=pre_err, pre_min=pre_min, pz_err=pz_err, max_gap=max_gap,
                            p=np.float64(p32), observation=rows["observation"], policy_p1=rows["policy_p1"], policy_p2=rows["policy_p2"],
                            value_p1=rows["value_p1"], value_p2=rows["value_p2"], **more, **{f"sd/{k}": v for k, v in sd.items()},
                            **{k: v for k, v in arrays.items() if k.startswith("f32/")})
        np.savez_compressed(out_dir / f"{name}.f64.npz", **{k: v for k, v in arrays.items() if k.startswith("f64/")})
        size = (out_dir / f"{name}.npz").stat().st_size, (out_dir / f"{name}.f64.npz").stat().st_size
        print(f"{name}: rows={n} of {len(pool)} seed={seed} pre_min={pre_min:.3e} pre_err={pre_err:.3e} "
              f"max_gap={max_gap:.3e} pz_err={pz_err:.3e} loss={float(arrays['f64/loss']):.6f} file={size} B")
    return 0


if __name__ == "__main__":
    os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
    sys.exit(main())
