#!/usr/bin/env python3
"""Golden vectors and checkpoints for KataGoCNN (architecture ``cnn_katago``) and LocalValueMLP (``local_value``),
made by importing the reference's own config / model classes (build container only -- the reference does not
travel to the GPU box; the files are committed under tests/golden/nets_katago/ and tests/golden/ckpt_katago/).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_katago_golden.py

nets_katago/<name>.arnet + .npz: a seeded random model (BatchNorm statistics randomised, see gen_net_golden.py), its
weight blob, N observations in the flat layout and the outputs of ``predict()`` / ``forward()``.
ckpt_katago/<name>.pt + .npz: the same kind of model saved in the trainer's checkpoint layout
(``alpharat/nn/training/loop.py:392-424``, as tools/gen_ckpt_golden.py writes them), with its outputs.
These live apart from tests/golden/nets/ because the CPU oracle, which loads every blob there, has no KataGoCNN.
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def _trunk(c: int, blocks: list[dict]) -> dict:
    return dict(channels=c, blocks=blocks)


def main() -> int:
    import gen_net_golden as G

    G._install_shims()
    sys.path.insert(0, str(G.REF))
    import numpy as np
    import torch

    from alpharat.nn.architectures.cnn.config import KataGoCNNModelConfig, KataGoCNNOptimConfig
    from alpharat.nn.architectures.local_value.config import LocalValueModelConfig, LocalValueOptimConfig
    from alpharat.nn.training.keys import ModelOutput
    from alpharat_amd.weights import write_blob

    def outputs(model, obs):
        with torch.no_grad():
            x = torch.from_numpy(obs)
            pred = model.predict(x)
            fwd = model.forward(x)
        return dict(
            obs=obs,
            policy_p1=pred[ModelOutput.POLICY_P1].numpy(), policy_p2=pred[ModelOutput.POLICY_P2].numpy(),
            value_p1=pred[ModelOutput.VALUE_P1].numpy(), value_p2=pred[ModelOutput.VALUE_P2].numpy(),
            logits_p1=fwd[ModelOutput.LOGITS_P1].numpy(), logits_p2=fwd[ModelOutput.LOGITS_P2].numpy())

    only = set(sys.argv[1:])
    # ---- weight blobs
    nets = ROOT / "tests" / "golden" / "nets_katago"
    nets.mkdir(parents=True, exist_ok=True)
    blob_cases = [
        # configs/train_cnn_pos_7x7.yaml: res, res, gpool(32), hidden 64 (two 32-channel halves, one row tile)
        ("katago_7x7_c64", (7, 7), dict(trunk=_trunk(64, [dict(type="res"), dict(type="res"),
                                                          dict(type="gpool", gpool_channels=32)]),
                                        hidden_dim=64, dropout=0.1)),
        ("katago_7x5_c32", (7, 5), dict(trunk=_trunk(32, [dict(type="res"), dict(type="gpool", gpool_channels=16)]),
                                        hidden_dim=32)),
        # above 128 cells: one leaf over two row tiles per wavefront
        ("katago_15x11_c32", (15, 11), dict(trunk=_trunk(32, [dict(type="gpool", gpool_channels=16)]), hidden_dim=32)),
    ]
    for idx, (name, (w, h), kw) in enumerate(blob_cases):
        if only and name not in only:
            continue
        torch.manual_seed(8000 + idx)
        gen = torch.Generator().manual_seed(8100 + idx)
        cfg = KataGoCNNModelConfig(**kw)
        cfg.set_data_dimensions(w, h)
        model = cfg.build_model()
        G.randomise_bn(model, gen)
        model.eval()
        res = outputs(model, G.synth_obs(np.random.default_rng(8200 + idx), w, h, 24, max_turns=50))
        blob = write_blob(nets / f"{name}.arnet", "cnn_katago", w, h,
                          {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()})
        np.savez_compressed(nets / f"{name}.npz", **res)
        print(f"{name}: blob {blob.stat().st_size} B")

    # ---- trainer-layout checkpoints
    ckpts = ROOT / "tests" / "golden" / "ckpt_katago"
    ckpts.mkdir(parents=True, exist_ok=True)
    ckpt_cases = [
        ("katago_7x5_c32", KataGoCNNModelConfig(trunk=_trunk(32, [dict(type="res"), dict(type="gpool", gpool_channels=16)]),
                                                hidden_dim=32), KataGoCNNOptimConfig(), (7, 5)),
        ("local_value_5x5_h32", LocalValueModelConfig(hidden_dim=32), LocalValueOptimConfig(), (5, 5)),
    ]
    for idx, (name, mc, oc, (w, h)) in enumerate(ckpt_cases):
        if only and name not in only:
            continue
        torch.manual_seed(9000 + idx)
        gen = torch.Generator().manual_seed(9100 + idx)
        mc.set_data_dimensions(w, h)
        model = mc.build_model()
        G.randomise_bn(model, gen)
        model.eval()
        res = outputs(model, G.synth_obs(np.random.default_rng(9200 + idx), w, h, 16, max_turns=50))
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        torch.save({
            "epoch": 3,
            "model_state_dict": model.state_dict(),
            "optimizer_state_dict": opt.state_dict(),
            "val_loss": 1.25,
            "best_val_loss": 1.25,
            "config": {"model": mc.model_dump(), "optim": oc.model_dump(), "data": {"train_dir": "x", "val_dir": "y"},
                       "game": None},
            "width": w,
            "height": h,
        }, ckpts / f"{name}.pt")
        np.savez_compressed(ckpts / f"{name}.npz", **res)
        print(f"{name}: {(ckpts / f'{name}.pt').stat().st_size} B, architecture {mc.architecture}")
    return 0


if __name__ == "__main__":
    os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
    sys.exit(main())
