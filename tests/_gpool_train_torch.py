"""PyRatCNN with GPoolResBlocks and dropout restated in plain torch ops, training mode, parameters passed as a dict -- test
infrastructure only.

tests/_cnn_train_torch.py with alpharat/nn/models/cnn/blocks.py ``GPoolResBlock`` (``F.conv2d`` with a 1x1 kernel,
``mean`` and ``amax`` over the board, ``F.linear``, ``regular + pool_out + identity``) and with the dropout of
``player_encoder`` and ``combiner`` as masks passed in: ``relu(z) * mask * scale``. With float64 tensors and autograd it
reproduces tests/golden/train_gpool (tests/test_train_gpool_np.py); in float32 ON THE CPU it is the reference error of the
tolerance (tests/_train.py grad_bounds). It is never run on the device: MIOpen compiles kernels at first use.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from _mlp_torch import losses  # noqa: F401
from _train_gpool_np import blocks_of, param_keys, running_keys


def forward(p: dict, x, width: int, height: int, running: dict | None = None, masks=None, scale: float = 1.0, keep: dict | None = None,
            dropout: float = 0.0):
    """(logits_p1, logits_p2, value_p1, value_p2); ``running``: the running_keys tensors, updated in place; ``masks``: the
    four of tests/_train_gpool_np.py or None; ``keep``: a dict that receives ``pre`` and ``pz`` as that file's step names them;
    ``dropout``: torch's own ``F.dropout`` at this rate instead of masks (tools/bench_train_cnn.py's torch side)"""
    r = running or {}
    hw, n = width * height, x.shape[0]
    blocks = blocks_of(p)
    sc = x[:, 7 * hw:]
    pre, pzs = [], []
    drop = [torch.as_tensor(m).to(x.dtype) * scale for m in masks] if masks is not None else [1.0] * 4

    def bn(name, z):
        out = F.batch_norm(z, r.get(f"{name}.running_mean"), r.get(f"{name}.running_var"), p[f"{name}.weight"], p[f"{name}.bias"],
                           True, 0.1, 1e-5)
        pre.append(out)
        return out

    maze = x[:, :4 * hw].view(n, height, width, 4).permute(0, 3, 1, 2)
    spatial = torch.cat([maze, x[:, 6 * hw:7 * hw].view(n, 1, height, width)], dim=1)
    feat = F.relu(bn("stem_bn", F.conv2d(spatial, p["stem.weight"], padding=1)))
    for b, G in enumerate(blocks):
        out = F.conv2d(F.relu(bn(f"blocks.{b}.bn1", feat)), p[f"blocks.{b}.conv1.weight"], padding=1)
        out = F.conv2d(F.relu(bn(f"blocks.{b}.bn2", out)), p[f"blocks.{b}.conv2.weight"], padding=1)
        if G:
            pool = F.conv2d(F.relu(bn(f"blocks.{b}.pool_bn", feat)), p[f"blocks.{b}.pool_conv.weight"])
            pzs.append(pool)
            cat = torch.cat([pool.mean(dim=(2, 3)), pool.amax(dim=(2, 3))], dim=1)
            po = F.linear(cat, p[f"blocks.{b}.pool_linear.weight"], p[f"blocks.{b}.pool_linear.bias"])
            feat = out + po.unsqueeze(2).unsqueeze(3) + feat
        else:
            feat = out + feat
    flat = feat.reshape(n, feat.shape[1], -1)
    h = []
    for i in (0, 1):
        f = (flat * x[:, (4 + i) * hw:(5 + i) * hw].unsqueeze(1)).sum(dim=2)
        side = torch.cat([sc[:, 4 + i:5 + i], sc[:, 2 + i:3 + i], sc[:, 1:2]], dim=1)
        ze = F.linear(side, p["player_encoder.0.weight"], p["player_encoder.0.bias"])
        zc = F.linear(torch.cat([f, F.dropout(F.relu(ze), dropout, True) * drop[i]], dim=1), p["combiner.0.weight"], p["combiner.0.bias"])
        pre += [ze, zc]
        h.append(F.dropout(F.relu(zc), dropout, True) * drop[2 + i])
    pre[-4:] = [pre[-4], pre[-2], pre[-3], pre[-1]]  # ze of both players, then zc: the order of the NumPy step
    agg = h[0] + h[1]
    cat = [torch.cat([h[i], agg], dim=1) for i in (0, 1)]
    logits = [F.linear(c, p["policy_head.linear.weight"], p["policy_head.linear.bias"]) for c in cat]
    values = [F.softplus(F.linear(c, p["value_head.linear.weight"], p["value_head.linear.bias"])).squeeze(-1) for c in cat]
    if keep is not None:
        keep["pre"] = [a.detach().numpy() for a in pre]
        keep["pz"] = [a.detach().permute(0, 2, 3, 1).reshape(n, hw, -1).numpy() for a in pzs]
    return logits[0], logits[1], values[0], values[1]


def step(case: dict, dtype=torch.float64, device="cpu") -> dict:
    """One step of a case of tests/_train_gpool_np.py with autograd: losses, outputs, grads, running, pre, pz as NumPy arrays"""
    def t(a):
        return torch.as_tensor(a).to(device=device, dtype=dtype)

    blocks = blocks_of(case["sd"])
    p = {k: t(case["sd"][k]).clone().requires_grad_(True) for k in param_keys(blocks)}
    running = {k: t(case["sd"][k]).clone() for k in running_keys(blocks)}
    keep = {}
    out = forward(p, t(case["observation"]), int(case["width"]), int(case["height"]), running, case.get("masks"),
                  float(case.get("scale", 1.0)), keep)
    ls = losses(out, t(case["policy_p1"]), t(case["policy_p2"]), t(case["value_p1"]), t(case["value_p2"]),
                float(case["policy_weight"]), float(case["value_weight"]))
    ls["loss"].backward()
    n = lambda a: a.detach().cpu().numpy()  # noqa: E731
    return dict(losses={k: n(v) for k, v in ls.items()}, logits_p1=n(out[0]), logits_p2=n(out[1]), value_p1=n(out[2]),
                value_p2=n(out[3]), grads={k: n(v.grad) for k, v in p.items()}, running={k: n(v) for k, v in running.items()}, **keep)


class _Block(torch.nn.Module):
    def __init__(self, channels: int, gpool_channels: int) -> None:
        super().__init__()
        nn = torch.nn
        self.bn1 = nn.BatchNorm2d(channels)
        self.conv1 = nn.Conv2d(channels, channels, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(channels)
        self.conv2 = nn.Conv2d(channels, channels, 3, padding=1, bias=False)
        if gpool_channels:
            self.pool_bn = nn.BatchNorm2d(channels)
            self.pool_conv = nn.Conv2d(channels, gpool_channels, 1, bias=False)
            self.pool_linear = nn.Linear(2 * gpool_channels, channels)


class GPoolCNN(torch.nn.Module):
    """PyRatCNN's modules under their names with ``blocks`` a tuple of gpool_channels (0: a ResBlock), loaded from a state
    dict of NumPy arrays. The model's own forward is never run in the tests: the training step reads its parameters."""

    def __init__(self, width: int, height: int, channels: int = 32, player_dim: int = 32, hidden_dim: int = 64, blocks=(0,),
                 dropout: float = 0.0, sd: dict | None = None) -> None:
        super().__init__()
        nn = torch.nn
        self.width, self.height = width, height
        self.stem = nn.Conv2d(5, channels, 3, padding=1, bias=False)
        self.stem_bn = nn.BatchNorm2d(channels)
        self.blocks = nn.ModuleList([_Block(channels, g) for g in blocks])
        self.player_encoder = nn.Sequential(nn.Linear(3, player_dim), nn.ReLU(), nn.Dropout(dropout))
        self.combiner = nn.Sequential(nn.Linear(channels + player_dim, hidden_dim), nn.ReLU(), nn.Dropout(dropout))
        self.policy_head, self.value_head = nn.Module(), nn.Module()
        self.policy_head.linear = nn.Linear(2 * hidden_dim, 5)
        self.value_head.linear = nn.Linear(2 * hidden_dim, 1)
        if sd is not None:
            self.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=False)
