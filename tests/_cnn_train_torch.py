"""PyRatCNN restated in plain torch ops, training mode, parameters passed as a dict -- test infrastructure only.

alpharat/nn/models/cnn/model.py forward (``_parse_obs``, ``F.conv2d`` with padding 1 and no bias, ``F.batch_norm(...,
training=True, momentum=0.1, eps=1e-5)`` over NCHW, which also updates the running statistics it is given, the
mask-multiply-sum at the player cells, the DeepSet heads) with ``ResBlock``s and dropout 0; the losses are those of
tests/_mlp_torch.py (architectures/cnn/loss.py has the MLP's terms). With float64 tensors and autograd it reproduces
tests/golden/train_cnn (tests/test_train_cnn_np.py); in float32 on the CPU it is the reference error of the tolerance
(tests/_train.py grad_bounds). It is never run on the device: MIOpen compiles kernels at first use.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from _mlp_torch import losses  # noqa: F401
from _train_cnn_np import n_blocks_of, param_keys, running_keys


def forward(p: dict, x, width: int, height: int, running: dict | None = None):
    """(logits_p1, logits_p2, value_p1, value_p2); ``running``: the running_keys tensors, updated in place"""
    r = running or {}
    hw, n = width * height, x.shape[0]
    B = n_blocks_of(p)
    sc = x[:, 7 * hw:]

    def bn(name, z):
        return F.batch_norm(z, r.get(f"{name}.running_mean"), r.get(f"{name}.running_var"), p[f"{name}.weight"], p[f"{name}.bias"],
                            True, 0.1, 1e-5)

    maze = x[:, :4 * hw].view(n, height, width, 4).permute(0, 3, 1, 2)
    spatial = torch.cat([maze, x[:, 6 * hw:7 * hw].view(n, 1, height, width)], dim=1)
    feat = F.relu(bn("stem_bn", F.conv2d(spatial, p["stem.weight"], padding=1)))
    for b in range(B):
        out = F.conv2d(F.relu(bn(f"blocks.{b}.bn1", feat)), p[f"blocks.{b}.conv1.weight"], padding=1)
        out = F.conv2d(F.relu(bn(f"blocks.{b}.bn2", out)), p[f"blocks.{b}.conv2.weight"], padding=1)
        feat = out + feat
    flat = feat.reshape(n, feat.shape[1], -1)
    h = []
    for i in (0, 1):
        f = (flat * x[:, (4 + i) * hw:(5 + i) * hw].unsqueeze(1)).sum(dim=2)
        side = torch.cat([sc[:, 4 + i:5 + i], sc[:, 2 + i:3 + i], sc[:, 1:2]], dim=1)
        e = F.relu(F.linear(side, p["player_encoder.0.weight"], p["player_encoder.0.bias"]))
        h.append(F.relu(F.linear(torch.cat([f, e], dim=1), p["combiner.0.weight"], p["combiner.0.bias"])))
    agg = h[0] + h[1]
    cat = [torch.cat([h[i], agg], dim=1) for i in (0, 1)]
    logits = [F.linear(c, p["policy_head.linear.weight"], p["policy_head.linear.bias"]) for c in cat]
    values = [F.softplus(F.linear(c, p["value_head.linear.weight"], p["value_head.linear.bias"])).squeeze(-1) for c in cat]
    return logits[0], logits[1], values[0], values[1]


def step(case: dict, dtype=torch.float64, device="cpu") -> dict:
    """One step of a case of tests/_train_cnn_np.py with autograd: losses, outputs, grads, running, as NumPy arrays"""
    def t(a):
        return torch.as_tensor(a).to(device=device, dtype=dtype)

    B = n_blocks_of(case["sd"])
    p = {k: t(case["sd"][k]).clone().requires_grad_(True) for k in param_keys(B)}
    running = {k: t(case["sd"][k]).clone() for k in running_keys(B)}
    out = forward(p, t(case["observation"]), int(case["width"]), int(case["height"]), running)
    ls = losses(out, t(case["policy_p1"]), t(case["policy_p2"]), t(case["value_p1"]), t(case["value_p2"]),
                float(case["policy_weight"]), float(case["value_weight"]))
    ls["loss"].backward()
    n = lambda a: a.detach().cpu().numpy()  # noqa: E731
    return dict(losses={k: n(v) for k, v in ls.items()}, logits_p1=n(out[0]), logits_p2=n(out[1]), value_p1=n(out[2]),
                value_p2=n(out[3]), grads={k: n(v.grad) for k, v in p.items()}, running={k: n(v) for k, v in running.items()})


class _ResBlock(torch.nn.Module):
    def __init__(self, channels: int, gpool: bool = False) -> None:
        super().__init__()
        nn = torch.nn
        self.bn1 = nn.BatchNorm2d(channels)
        self.conv1 = nn.Conv2d(channels, channels, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(channels)
        self.conv2 = nn.Conv2d(channels, channels, 3, padding=1, bias=False)
        if gpool:  # GPoolResBlock's extra modules: only their names matter here
            self.pool_bn = nn.BatchNorm2d(channels)
            self.pool_conv = nn.Conv2d(channels, 8, 1, bias=False)
            self.pool_linear = nn.Linear(16, channels)


class _Head(torch.nn.Module):
    def __init__(self, i: int, o: int) -> None:
        super().__init__()
        self.linear = torch.nn.Linear(i, o)


class _PooledHead(torch.nn.Module):
    def __init__(self, i: int) -> None:
        super().__init__()
        self.mlp = torch.nn.Sequential(torch.nn.Linear(i, 8), torch.nn.ReLU(), torch.nn.Linear(8, 1))


class CNN(torch.nn.Module):
    """PyRatCNN's modules under their names (alpharat/nn/models/cnn/model.py), loaded from a state dict of NumPy arrays;
    ``forward`` is the restatement above over this module's own parameters and buffers. ``gpool`` / ``pooled_value`` /
    ``katago`` give it the modules the training step refuses; such a model is not meant to be run."""

    def __init__(self, width: int, height: int, channels: int = 32, player_dim: int = 32, hidden_dim: int = 64, n_blocks: int = 1,
                 dropout: float = 0.0, sd: dict | None = None, gpool: bool = False, pooled_value: bool = False,
                 katago: bool = False) -> None:
        super().__init__()
        nn = torch.nn
        self.width, self.height = width, height
        self.stem = nn.Conv2d(5, channels, 3, padding=1, bias=False)
        if katago:
            self.scalar_encoder = nn.Linear(6, channels)
        self.stem_bn = nn.BatchNorm2d(channels)
        self.blocks = nn.ModuleList([_ResBlock(channels, gpool and b == n_blocks - 1) for b in range(n_blocks)])
        self.player_encoder = nn.Sequential(nn.Linear(3, player_dim), nn.ReLU(), nn.Dropout(dropout))
        self.combiner = nn.Sequential(nn.Linear(channels + player_dim, hidden_dim), nn.ReLU(), nn.Dropout(dropout))
        self.policy_head = _Head(2 * hidden_dim, 5)
        self.value_head = _PooledHead(2 * channels + 2 * hidden_dim) if pooled_value else _Head(2 * hidden_dim, 1)
        if sd is not None:
            self.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=False)

    def forward(self, x):
        B = len(self.blocks)
        running = {k: v for k, v in self.named_buffers() if k in running_keys(B)} if self.training else None
        return forward(dict(self.named_parameters()), x, self.width, self.height, running)
