"""SymmetricMLP restated in plain torch ops, training mode, parameters passed as a dict -- test infrastructure only.

alpharat/nn/models/symmetric.py forward with BatchNorm1d in training mode (``F.batch_norm(..., training=True, momentum=0.1,
eps=1e-5)``, which also updates the running statistics it is given: a module called for both players takes P1's update,
then P2's) and dropout 0; the losses are those of tests/_mlp_torch.py (architectures/symmetric/loss.py has the MLP's terms).
With float64 tensors and autograd it reproduces tests/golden/train_sym to 1e-12 (tests/test_train_sym_np.py); in float32 it
is the reference error of the tolerance (tests/_train.py grad_bounds).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from _mlp_torch import losses  # noqa: F401
from _train_sym_np import PARAM_KEYS, RUNNING_KEYS


def forward(p: dict, x, width: int, height: int, running: dict | None = None):
    """(logits_p1, logits_p2, value_p1, value_p2); ``running``: the eight RUNNING_KEYS tensors, updated in place"""
    r = running or {}
    hw = width * height
    sc = x[:, 7 * hw:]

    def block(lin, bn, a):
        z = F.linear(a, p[f"{lin}.weight"], p[f"{lin}.bias"])
        return F.relu(F.batch_norm(z, r.get(f"{bn}.running_mean"), r.get(f"{bn}.running_var"), p[f"{bn}.weight"], p[f"{bn}.bias"],
                                   True, 0.1, 1e-5))

    shared = block("shared_encoder.0", "shared_encoder.1", torch.cat([x[:, :4 * hw], x[:, 6 * hw:7 * hw], sc[:, 1:2]], dim=1))
    h = []
    for i in (0, 1):
        pe = block("player_encoder.0", "player_encoder.1",
                   torch.cat([x[:, (4 + i) * hw:(5 + i) * hw], sc[:, 2 + i:3 + i], sc[:, 4 + i:5 + i]], dim=1))
        h.append(block("trunk.4", "trunk.5", block("trunk.0", "trunk.1", torch.cat([shared, pe], dim=1))))
    agg = h[0] + h[1]
    cat = [torch.cat([h[i], agg], dim=1) for i in (0, 1)]
    logits = [F.linear(c, p["policy_head.weight"], p["policy_head.bias"]) for c in cat]
    values = [F.softplus(F.linear(c, p["value_head.weight"], p["value_head.bias"])).squeeze(-1) for c in cat]
    return logits[0], logits[1], values[0], values[1]


def step(case: dict, dtype=torch.float64, device="cpu") -> dict:
    """One step of a case of tests/_train_sym_np.py with autograd: losses, outputs, grads, running, as NumPy arrays"""
    def t(a):
        return torch.as_tensor(a).to(device=device, dtype=dtype)

    p = {k: t(case["sd"][k]).clone().requires_grad_(True) for k in PARAM_KEYS}
    running = {k: t(case["sd"][k]).clone() for k in RUNNING_KEYS}
    out = forward(p, t(case["observation"]), int(case["width"]), int(case["height"]), running)
    ls = losses(out, t(case["policy_p1"]), t(case["policy_p2"]), t(case["value_p1"]), t(case["value_p2"]),
                float(case["policy_weight"]), float(case["value_weight"]))
    ls["loss"].backward()
    n = lambda a: a.detach().cpu().numpy()  # noqa: E731
    return dict(losses={k: n(v) for k, v in ls.items()}, logits_p1=n(out[0]), logits_p2=n(out[1]), value_p1=n(out[2]),
                value_p2=n(out[3]), grads={k: n(v.grad) for k, v in p.items()}, running={k: n(v) for k, v in running.items()})


class Symmetric(torch.nn.Module):
    """SymmetricMLP's modules under their names (alpharat/nn/models/symmetric.py), loaded from a state dict of NumPy
    arrays; ``forward`` is the restatement above over this module's own parameters and buffers"""

    def __init__(self, width: int, height: int, hidden: int, dropout: float = 0.0, sd: dict | None = None) -> None:
        super().__init__()
        nn = torch.nn
        hw = width * height
        self.width, self.height = width, height

        def block(i):
            return [nn.Linear(i, hidden), nn.BatchNorm1d(hidden), nn.ReLU(), nn.Dropout(dropout)]

        self.shared_encoder = nn.Sequential(*block(5 * hw + 1))
        self.player_encoder = nn.Sequential(*block(hw + 2))
        self.trunk = nn.Sequential(*block(2 * hidden), *block(hidden))
        self.policy_head = nn.Linear(2 * hidden, 5)
        self.value_head = nn.Linear(2 * hidden, 1)
        if sd is not None:
            self.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=False)

    def forward(self, x):
        running = {k: v for k, v in self.named_buffers() if k in RUNNING_KEYS} if self.training else None
        return forward(dict(self.named_parameters()), x, self.width, self.height, running)
