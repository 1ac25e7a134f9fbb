"""LocalValueMLP restated in plain torch ops, training mode, parameters passed as a dict -- test infrastructure only.

alpharat/nn/models/local_value.py forward: PyRatMLP's trunk and three heads (tests/_mlp_torch.py) and the ownership head,
Linear - ReLU - Linear on the trunk output, viewed as (n, h, w, 4); the losses of alpharat/nn/architectures/local_value/loss.py
with alpharat/nn/losses/ownership.py's masked cross-entropy. With float64 tensors and autograd it reproduces
tests/golden/train_lv to 1e-12 (tests/test_train_lv_np.py); in float32 it is the reference error of the tolerance
(tests/_train.py grad_bounds).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import _mlp_torch as MT
from _train_lv_np import LOSS_KEYS, PARAM_KEYS, RUNNING_KEYS


def forward(p: dict, x, width: int, height: int, running: dict | None = None):
    """(logits_p1, logits_p2, value_p1, value_p2, ownership_logits (n, h, w, 4)); ``running`` updated in place"""
    r = running or {}
    h = F.linear(x, p["trunk.0.weight"], p["trunk.0.bias"])
    h = F.relu(F.batch_norm(h, r.get("trunk.1.running_mean"), r.get("trunk.1.running_var"), p["trunk.1.weight"],
                            p["trunk.1.bias"], True, 0.1, 1e-5))
    h = F.linear(h, p["trunk.4.weight"], p["trunk.4.bias"])
    h = F.relu(F.batch_norm(h, r.get("trunk.5.running_mean"), r.get("trunk.5.running_var"), p["trunk.5.weight"],
                            p["trunk.5.bias"], True, 0.1, 1e-5))
    values = F.softplus(F.linear(h, p["value_head.weight"], p["value_head.bias"]))
    own = F.linear(F.relu(F.linear(h, p["ownership_head.0.weight"], p["ownership_head.0.bias"])), p["ownership_head.2.weight"],
                   p["ownership_head.2.bias"])
    return (F.linear(h, p["policy_p1_head.weight"], p["policy_p1_head.bias"]),
            F.linear(h, p["policy_p2_head.weight"], p["policy_p2_head.bias"]), values[:, 0], values[:, 1],
            own.view(-1, height, width, 4))


def ownership_loss(logits, cheese_outcomes):
    """the mean over the cells with an outcome >= 0 of the cross-entropy against it; 0 without such a cell"""
    flat = logits.reshape(-1, 4)
    target = cheese_outcomes.reshape(-1).long()
    mask = target >= 0
    if not bool(mask.any()):
        return torch.zeros((), dtype=logits.dtype, device=logits.device)
    ce = F.cross_entropy(flat, target.clamp(min=0), reduction="none")
    m = mask.to(logits.dtype)
    return (ce * m).sum() / m.sum()


def losses(outputs, t1, t2, y1, y2, cheese_outcomes, policy_weight: float, value_weight: float, ownership_weight: float) -> dict:
    ls = MT.losses(outputs[:4], t1, t2, y1, y2, policy_weight, value_weight)
    ls["loss_ownership"] = ownership_loss(outputs[4], cheese_outcomes)
    ls["loss"] = ls["loss"] + ownership_weight * ls["loss_ownership"]
    assert tuple(ls) == LOSS_KEYS
    return ls


def step(case: dict, dtype=torch.float64, device="cpu") -> dict:
    """One step of a case of tests/_train_lv_np.py with autograd: losses, outputs, grads, running, as NumPy arrays"""
    def t(a):
        return torch.as_tensor(a).to(device=device, dtype=dtype)

    p = {k: t(case["sd"][k]).clone().requires_grad_(True) for k in PARAM_KEYS}
    running = {k: t(case["sd"][k]).clone() for k in RUNNING_KEYS}
    out = forward(p, t(case["observation"]), int(case["width"]), int(case["height"]), running)
    co = torch.as_tensor(case["cheese_outcomes"]).to(device=device)
    ls = losses(out, t(case["policy_p1"]), t(case["policy_p2"]), t(case["value_p1"]), t(case["value_p2"]), co,
                float(case["policy_weight"]), float(case["value_weight"]), float(case["ownership_weight"]))
    ls["loss"].backward()
    n = lambda a: a.detach().cpu().numpy()  # noqa: E731
    return dict(losses={k: n(v) for k, v in ls.items()}, logits_p1=n(out[0]), logits_p2=n(out[1]), value_p1=n(out[2]),
                value_p2=n(out[3]), ownership_logits=n(out[4]),
                grads={k: n(v.grad) if v.grad is not None else n(torch.zeros_like(v)) for k, v in p.items()},
                running={k: n(v) for k, v in running.items()})


class LocalValue(torch.nn.Module):
    """LocalValueMLP's modules under their names (alpharat/nn/models/local_value.py), loaded from a state dict of NumPy
    arrays; ``forward`` is the restatement above over this module's own parameters and buffers"""

    def __init__(self, width: int, height: int, hidden: int, dropout: float = 0.0, sd: dict | None = None) -> None:
        super().__init__()
        nn = torch.nn
        self.width, self.height = width, height
        obs_dim = width * height * 7 + 6
        self.trunk = nn.Sequential(nn.Linear(obs_dim, hidden), nn.BatchNorm1d(hidden), nn.ReLU(), nn.Dropout(dropout),
                                   nn.Linear(hidden, hidden), nn.BatchNorm1d(hidden), nn.ReLU(), nn.Dropout(dropout))
        self.policy_p1_head = nn.Linear(hidden, 5)
        self.policy_p2_head = nn.Linear(hidden, 5)
        self.value_head = nn.Linear(hidden, 2)
        self.ownership_head = nn.Sequential(nn.Linear(hidden, hidden), nn.ReLU(), nn.Linear(hidden, width * height * 4))
        self.register_buffer("outcome_values", torch.tensor([1.0, 0.0, 0.0, -1.0]))
        if sd is not None:
            self.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=False)

    def forward(self, x):
        running = {k: v for k, v in self.named_buffers() if k in RUNNING_KEYS} if self.training else None
        return forward(dict(self.named_parameters()), x, self.width, self.height, running)
