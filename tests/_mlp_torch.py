"""PyRatMLP restated in plain torch ops, training mode, parameters passed as a dict -- test infrastructure only.

alpharat/nn/models/mlp.py forward with BatchNorm1d in training mode (``F.batch_norm(..., training=True, momentum=0.1,
eps=1e-5)``, which also updates the running statistics it is given) and dropout 0, and the losses of
alpharat/nn/architectures/mlp/loss.py. tools/bench_validate.py does the same for eval mode. With float64 tensors and
autograd it reproduces tests/golden/train to 1e-12 (tests/test_train_np.py); in float32 it is the reference error of the
gradient tolerance (tests/_train.py).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from _train_np import LOSS_KEYS, PARAM_KEYS, RUNNING_KEYS


def forward(p: dict, x, running: dict | None = None):
    """(logits_p1, logits_p2, value_p1, value_p2); ``running``: the four RUNNING_KEYS tensors, updated in place"""
    r = running or {}
    h = F.linear(x, p["trunk.0.weight"], p["trunk.0.bias"])
    h = F.relu(F.batch_norm(h, r.get("trunk.1.running_mean"), r.get("trunk.1.running_var"), p["trunk.1.weight"],
                            p["trunk.1.bias"], True, 0.1, 1e-5))
    h = F.linear(h, p["trunk.4.weight"], p["trunk.4.bias"])
    h = F.relu(F.batch_norm(h, r.get("trunk.5.running_mean"), r.get("trunk.5.running_var"), p["trunk.5.weight"],
                            p["trunk.5.bias"], True, 0.1, 1e-5))
    values = F.softplus(F.linear(h, p["value_head.weight"], p["value_head.bias"]))
    return (F.linear(h, p["policy_p1_head.weight"], p["policy_p1_head.bias"]),
            F.linear(h, p["policy_p2_head.weight"], p["policy_p2_head.bias"]), values[:, 0], values[:, 1])


def losses(outputs, t1, t2, y1, y2, policy_weight: float, value_weight: float) -> dict:
    l1, l2, v1, v2 = outputs
    loss_p1, loss_p2 = F.cross_entropy(l1, t1), F.cross_entropy(l2, t2)
    loss_v1, loss_v2 = F.mse_loss(v1, y1.reshape(-1)), F.mse_loss(v2, y2.reshape(-1))
    loss_value = 0.5 * (loss_v1 + loss_v2)
    loss = policy_weight * (loss_p1 + loss_p2) + value_weight * loss_value
    return dict(zip(LOSS_KEYS, (loss_p1, loss_p2, loss_v1, loss_v2, loss_value, loss)))


def step(case: dict, dtype=torch.float64, device="cpu") -> dict:
    """One step of a case of tests/_train_np.py with autograd: losses, outputs, grads, running, as NumPy arrays"""
    def t(a):
        return torch.as_tensor(a).to(device=device, dtype=dtype)

    p = {k: t(case["sd"][k]).clone().requires_grad_(True) for k in PARAM_KEYS}
    running = {k: t(case["sd"][k]).clone() for k in RUNNING_KEYS}
    out = forward(p, t(case["observation"]), running)
    ls = losses(out, t(case["policy_p1"]), t(case["policy_p2"]), t(case["value_p1"]), t(case["value_p2"]),
                float(case["policy_weight"]), float(case["value_weight"]))
    ls["loss"].backward()
    n = lambda a: a.detach().cpu().numpy()  # noqa: E731
    return dict(losses={k: n(v) for k, v in ls.items()}, logits_p1=n(out[0]), logits_p2=n(out[1]), value_p1=n(out[2]),
                value_p2=n(out[3]), grads={k: n(v.grad) for k, v in p.items()}, running={k: n(v) for k, v in running.items()})


class MLP(torch.nn.Module):
    """PyRatMLP's modules under their names (alpharat/nn/models/mlp.py), loaded from a state dict of NumPy arrays"""

    def __init__(self, obs_dim: int, hidden: int, dropout: float = 0.0, sd: dict | None = None) -> None:
        super().__init__()
        nn = torch.nn
        self.trunk = nn.Sequential(nn.Linear(obs_dim, hidden), nn.BatchNorm1d(hidden), nn.ReLU(), nn.Dropout(dropout),
                                   nn.Linear(hidden, hidden), nn.BatchNorm1d(hidden), nn.ReLU(), nn.Dropout(dropout))
        self.policy_p1_head = nn.Linear(hidden, 5)
        self.policy_p2_head = nn.Linear(hidden, 5)
        self.value_head = nn.Linear(hidden, 2)
        if sd is not None:
            self.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=False)
