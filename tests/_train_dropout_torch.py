"""The three networks restated in plain torch ops with dropout masks given from outside, training mode -- test
infrastructure only.

tests/_mlp_torch.py, tests/_sym_torch.py and tests/_lv_torch.py with ``relu(bn(z)) * mask * scale`` where the models have
``nn.Dropout``; the losses are those files'. With float64 tensors and autograd it reproduces tests/golden/train_dropout to
1e-12 (tests/test_train_dropout_np.py); in float32 on the device it is the reference error of the gradient tolerance
(tests/_train.py grad_bounds). A *case* is tests/_train_dropout_np.py's.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import _lv_torch as LT
import _mlp_torch as MT
import _train_lv_np as NL
import _train_np as N
import _train_sym_np as NS


def _block(p, r, lin, bn, a, m):
    z = F.linear(a, p[f"{lin}.weight"], p[f"{lin}.bias"])
    return F.relu(F.batch_norm(z, r.get(f"{bn}.running_mean"), r.get(f"{bn}.running_var"), p[f"{bn}.weight"], p[f"{bn}.bias"],
                               True, 0.1, 1e-5)) * m


def forward_mlp(p: dict, x, m, running: dict | None = None, lv=None):
    """tests/_mlp_torch.py forward with the two masks (already times scale); ``lv``: (width, height) for LocalValueMLP"""
    r = running or {}
    h = _block(p, r, "trunk.0", "trunk.1", x, m[0])
    h = _block(p, r, "trunk.4", "trunk.5", h, m[1])
    values = F.softplus(F.linear(h, p["value_head.weight"], p["value_head.bias"]))
    out = (F.linear(h, p["policy_p1_head.weight"], p["policy_p1_head.bias"]),
           F.linear(h, p["policy_p2_head.weight"], p["policy_p2_head.bias"]), values[:, 0], values[:, 1])
    if lv is None:
        return out
    own = F.linear(F.relu(F.linear(h, p["ownership_head.0.weight"], p["ownership_head.0.bias"])), p["ownership_head.2.weight"],
                   p["ownership_head.2.bias"])
    return out + (own.view(-1, lv[1], lv[0], 4),)


def forward_sym(p: dict, x, m, width: int, height: int, running: dict | None = None):
    """tests/_sym_torch.py forward with the seven masks, in the order of tests/_dropout_np.py SYM_CALLS"""
    r = running or {}
    hw = width * height
    sc = x[:, 7 * hw:]
    shared = _block(p, r, "shared_encoder.0", "shared_encoder.1", torch.cat([x[:, :4 * hw], x[:, 6 * hw:7 * hw], sc[:, 1:2]], dim=1),
                    m[0])
    h = []
    for i in (0, 1):
        pe = _block(p, r, "player_encoder.0", "player_encoder.1",
                    torch.cat([x[:, (4 + i) * hw:(5 + i) * hw], sc[:, 2 + i:3 + i], sc[:, 4 + i:5 + i]], dim=1), m[1 + i])
        h.append(_block(p, r, "trunk.4", "trunk.5", _block(p, r, "trunk.0", "trunk.1", torch.cat([shared, pe], dim=1), m[3 + i]),
                        m[5 + i]))
    agg = h[0] + h[1]
    cat = [torch.cat([h[i], agg], dim=1) for i in (0, 1)]
    logits = [F.linear(c, p["policy_head.weight"], p["policy_head.bias"]) for c in cat]
    values = [F.softplus(F.linear(c, p["value_head.weight"], p["value_head.bias"])).squeeze(-1) for c in cat]
    return logits[0], logits[1], values[0], values[1]


def step(arch: str, case: dict, dtype=torch.float64, device="cpu") -> dict:
    """One step of a case with autograd: losses, outputs, grads, running, as NumPy arrays"""
    def t(a):
        return torch.as_tensor(a).to(device=device, dtype=dtype)

    keys = dict(mlp=N, symmetric=NS, local_value=NL)[arch]
    p = {k: t(case["sd"][k]).clone().requires_grad_(True) for k in keys.PARAM_KEYS}
    running = {k: t(case["sd"][k]).clone() for k in keys.RUNNING_KEYS}
    m = [t(a) * float(case["scale"]) for a in case["masks"]]
    x = t(case["observation"])
    targets = (t(case["policy_p1"]), t(case["policy_p2"]), t(case["value_p1"]), t(case["value_p2"]))
    pw, vw = float(case["policy_weight"]), float(case["value_weight"])
    if arch == "symmetric":
        out = forward_sym(p, x, m, int(case["width"]), int(case["height"]), running)
        ls = MT.losses(out, *targets, pw, vw)
    elif arch == "mlp":
        out = forward_mlp(p, x, m, running)
        ls = MT.losses(out, *targets, pw, vw)
    else:
        out = forward_mlp(p, x, m, running, lv=(int(case["width"]), int(case["height"])))
        co = torch.as_tensor(case["cheese_outcomes"]).to(device=device)
        ls = LT.losses(out, *targets, co, pw, vw, float(case["ownership_weight"]))
    ls["loss"].backward()
    n = lambda a: a.detach().cpu().numpy()  # noqa: E731
    res = dict(losses={k: n(v) for k, v in ls.items()}, logits_p1=n(out[0]), logits_p2=n(out[1]), value_p1=n(out[2]),
               value_p2=n(out[3]), grads={k: n(v.grad) if v.grad is not None else n(torch.zeros_like(v)) for k, v in p.items()},
               running={k: n(v) for k, v in running.items()})
    if arch == "local_value":
        res["ownership_logits"] = n(out[4])
    return res
