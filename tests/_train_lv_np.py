"""One training step of LocalValueMLP in float64 NumPy -- test infrastructure only.

A restatement, written from their text, of alpharat/nn/models/local_value.py (forward, BatchNorm1d in training mode, dropout
0), alpharat/nn/losses/ownership.py (compute_ownership_loss), alpharat/nn/architectures/local_value/loss.py
(compute_local_value_losses) and what ``loss.backward()`` leaves in the eighteen ``.grad`` tensors. The trunk, the three
heads and their loss terms are PyRatMLP's (tests/_train_np.py, whose helpers are used). It is tied to the reference by
tests/golden/train_lv (tools/gen_train_lv_golden.py runs the reference's own model, loss and autograd in float64);
tests/test_train_lv_np.py checks every array to 1e-12.

A *case* is tests/_train_np.py's with ``cheese_outcomes`` (n, h, w) int8 and ``ownership_weight``.
"""
from __future__ import annotations

import numpy as np

import _train_np as N
from _train_np import EPS, MOMENTUM, RUNNING_KEYS, _bn_backward, _bn_forward, _f64, _log_softmax, _softplus  # noqa: F401

OWN_KEYS = ("ownership_head.0.weight", "ownership_head.0.bias", "ownership_head.2.weight", "ownership_head.2.bias")
PARAM_KEYS = N.PARAM_KEYS + OWN_KEYS
LOSS_KEYS = N.LOSS_KEYS + ("loss_ownership",)
OUT_KEYS = N.OUT_KEYS + ("ownership_logits",)
LAYER_WEIGHT = {k: k.rsplit(".", 1)[0] + ".weight" for k in PARAM_KEYS}


def cell_terms(l, target, scale):
    """One cell: (ce, dl[4]) from its four logits, float64. target < 0: not active, zeros."""
    l = _f64(l)
    if target < 0:
        return 0.0, np.zeros(4)
    m = l.max()
    e = np.exp(l - m)
    s = e.sum()
    onehot = np.zeros(4)
    onehot[int(target)] = 1.0
    return float(m + np.log(s) - l[int(target)]), scale * (e / s - onehot)


def own_scale(ow: float, cells: int) -> float:
    return ow / cells if cells else 0.0


def step(case: dict) -> dict:
    """``losses`` (the seven of LOSS_KEYS), the five outputs, ``grads`` (PARAM_KEYS), ``running``, ``y1`` / ``y2`` (the
    BatchNorm outputs in front of the trunk's ReLUs), ``zo`` (the ownership head's hidden pre-activation), all float64."""
    sd = {k: _f64(v) for k, v in case["sd"].items() if np.issubdtype(np.asarray(v).dtype, np.floating)}
    x = _f64(case["observation"])
    t1, t2 = _f64(case["policy_p1"]), _f64(case["policy_p2"])
    v1t, v2t = _f64(case["value_p1"]).reshape(-1), _f64(case["value_p2"]).reshape(-1)
    pw, vw, ow = float(case["policy_weight"]), float(case["value_weight"]), float(case["ownership_weight"])
    n = len(x)
    co = np.asarray(case["cheese_outcomes"]).reshape(n, -1).astype(np.int64)
    hw = co.shape[1]
    z1 = x @ sd["trunk.0.weight"].T + sd["trunk.0.bias"]
    y1, c1 = _bn_forward(z1, sd["trunk.1.weight"], sd["trunk.1.bias"])
    a1 = np.maximum(y1, 0.0)
    z2 = a1 @ sd["trunk.4.weight"].T + sd["trunk.4.bias"]
    y2, c2 = _bn_forward(z2, sd["trunk.5.weight"], sd["trunk.5.bias"])
    a2 = np.maximum(y2, 0.0)
    l1 = a2 @ sd["policy_p1_head.weight"].T + sd["policy_p1_head.bias"]
    l2 = a2 @ sd["policy_p2_head.weight"].T + sd["policy_p2_head.bias"]
    o = a2 @ sd["value_head.weight"].T + sd["value_head.bias"]
    v = _softplus(o)
    zo = a2 @ sd["ownership_head.0.weight"].T + sd["ownership_head.0.bias"]
    ao = np.maximum(zo, 0.0)
    L = (ao @ sd["ownership_head.2.weight"].T + sd["ownership_head.2.bias"]).reshape(n, hw, 4)
    ls1, ls2 = _log_softmax(l1), _log_softmax(l2)
    loss_p1 = (-(t1 * ls1).sum(axis=1)).mean()
    loss_p2 = (-(t2 * ls2).sum(axis=1)).mean()
    loss_v1 = ((v[:, 0] - v1t) ** 2).mean()
    loss_v2 = ((v[:, 1] - v2t) ** 2).mean()
    loss_value = 0.5 * (loss_v1 + loss_v2)
    active = co >= 0
    cells = int(active.sum())
    lso = _log_softmax(L.reshape(-1, 4)).reshape(n, hw, 4)
    target = np.where(active, co, 0)
    ce = -np.take_along_axis(lso, target[:, :, None], axis=2)[:, :, 0]
    loss_own = float((ce * active).sum() / cells) if cells else 0.0
    loss = pw * (loss_p1 + loss_p2) + vw * loss_value + ow * loss_own
    # backward
    dl1 = pw / n * (np.exp(ls1) * t1.sum(axis=1, keepdims=True) - t1)
    dl2 = pw / n * (np.exp(ls2) * t2.sum(axis=1, keepdims=True) - t2)
    with np.errstate(over="ignore"):
        sig = np.where(o > 20.0, 1.0, 1.0 / (1.0 + np.exp(-o)))
    do = vw / n * (v - np.stack([v1t, v2t], axis=1)) * sig
    onehot = np.zeros((n, hw, 4))
    np.put_along_axis(onehot, target[:, :, None], 1.0, axis=2)
    dL = (own_scale(ow, cells) * (np.exp(lso) - onehot) * active[:, :, None]).reshape(n, 4 * hw)
    g = {}
    for name, d in (("policy_p1_head", dl1), ("policy_p2_head", dl2), ("value_head", do)):
        g[f"{name}.weight"] = d.T @ a2
        g[f"{name}.bias"] = d.sum(axis=0)
    g["ownership_head.2.weight"], g["ownership_head.2.bias"] = dL.T @ ao, dL.sum(axis=0)
    dzo = (dL @ sd["ownership_head.2.weight"]) * (zo > 0)
    g["ownership_head.0.weight"], g["ownership_head.0.bias"] = dzo.T @ a2, dzo.sum(axis=0)
    da2 = (dl1 @ sd["policy_p1_head.weight"] + dl2 @ sd["policy_p2_head.weight"] + do @ sd["value_head.weight"]
           + dzo @ sd["ownership_head.0.weight"])
    dz2, g["trunk.5.weight"], g["trunk.5.bias"] = _bn_backward(da2 * (y2 > 0), sd["trunk.5.weight"], c2)
    g["trunk.4.weight"], g["trunk.4.bias"] = dz2.T @ a1, dz2.sum(axis=0)
    da1 = dz2 @ sd["trunk.4.weight"]
    dz1, g["trunk.1.weight"], g["trunk.1.bias"] = _bn_backward(da1 * (y1 > 0), sd["trunk.1.weight"], c1)
    g["trunk.0.weight"], g["trunk.0.bias"] = dz1.T @ x, dz1.sum(axis=0)
    running = {}
    for bn, c in (("trunk.1", c1), ("trunk.5", c2)):
        running[f"{bn}.running_mean"] = (1 - MOMENTUM) * sd[f"{bn}.running_mean"] + MOMENTUM * c[2]
        running[f"{bn}.running_var"] = (1 - MOMENTUM) * sd[f"{bn}.running_var"] + MOMENTUM * c[3] * n / (n - 1)
    h, w = np.asarray(case["cheese_outcomes"]).shape[1:]
    return dict(losses=dict(zip(LOSS_KEYS, (loss_p1, loss_p2, loss_v1, loss_v2, loss_value, loss, loss_own))),
                logits_p1=l1, logits_p2=l2, value_p1=v[:, 0], value_p2=v[:, 1], ownership_logits=L.reshape(n, h, w, 4), grads=g,
                running=running, y1=y1, y2=y2, zo=zo, cells=cells, active=active, dl=dL.reshape(n, hw, 4), ce=ce * active)


def relu_margin(case: dict, result: dict | None = None) -> float:
    """The smallest |.| over both BatchNorm outputs and the ownership head's hidden pre-activation: how far every ReLU of
    the case is from flipping."""
    r = result if result is not None else step(case)
    return float(min(np.abs(r["y1"]).min(), np.abs(r["y2"]).min(), np.abs(r["zo"]).min()))
