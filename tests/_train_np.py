"""One training step of PyRatMLP in float64 NumPy -- test infrastructure only.

A restatement, written from their text, of alpharat/nn/models/mlp.py (forward, BatchNorm1d in training mode, dropout 0),
alpharat/nn/architectures/mlp/loss.py (compute_mlp_losses) and what ``loss.backward()`` leaves in the fourteen ``.grad``
tensors. It is tied to the reference by tests/golden/train (tools/gen_train_golden.py runs the reference's own model, loss
and autograd in float64); tests/test_train_np.py checks every array to 1e-12.

A *case* is a dict: ``sd`` (state-dict tensors under torch's names), ``observation`` (n, D), ``policy_p1`` / ``policy_p2``
(n, 5), ``value_p1`` / ``value_p2`` (n,), ``policy_weight``, ``value_weight``.
"""
from __future__ import annotations

import numpy as np

EPS = 1e-5
MOMENTUM = 0.1
PARAM_KEYS = ("trunk.0.weight", "trunk.0.bias", "trunk.1.weight", "trunk.1.bias", "trunk.4.weight", "trunk.4.bias",
              "trunk.5.weight", "trunk.5.bias", "policy_p1_head.weight", "policy_p1_head.bias", "policy_p2_head.weight",
              "policy_p2_head.bias", "value_head.weight", "value_head.bias")
RUNNING_KEYS = ("trunk.1.running_mean", "trunk.1.running_var", "trunk.5.running_mean", "trunk.5.running_var")
LOSS_KEYS = ("loss_p1", "loss_p2", "loss_value_p1", "loss_value_p2", "loss_value", "loss")
OUT_KEYS = ("logits_p1", "logits_p2", "value_p1", "value_p2")
# the weight whose gradient sets the floor of a layer's tolerance (tests/_train.py grad_bound)
LAYER_WEIGHT = {k: k.rsplit(".", 1)[0] + ".weight" for k in PARAM_KEYS}


def _f64(a):
    return np.asarray(a, np.float64)


def _bn_forward(z, gamma, beta):
    mu = z.mean(axis=0)
    var = ((z - mu) ** 2).mean(axis=0)
    rstd = 1.0 / np.sqrt(var + EPS)
    xhat = (z - mu) * rstd
    return gamma * xhat + beta, (xhat, rstd, mu, var)


def _bn_backward(dy, gamma, cache):
    xhat, rstd, _, _ = cache
    dxhat = dy * gamma
    dz = rstd * (dxhat - dxhat.mean(axis=0) - xhat * (dxhat * xhat).mean(axis=0))
    return dz, (dy * xhat).sum(axis=0), dy.sum(axis=0)


def _log_softmax(l):
    m = l.max(axis=1, keepdims=True)
    return l - m - np.log(np.exp(l - m).sum(axis=1, keepdims=True))


def _softplus(o):
    return np.where(o > 20.0, o, np.log1p(np.exp(np.minimum(o, 20.0))))


def step(case: dict) -> dict:
    """``losses`` (the six of LOSS_KEYS), the four outputs, ``grads`` (PARAM_KEYS), ``running`` (RUNNING_KEYS after the
    update), ``y1`` / ``y2`` (the BatchNorm outputs in front of the two ReLUs), all float64."""
    sd = {k: _f64(v) for k, v in case["sd"].items() if np.issubdtype(np.asarray(v).dtype, np.floating)}
    x = _f64(case["observation"])
    t1, t2 = _f64(case["policy_p1"]), _f64(case["policy_p2"])
    v1t, v2t = _f64(case["value_p1"]).reshape(-1), _f64(case["value_p2"]).reshape(-1)
    pw, vw = float(case["policy_weight"]), float(case["value_weight"])
    n = len(x)
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
    ls1, ls2 = _log_softmax(l1), _log_softmax(l2)
    loss_p1 = (-(t1 * ls1).sum(axis=1)).mean()
    loss_p2 = (-(t2 * ls2).sum(axis=1)).mean()
    loss_v1 = ((v[:, 0] - v1t) ** 2).mean()
    loss_v2 = ((v[:, 1] - v2t) ** 2).mean()
    loss_value = 0.5 * (loss_v1 + loss_v2)
    loss = pw * (loss_p1 + loss_p2) + vw * loss_value
    # backward
    dl1 = pw / n * (np.exp(ls1) * t1.sum(axis=1, keepdims=True) - t1)
    dl2 = pw / n * (np.exp(ls2) * t2.sum(axis=1, keepdims=True) - t2)
    with np.errstate(over="ignore"):  # exp(-o) is inf below -709, and the sigmoid there 0, as it should be
        sig = np.where(o > 20.0, 1.0, 1.0 / (1.0 + np.exp(-o)))
    do = vw / n * (v - np.stack([v1t, v2t], axis=1)) * sig
    g = {}
    for name, d in (("policy_p1_head", dl1), ("policy_p2_head", dl2), ("value_head", do)):
        g[f"{name}.weight"] = d.T @ a2
        g[f"{name}.bias"] = d.sum(axis=0)
    da2 = dl1 @ sd["policy_p1_head.weight"] + dl2 @ sd["policy_p2_head.weight"] + do @ sd["value_head.weight"]
    dz2, g["trunk.5.weight"], g["trunk.5.bias"] = _bn_backward(da2 * (y2 > 0), sd["trunk.5.weight"], c2)
    g["trunk.4.weight"], g["trunk.4.bias"] = dz2.T @ a1, dz2.sum(axis=0)
    da1 = dz2 @ sd["trunk.4.weight"]
    dz1, g["trunk.1.weight"], g["trunk.1.bias"] = _bn_backward(da1 * (y1 > 0), sd["trunk.1.weight"], c1)
    g["trunk.0.weight"], g["trunk.0.bias"] = dz1.T @ x, dz1.sum(axis=0)
    running = {}
    for bn, c in (("trunk.1", c1), ("trunk.5", c2)):
        running[f"{bn}.running_mean"] = (1 - MOMENTUM) * sd[f"{bn}.running_mean"] + MOMENTUM * c[2]
        running[f"{bn}.running_var"] = (1 - MOMENTUM) * sd[f"{bn}.running_var"] + MOMENTUM * c[3] * n / (n - 1)
    return dict(losses=dict(zip(LOSS_KEYS, (loss_p1, loss_p2, loss_v1, loss_v2, loss_value, loss))),
                logits_p1=l1, logits_p2=l2, value_p1=v[:, 0], value_p2=v[:, 1], grads=g, running=running, y1=y1, y2=y2,
                xhat1=c1[0], xhat2=c2[0], stats1=c1[1:], stats2=c2[1:], dy1=da1 * (y1 > 0), dy2=da2 * (y2 > 0), dz1=dz1, dz2=dz2,
                dout=np.concatenate([dl1, dl2, do], axis=1), head_out=np.concatenate([l1, l2, o], axis=1), z1=z1, z2=z2)


def relu_margin(case: dict, result: dict | None = None) -> float:
    """The smallest |y| over both BatchNorm outputs: how far every ReLU of the case is from flipping."""
    r = result if result is not None else step(case)
    return float(min(np.abs(r["y1"]).min(), np.abs(r["y2"]).min()))
