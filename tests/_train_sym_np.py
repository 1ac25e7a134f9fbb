"""One training step of SymmetricMLP in float64 NumPy -- test infrastructure only.

A restatement, written from their text, of alpharat/nn/models/symmetric.py (``_parse_obs`` and ``forward`` with BatchNorm1d
in training mode, dropout 0), alpharat/nn/architectures/symmetric/loss.py (``compute_symmetric_losses``) and what
``loss.backward()`` leaves in the twenty ``.grad`` tensors. It is tied to the reference by tests/golden/train_sym
(tools/gen_train_sym_golden.py runs the reference's own model, loss and autograd in float64); tests/test_train_sym_np.py
checks every array to 1e-12.

Four BatchNorm modules are applied seven times: ``shared_encoder.1`` once, ``player_encoder.1``, ``trunk.1`` and ``trunk.5``
for P1's rows and then for P2's, each call with its own batch statistics; a module's running statistics take P1's update and
then P2's on top of it, and every shared tensor's gradient is the sum of its two calls' contributions.

A *case* is tests/_train_np.py's, with ``width`` and ``height`` and a SymmetricMLP state dict under ``sd``.
"""
from __future__ import annotations

import numpy as np

from _train_np import EPS, LOSS_KEYS, MOMENTUM, OUT_KEYS, _bn_backward, _bn_forward, _f64, _log_softmax, _softplus  # noqa: F401

PARAM_KEYS = ("shared_encoder.0.weight", "shared_encoder.0.bias", "shared_encoder.1.weight", "shared_encoder.1.bias",
              "player_encoder.0.weight", "player_encoder.0.bias", "player_encoder.1.weight", "player_encoder.1.bias",
              "trunk.0.weight", "trunk.0.bias", "trunk.1.weight", "trunk.1.bias", "trunk.4.weight", "trunk.4.bias",
              "trunk.5.weight", "trunk.5.bias", "policy_head.weight", "policy_head.bias", "value_head.weight", "value_head.bias")
BN_MODULES = ("shared_encoder.1", "player_encoder.1", "trunk.1", "trunk.5")
RUNNING_KEYS = tuple(f"{bn}.{s}" for bn in BN_MODULES for s in ("running_mean", "running_var"))
# the biases in front of a BatchNorm: their true gradient is zero
NOISE_BIASES = ("shared_encoder.0.bias", "player_encoder.0.bias", "trunk.0.bias", "trunk.4.bias")
# the weight whose gradient sets the floor of a layer's tolerance (tests/_train.py grad_bounds)
LAYER_WEIGHT = {k: k.rsplit(".", 1)[0] + ".weight" for k in PARAM_KEYS}
# the seven BatchNorm applications, in the order the step makes them
BN_CALLS = ("shared_encoder.1", "player_encoder.1/p1", "player_encoder.1/p2", "trunk.1/p1", "trunk.1/p2", "trunk.5/p1",
            "trunk.5/p2")


def split_inputs(x, width: int, height: int):
    """(shared_raw, [p1_raw, p2_raw]) of flat rows x: ``_parse_obs``"""
    hw = width * height
    sc = x[:, 7 * hw:]
    shared = np.concatenate([x[:, :4 * hw], x[:, 6 * hw:7 * hw], sc[:, 1:2]], axis=1)
    players = [np.concatenate([x[:, (4 + p) * hw:(5 + p) * hw], sc[:, 2 + p:3 + p], sc[:, 4 + p:5 + p]], axis=1) for p in (0, 1)]
    return shared, players


def step(case: dict) -> dict:
    """``losses``, the four outputs, ``grads`` (PARAM_KEYS), ``running`` (RUNNING_KEYS after the update) and ``bn_out``, the
    seven BatchNorm outputs in front of the ReLUs in BN_CALLS' order; all float64. The rest are intermediates for the
    harness tests."""
    sd = {k: _f64(v) for k, v in case["sd"].items() if np.issubdtype(np.asarray(v).dtype, np.floating)}
    x = _f64(case["observation"])
    t = [_f64(case["policy_p1"]), _f64(case["policy_p2"])]
    y = [_f64(case["value_p1"]).reshape(-1), _f64(case["value_p2"]).reshape(-1)]
    pw, vw = float(case["policy_weight"]), float(case["value_weight"])
    n = len(x)
    H = sd["trunk.4.weight"].shape[0]
    lin = lambda name, a: a @ sd[f"{name}.weight"].T + sd[f"{name}.bias"]  # noqa: E731
    bn = lambda name, z: _bn_forward(z, sd[f"{name}.weight"], sd[f"{name}.bias"])  # noqa: E731
    xs, xp = split_inputs(x, int(case["width"]), int(case["height"]))
    # forward
    ys, cs = bn("shared_encoder.1", lin("shared_encoder.0", xs))
    shared = np.maximum(ys, 0.0)
    yp, cp, pe, cat, y1, c1, a1, y5, c5, hh = ([None, None] for _ in range(10))
    for i in (0, 1):
        yp[i], cp[i] = bn("player_encoder.1", lin("player_encoder.0", xp[i]))
        pe[i] = np.maximum(yp[i], 0.0)
        cat[i] = np.concatenate([shared, pe[i]], axis=1)
        y1[i], c1[i] = bn("trunk.1", lin("trunk.0", cat[i]))
        a1[i] = np.maximum(y1[i], 0.0)
        y5[i], c5[i] = bn("trunk.5", lin("trunk.4", a1[i]))
        hh[i] = np.maximum(y5[i], 0.0)
    agg = hh[0] + hh[1]
    hcat = [np.concatenate([hh[i], agg], axis=1) for i in (0, 1)]
    l = [lin("policy_head", hcat[i]) for i in (0, 1)]
    o = [lin("value_head", hcat[i])[:, 0] for i in (0, 1)]
    v = [_softplus(o[i]) for i in (0, 1)]
    ls = [_log_softmax(l[i]) for i in (0, 1)]
    loss_p = [(-(t[i] * ls[i]).sum(axis=1)).mean() for i in (0, 1)]
    loss_v = [((v[i] - y[i]) ** 2).mean() for i in (0, 1)]
    loss_value = 0.5 * (loss_v[0] + loss_v[1])
    loss = pw * (loss_p[0] + loss_p[1]) + vw * loss_value
    # backward: the heads, Wh = [policy_head; value_head] (6, 2H)
    dout = []
    for i in (0, 1):
        dl = pw / n * (np.exp(ls[i]) * t[i].sum(axis=1, keepdims=True) - t[i])
        with np.errstate(over="ignore"):
            sig = np.where(o[i] > 20.0, 1.0, 1.0 / (1.0 + np.exp(-o[i])))
        dout.append(np.concatenate([dl, (vw / n * (v[i] - y[i]) * sig)[:, None]], axis=1))
    dsum = dout[0] + dout[1]
    wh = np.concatenate([sd["policy_head.weight"], sd["value_head.weight"]], axis=0)
    dwh = np.concatenate([dout[0].T @ hh[0] + dout[1].T @ hh[1], dsum.T @ agg], axis=1)
    dbh = dsum.sum(axis=0)
    g = {"policy_head.weight": dwh[:5], "policy_head.bias": dbh[:5], "value_head.weight": dwh[5:], "value_head.bias": dbh[5:]}
    dh = [dout[i] @ wh[:, :H] + dsum @ wh[:, H:] for i in (0, 1)]

    def bn_back(name, dys, caches):
        """the calls of one module: [dz], and the module's two gradients, P1's contribution before P2's"""
        res = [_bn_backward(dy, sd[f"{name}.weight"], c) for dy, c in zip(dys, caches)]
        g[f"{name}.weight"] = sum(r[1] for r in res)
        g[f"{name}.bias"] = sum(r[2] for r in res)
        return [r[0] for r in res]

    def lin_back(name, dzs, ins):
        g[f"{name}.weight"] = sum(dz.T @ a for dz, a in zip(dzs, ins))
        g[f"{name}.bias"] = sum(dz.sum(axis=0) for dz in dzs)
        return [dz @ sd[f"{name}.weight"] for dz in dzs]

    dy5 = [dh[i] * (y5[i] > 0) for i in (0, 1)]
    dz4 = bn_back("trunk.5", dy5, c5)
    da1 = lin_back("trunk.4", dz4, a1)
    dz0 = bn_back("trunk.1", [da1[i] * (y1[i] > 0) for i in (0, 1)], c1)
    dcat = lin_back("trunk.0", dz0, cat)
    dshared = dcat[0][:, :H] + dcat[1][:, :H]
    dzp = bn_back("player_encoder.1", [dcat[i][:, H:] * (yp[i] > 0) for i in (0, 1)], cp)
    lin_back("player_encoder.0", dzp, xp)
    dzs = bn_back("shared_encoder.1", [dshared * (ys > 0)], [cs])
    lin_back("shared_encoder.0", dzs, [xs])
    running = {}
    for name, caches in (("shared_encoder.1", [cs]), ("player_encoder.1", cp), ("trunk.1", c1), ("trunk.5", c5)):
        rm, rv = sd[f"{name}.running_mean"], sd[f"{name}.running_var"]
        for c in caches:
            rm = (1 - MOMENTUM) * rm + MOMENTUM * c[2]
            rv = (1 - MOMENTUM) * rv + MOMENTUM * c[3] * n / (n - 1)
        running[f"{name}.running_mean"], running[f"{name}.running_var"] = rm, rv
    return dict(losses=dict(zip(LOSS_KEYS, (loss_p[0], loss_p[1], loss_v[0], loss_v[1], loss_value, loss))),
                logits_p1=l[0], logits_p2=l[1], value_p1=v[0], value_p2=v[1], grads=g, running=running,
                bn_out=[ys, yp[0], yp[1], y1[0], y1[1], y5[0], y5[1]], shared_raw=xs, p_raw=xp,
                head_out=np.concatenate([l[0], l[1], o[0][:, None], o[1][:, None]], axis=1),
                dout=np.concatenate([dout[0][:, :5], dout[1][:, :5], dout[0][:, 5:], dout[1][:, 5:]], axis=1), dh=dh, wh=wh)


def relu_margin(case: dict, result: dict | None = None) -> float:
    """The smallest |y| over the seven BatchNorm outputs: how far every ReLU of the case is from flipping."""
    r = result if result is not None else step(case)
    return float(min(np.abs(b).min() for b in r["bn_out"]))
