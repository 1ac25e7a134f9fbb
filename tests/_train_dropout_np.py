"""One training step of PyRatMLP, SymmetricMLP or LocalValueMLP with dropout, in float64 NumPy -- test infrastructure only.

tests/_train_np.py, tests/_train_sym_np.py and tests/_train_lv_np.py with ``nn.Dropout`` in training mode behind every
``BatchNorm1d -> ReLU`` of the encoders and the trunk, the mask given from outside: where the models have
``dropout(relu(y))`` this file has ``relu(y) * mask * scale``, and the backward multiplies the gradient that reaches the
activation by ``mask * scale`` before the ReLU's own mask. The helpers (BatchNorm, softmax, softplus) and the key tuples are
those files'. It is tied to the reference by tests/golden/train_dropout (tools/gen_train_dropout_golden.py runs the
reference's own models with a forward hook on every ``nn.Dropout`` that applies the same masks); tests/test_train_dropout_np.py
checks every array to 1e-12, and that masks of ones with scale 1 give the three files' own results exactly.

A *case* is that of the architecture's own file with ``masks`` -- one bool (n, H) array per BatchNorm call, in the order of
tests/_dropout_np.py MLP_CALLS / SYM_CALLS -- and ``scale`` (1 / (1 - p) as the library rounds it).
"""
from __future__ import annotations

import numpy as np

import _dropout_np as D
import _train_lv_np as NL
import _train_np as N
import _train_sym_np as NS
from _train_np import MOMENTUM, _bn_backward, _bn_forward, _f64, _log_softmax, _softplus


def with_masks(case: dict, seed: int, step: int, p: float, calls: int | None = None) -> dict:
    """the case with the masks of (seed, step) at rate p and the library's scale; p == 0: masks of ones, scale 1"""
    n = len(case["observation"])
    sd = case["sd"]
    H = sd["trunk.4.weight"].shape[0]
    if calls is None:
        calls = len(D.SYM_CALLS) if "shared_encoder.0.weight" in sd else len(D.MLP_CALLS)
    return dict(case, masks=D.masks(seed, step, calls, n, H, p), scale=float(D.scale(p)), p=float(np.float32(p)),
                dropout_seed=int(seed), dropout_step=int(step))


def no_dropout(case: dict, calls: int) -> dict:
    n = len(case["observation"])
    H = case["sd"]["trunk.4.weight"].shape[0]
    return dict(case, masks=[np.ones((n, H), bool)] * calls, scale=1.0)


def _drop(case):
    return [np.asarray(m, np.float64) * float(case["scale"]) for m in case["masks"]]


def _heads_mlp(sd, a2, t1, t2, v1t, v2t, pw, vw, n):
    """PyRatMLP's three heads over the trunk output: outputs, losses, the heads' gradients and their part of d a2"""
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
    dl1 = pw / n * (np.exp(ls1) * t1.sum(axis=1, keepdims=True) - t1)
    dl2 = pw / n * (np.exp(ls2) * t2.sum(axis=1, keepdims=True) - t2)
    with np.errstate(over="ignore"):
        sig = np.where(o > 20.0, 1.0, 1.0 / (1.0 + np.exp(-o)))
    do = vw / n * (v - np.stack([v1t, v2t], axis=1)) * sig
    g = {}
    for name, d in (("policy_p1_head", dl1), ("policy_p2_head", dl2), ("value_head", do)):
        g[f"{name}.weight"] = d.T @ a2
        g[f"{name}.bias"] = d.sum(axis=0)
    da2 = dl1 @ sd["policy_p1_head.weight"] + dl2 @ sd["policy_p2_head.weight"] + do @ sd["value_head.weight"]
    return (l1, l2, v), (loss_p1, loss_p2, loss_v1, loss_v2, loss_value), g, da2


def _mlp_like(case: dict, lv: bool) -> dict:
    sd = {k: _f64(v) for k, v in case["sd"].items() if np.issubdtype(np.asarray(v).dtype, np.floating)}
    x = _f64(case["observation"])
    t1, t2 = _f64(case["policy_p1"]), _f64(case["policy_p2"])
    v1t, v2t = _f64(case["value_p1"]).reshape(-1), _f64(case["value_p2"]).reshape(-1)
    pw, vw = float(case["policy_weight"]), float(case["value_weight"])
    m1, m2 = _drop(case)
    n = len(x)
    z1 = x @ sd["trunk.0.weight"].T + sd["trunk.0.bias"]
    y1, c1 = _bn_forward(z1, sd["trunk.1.weight"], sd["trunk.1.bias"])
    a1 = np.maximum(y1, 0.0) * m1
    z2 = a1 @ sd["trunk.4.weight"].T + sd["trunk.4.bias"]
    y2, c2 = _bn_forward(z2, sd["trunk.5.weight"], sd["trunk.5.bias"])
    a2 = np.maximum(y2, 0.0) * m2
    (l1, l2, v), ls, g, da2 = _heads_mlp(sd, a2, t1, t2, v1t, v2t, pw, vw, n)
    loss = pw * (ls[0] + ls[1]) + vw * ls[4]
    more = {}
    if lv:
        ow = float(case["ownership_weight"])
        co = np.asarray(case["cheese_outcomes"]).reshape(n, -1).astype(np.int64)
        hw = co.shape[1]
        zo = a2 @ sd["ownership_head.0.weight"].T + sd["ownership_head.0.bias"]
        ao = np.maximum(zo, 0.0)
        L = (ao @ sd["ownership_head.2.weight"].T + sd["ownership_head.2.bias"]).reshape(n, hw, 4)
        active = co >= 0
        cells = int(active.sum())
        lso = _log_softmax(L.reshape(-1, 4)).reshape(n, hw, 4)
        target = np.where(active, co, 0)
        ce = -np.take_along_axis(lso, target[:, :, None], axis=2)[:, :, 0]
        loss_own = float((ce * active).sum() / cells) if cells else 0.0
        loss = loss + ow * loss_own
        onehot = np.zeros((n, hw, 4))
        np.put_along_axis(onehot, target[:, :, None], 1.0, axis=2)
        dL = (NL.own_scale(ow, cells) * (np.exp(lso) - onehot) * active[:, :, None]).reshape(n, 4 * hw)
        g["ownership_head.2.weight"], g["ownership_head.2.bias"] = dL.T @ ao, dL.sum(axis=0)
        dzo = (dL @ sd["ownership_head.2.weight"]) * (zo > 0)
        g["ownership_head.0.weight"], g["ownership_head.0.bias"] = dzo.T @ a2, dzo.sum(axis=0)
        da2 = da2 + dzo @ sd["ownership_head.0.weight"]  # the head reads the trunk output behind the last dropout
        h, w = np.asarray(case["cheese_outcomes"]).shape[1:]
        more = dict(ownership_logits=L.reshape(n, h, w, 4), zo=zo, cells=cells)
    dz2, g["trunk.5.weight"], g["trunk.5.bias"] = _bn_backward(da2 * m2 * (y2 > 0), sd["trunk.5.weight"], c2)
    g["trunk.4.weight"], g["trunk.4.bias"] = dz2.T @ a1, dz2.sum(axis=0)
    da1 = dz2 @ sd["trunk.4.weight"]
    dz1, g["trunk.1.weight"], g["trunk.1.bias"] = _bn_backward(da1 * m1 * (y1 > 0), sd["trunk.1.weight"], c1)
    g["trunk.0.weight"], g["trunk.0.bias"] = dz1.T @ x, dz1.sum(axis=0)
    running = {}
    for bn, c in (("trunk.1", c1), ("trunk.5", c2)):
        running[f"{bn}.running_mean"] = (1 - MOMENTUM) * sd[f"{bn}.running_mean"] + MOMENTUM * c[2]
        running[f"{bn}.running_var"] = (1 - MOMENTUM) * sd[f"{bn}.running_var"] + MOMENTUM * c[3] * n / (n - 1)
    losses = dict(zip(N.LOSS_KEYS, (*ls, loss)))
    if lv:
        losses["loss_ownership"] = loss_own
    return dict(losses=losses, logits_p1=l1, logits_p2=l2, value_p1=v[:, 0], value_p2=v[:, 1], grads=g, running=running, y1=y1,
                y2=y2, a1=a1, a2=a2, **more)


def step_mlp(case: dict) -> dict:
    """tests/_train_np.py ``step`` with the case's two masks"""
    return _mlp_like(case, False)


def step_lv(case: dict) -> dict:
    """tests/_train_lv_np.py ``step`` with the case's two masks"""
    return _mlp_like(case, True)


def step_sym(case: dict) -> dict:
    """tests/_train_sym_np.py ``step`` with the case's seven masks"""
    sd = {k: _f64(v) for k, v in case["sd"].items() if np.issubdtype(np.asarray(v).dtype, np.floating)}
    x = _f64(case["observation"])
    t = [_f64(case["policy_p1"]), _f64(case["policy_p2"])]
    y = [_f64(case["value_p1"]).reshape(-1), _f64(case["value_p2"]).reshape(-1)]
    pw, vw = float(case["policy_weight"]), float(case["value_weight"])
    m = _drop(case)
    ms, mp, m1, m5 = m[0], m[1:3], m[3:5], m[5:7]
    n = len(x)
    H = sd["trunk.4.weight"].shape[0]
    lin = lambda name, a: a @ sd[f"{name}.weight"].T + sd[f"{name}.bias"]  # noqa: E731
    bn = lambda name, z: _bn_forward(z, sd[f"{name}.weight"], sd[f"{name}.bias"])  # noqa: E731
    xs, xp = NS.split_inputs(x, int(case["width"]), int(case["height"]))
    ys, cs = bn("shared_encoder.1", lin("shared_encoder.0", xs))
    shared = np.maximum(ys, 0.0) * ms
    yp, cp, pe, cat, y1, c1, a1, y5, c5, hh = ([None, None] for _ in range(10))
    for i in (0, 1):
        yp[i], cp[i] = bn("player_encoder.1", lin("player_encoder.0", xp[i]))
        pe[i] = np.maximum(yp[i], 0.0) * mp[i]
        cat[i] = np.concatenate([shared, pe[i]], axis=1)
        y1[i], c1[i] = bn("trunk.1", lin("trunk.0", cat[i]))
        a1[i] = np.maximum(y1[i], 0.0) * m1[i]
        y5[i], c5[i] = bn("trunk.5", lin("trunk.4", a1[i]))
        hh[i] = np.maximum(y5[i], 0.0) * m5[i]
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
        res = [_bn_backward(dy, sd[f"{name}.weight"], c) for dy, c in zip(dys, caches)]
        g[f"{name}.weight"] = sum(r[1] for r in res)
        g[f"{name}.bias"] = sum(r[2] for r in res)
        return [r[0] for r in res]

    def lin_back(name, dzs, ins):
        g[f"{name}.weight"] = sum(dz.T @ a for dz, a in zip(dzs, ins))
        g[f"{name}.bias"] = sum(dz.sum(axis=0) for dz in dzs)
        return [dz @ sd[f"{name}.weight"] for dz in dzs]

    dz4 = bn_back("trunk.5", [dh[i] * m5[i] * (y5[i] > 0) for i in (0, 1)], c5)
    da1 = lin_back("trunk.4", dz4, a1)
    dz0 = bn_back("trunk.1", [da1[i] * m1[i] * (y1[i] > 0) for i in (0, 1)], c1)
    dcat = lin_back("trunk.0", dz0, cat)
    dshared = dcat[0][:, :H] + dcat[1][:, :H]
    dzp = bn_back("player_encoder.1", [dcat[i][:, H:] * mp[i] * (yp[i] > 0) for i in (0, 1)], cp)
    lin_back("player_encoder.0", dzp, xp)
    dzs = bn_back("shared_encoder.1", [dshared * ms * (ys > 0)], [cs])
    lin_back("shared_encoder.0", dzs, [xs])
    running = {}
    for name, caches in (("shared_encoder.1", [cs]), ("player_encoder.1", cp), ("trunk.1", c1), ("trunk.5", c5)):
        rm, rv = sd[f"{name}.running_mean"], sd[f"{name}.running_var"]
        for c in caches:
            rm = (1 - MOMENTUM) * rm + MOMENTUM * c[2]
            rv = (1 - MOMENTUM) * rv + MOMENTUM * c[3] * n / (n - 1)
        running[f"{name}.running_mean"], running[f"{name}.running_var"] = rm, rv
    return dict(losses=dict(zip(N.LOSS_KEYS, (loss_p[0], loss_p[1], loss_v[0], loss_v[1], loss_value, loss))),
                logits_p1=l[0], logits_p2=l[1], value_p1=v[0], value_p2=v[1], grads=g, running=running,
                bn_out=[ys, yp[0], yp[1], y1[0], y1[1], y5[0], y5[1]], acts=[shared, pe[0], pe[1], a1[0], a1[1], hh[0], hh[1]])


STEPS = dict(mlp=step_mlp, symmetric=step_sym, local_value=step_lv)
PLAIN = dict(mlp=N, symmetric=NS, local_value=NL)


def relu_margin(arch: str, case: dict, result: dict | None = None) -> float:
    """The smallest |.| in front of any ReLU of the case, with its masks applied: how far every ReLU is from flipping."""
    r = result if result is not None else STEPS[arch](case)
    if arch == "symmetric":
        return float(min(np.abs(b).min() for b in r["bn_out"]))
    m = min(np.abs(r["y1"]).min(), np.abs(r["y2"]).min())
    return float(min(m, np.abs(r["zo"]).min()) if arch == "local_value" else m)
