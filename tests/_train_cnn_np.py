"""One training step of PyRatCNN in float64 NumPy -- test infrastructure only.

A restatement, written from their text, of alpharat/nn/models/cnn/model.py (``_parse_obs`` and ``forward`` with
BatchNorm2d in training mode, dropout 0), alpharat/nn/models/cnn/blocks.py ``ResBlock``, alpharat/nn/models/cnn/heads.py
``MLPPolicyHead`` and ``PointValueHead``, alpharat/nn/architectures/cnn/loss.py (``compute_cnn_losses``) and what
``loss.backward()`` leaves in the ``.grad`` tensors. It is tied to the reference by tests/golden/train_cnn
(tools/gen_train_cnn_golden.py runs the reference's own model, loss and autograd in float64); tests/test_train_cnn_np.py
checks every array.

Activations are channels-last here, ``(n, h, w, C)``; the weights keep torch's ``(Cout, Cin, 3, 3)``. A *case* is
tests/_train_np.py's, with ``width`` and ``height`` and a PyRatCNN state dict under ``sd``.
"""
from __future__ import annotations

import numpy as np

from _train_np import EPS, LOSS_KEYS, MOMENTUM, OUT_KEYS, _f64, _log_softmax, _softplus  # noqa: F401

BLOCK_KEYS = ("bn1.weight", "bn1.bias", "conv1.weight", "bn2.weight", "bn2.bias", "conv2.weight")
TAIL_KEYS = ("player_encoder.0.weight", "player_encoder.0.bias", "combiner.0.weight", "combiner.0.bias",
             "policy_head.linear.weight", "policy_head.linear.bias", "value_head.linear.weight", "value_head.linear.bias")


def param_keys(n_blocks: int) -> tuple:
    return (("stem.weight", "stem_bn.weight", "stem_bn.bias") + tuple(f"blocks.{b}.{k}" for b in range(n_blocks) for k in BLOCK_KEYS)
            + TAIL_KEYS)


def bn_modules(n_blocks: int) -> tuple:
    return ("stem_bn",) + tuple(f"blocks.{b}.{bn}" for b in range(n_blocks) for bn in ("bn1", "bn2"))


def running_keys(n_blocks: int) -> tuple:
    return tuple(f"{bn}.{s}" for bn in bn_modules(n_blocks) for s in ("running_mean", "running_var"))


def n_blocks_of(sd: dict) -> int:
    return 1 + max((int(k.split(".")[1]) for k in sd if k.startswith("blocks.")), default=-1)


def layer_weight(key: str) -> str:
    """the weight whose gradient sets the floor of a tensor's tolerance (tests/_train.py grad_bounds)"""
    return key.rsplit(".", 1)[0] + ".weight"


def parse_obs(x, width: int, height: int):
    """(spatial (n, h, w, 5), [side_1, side_2] (n, 3), [mask_1, mask_2] (n, hw)) of flat rows: ``_parse_obs``"""
    hw, n = width * height, len(x)
    sc = x[:, 7 * hw:]
    spatial = np.concatenate([x[:, :4 * hw].reshape(n, height, width, 4), x[:, 6 * hw:7 * hw].reshape(n, height, width, 1)], axis=3)
    sides = [np.stack([sc[:, 4 + p], sc[:, 2 + p], sc[:, 1]], axis=1) for p in (0, 1)]
    masks = [x[:, (4 + p) * hw:(5 + p) * hw] for p in (0, 1)]
    return spatial, sides, masks


def _pad(a):
    return np.pad(a, ((0, 0), (1, 1), (1, 1), (0, 0)))


def conv3(a, w):
    """out[y][x][co] = sum W[co][ci][ky][kx] in[y + ky - 1][x + kx - 1][ci], zero outside the board"""
    n, h, wd, _ = a.shape
    ap = _pad(a)
    return sum(ap[:, ky:ky + h, kx:kx + wd, :] @ w[:, :, ky, kx].T for ky in range(3) for kx in range(3))


def conv3_backward(dout, a, w):
    """(dIn, dW): dIn[y][x][ci] = sum W[co][ci][ky][kx] dOut[y - ky + 1][x - kx + 1][co]; dW = sum dOut[y][x] in[y + ky - 1][x + kx - 1]"""
    n, h, wd, _ = a.shape
    ap, dp = _pad(a), _pad(dout)
    din = sum(dp[:, 2 - ky:2 - ky + h, 2 - kx:2 - kx + wd, :] @ w[:, :, ky, kx] for ky in range(3) for kx in range(3))
    dw = np.zeros_like(w)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = np.einsum("nyxo,nyxi->oi", dout, ap[:, ky:ky + h, kx:kx + wd, :])
    return din, dw


def _bn2_forward(z, gamma, beta):
    """BatchNorm2d in training mode over (n, h, w) of a channels-last array"""
    mu = z.mean(axis=(0, 1, 2))
    var = ((z - mu) ** 2).mean(axis=(0, 1, 2))
    rstd = 1.0 / np.sqrt(var + EPS)
    xhat = (z - mu) * rstd
    return gamma * xhat + beta, (xhat, rstd, mu, var)


def _bn2_backward(dy, gamma, cache):
    xhat, rstd, _, _ = cache
    dxhat = dy * gamma
    dz = rstd * (dxhat - dxhat.mean(axis=(0, 1, 2)) - xhat * (dxhat * xhat).mean(axis=(0, 1, 2)))
    return dz, (dy * xhat).sum(axis=(0, 1, 2)), dy.sum(axis=(0, 1, 2))


def step(case: dict) -> dict:
    """``losses``, the four outputs, ``grads`` (param_keys), ``running`` (running_keys after the update) and ``pre``, every
    array in front of a ReLU (the 1 + 2 B BatchNorm outputs, then the encoder's and the combiner's pre-activations of both
    players); all float64."""
    sd = {k: _f64(v) for k, v in case["sd"].items() if np.issubdtype(np.asarray(v).dtype, np.floating)}
    B = n_blocks_of(sd)
    x = _f64(case["observation"])
    t = [_f64(case["policy_p1"]), _f64(case["policy_p2"])]
    y = [_f64(case["value_p1"]).reshape(-1), _f64(case["value_p2"]).reshape(-1)]
    pw, vw = float(case["policy_weight"]), float(case["value_weight"])
    n, width, height = len(x), int(case["width"]), int(case["height"])
    hw = width * height
    spatial, sides, masks = parse_obs(x, width, height)
    lin = lambda name, a: a @ sd[f"{name}.weight"].T + sd[f"{name}.bias"]  # noqa: E731
    bn = lambda name, z: _bn2_forward(z, sd[f"{name}.weight"], sd[f"{name}.bias"])  # noqa: E731
    caches, pre = {}, []
    # forward: the trunk
    zs = conv3(spatial, sd["stem.weight"])
    ys, caches["stem_bn"] = bn("stem_bn", zs)
    pre.append(ys)
    xs = [np.maximum(ys, 0.0)]
    blocks = []
    for b in range(B):
        y1, caches[f"blocks.{b}.bn1"] = bn(f"blocks.{b}.bn1", xs[b])
        a1 = np.maximum(y1, 0.0)
        z1 = conv3(a1, sd[f"blocks.{b}.conv1.weight"])
        y2, caches[f"blocks.{b}.bn2"] = bn(f"blocks.{b}.bn2", z1)
        a2 = np.maximum(y2, 0.0)
        xs.append(conv3(a2, sd[f"blocks.{b}.conv2.weight"]) + xs[b])
        blocks.append((y1, a1, y2, a2))
        pre += [y1, y2]
    feat = xs[B].reshape(n, hw, -1)
    C = feat.shape[2]
    # the player cells and the heads
    f = [(feat * masks[i][:, :, None]).sum(axis=1) for i in (0, 1)]
    ze = [lin("player_encoder.0", sides[i]) for i in (0, 1)]
    cat = [np.concatenate([f[i], np.maximum(ze[i], 0.0)], axis=1) for i in (0, 1)]
    zc = [lin("combiner.0", cat[i]) for i in (0, 1)]
    pre += [ze[0], ze[1], zc[0], zc[1]]
    hh = [np.maximum(zc[i], 0.0) for i in (0, 1)]
    H = hh[0].shape[1]
    agg = hh[0] + hh[1]
    hcat = [np.concatenate([hh[i], agg], axis=1) for i in (0, 1)]
    l = [lin("policy_head.linear", hcat[i]) for i in (0, 1)]
    o = [lin("value_head.linear", hcat[i])[:, 0] for i in (0, 1)]
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
    wh = np.concatenate([sd["policy_head.linear.weight"], sd["value_head.linear.weight"]], axis=0)
    dwh = np.concatenate([dout[0].T @ hh[0] + dout[1].T @ hh[1], dsum.T @ agg], axis=1)
    dbh = dsum.sum(axis=0)
    g = {"policy_head.linear.weight": dwh[:5], "policy_head.linear.bias": dbh[:5], "value_head.linear.weight": dwh[5:],
         "value_head.linear.bias": dbh[5:]}
    dh = [dout[i] @ wh[:, :H] + dsum @ wh[:, H:] for i in (0, 1)]
    dzc = [dh[i] * (zc[i] > 0) for i in (0, 1)]
    g["combiner.0.weight"] = dzc[0].T @ cat[0] + dzc[1].T @ cat[1]
    g["combiner.0.bias"] = dzc[0].sum(axis=0) + dzc[1].sum(axis=0)
    dcat = [dzc[i] @ sd["combiner.0.weight"] for i in (0, 1)]
    dze = [dcat[i][:, C:] * (ze[i] > 0) for i in (0, 1)]
    g["player_encoder.0.weight"] = dze[0].T @ sides[0] + dze[1].T @ sides[1]
    g["player_encoder.0.bias"] = dze[0].sum(axis=0) + dze[1].sum(axis=0)
    grad = (masks[0][:, :, None] * dcat[0][:, None, :C] + masks[1][:, :, None] * dcat[1][:, None, :C]).reshape(n, height, width, C)
    # the trunk
    for b in range(B - 1, -1, -1):
        y1, a1, y2, a2 = blocks[b]
        name = f"blocks.{b}"
        da2, g[f"{name}.conv2.weight"] = conv3_backward(grad, a2, sd[f"{name}.conv2.weight"])
        dz1, g[f"{name}.bn2.weight"], g[f"{name}.bn2.bias"] = _bn2_backward(da2 * (y2 > 0), sd[f"{name}.bn2.weight"], caches[f"{name}.bn2"])
        da1, g[f"{name}.conv1.weight"] = conv3_backward(dz1, a1, sd[f"{name}.conv1.weight"])
        dx, g[f"{name}.bn1.weight"], g[f"{name}.bn1.bias"] = _bn2_backward(da1 * (y1 > 0), sd[f"{name}.bn1.weight"], caches[f"{name}.bn1"])
        grad = grad + dx
    dzs, g["stem_bn.weight"], g["stem_bn.bias"] = _bn2_backward(grad * (ys > 0), sd["stem_bn.weight"], caches["stem_bn"])
    _, g["stem.weight"] = conv3_backward(dzs, spatial, sd["stem.weight"])
    R = n * hw
    running = {}
    for name in bn_modules(B):
        c = caches[name]
        running[f"{name}.running_mean"] = (1 - MOMENTUM) * sd[f"{name}.running_mean"] + MOMENTUM * c[2]
        running[f"{name}.running_var"] = (1 - MOMENTUM) * sd[f"{name}.running_var"] + MOMENTUM * c[3] * R / (R - 1)
    return dict(losses=dict(zip(LOSS_KEYS, (loss_p[0], loss_p[1], loss_v[0], loss_v[1], loss_value, loss))),
                logits_p1=l[0], logits_p2=l[1], value_p1=v[0], value_p2=v[1], grads=g, running=running, pre=pre)


def relu_margin(case: dict, result: dict | None = None) -> float:
    """The smallest |value| in front of any ReLU of the case: how far every ReLU is from flipping."""
    r = result if result is not None else step(case)
    return float(min(np.abs(a).min() for a in r["pre"]))


def random_cnn(width: int, height: int, C: int, PD: int, HD: int, B: int, seed: int, decided: bool = True) -> dict:
    """A PyRatCNN state dict of float32 arrays. ``decided``: a network whose ReLU signs do not hang on rounding -- every
    BatchNorm beta is +4 or -4, drawn per channel, gamma in [0.25, 0.75]; the two Linear layers in front of a ReLU have
    weights scaled by 0.1 and biases of +-4. Otherwise gamma in [0.5, 1.5], beta and the biases normal at 0.5."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, np.float32)  # noqa: E731
    sign = lambda k: rng.choice([-4.0, 4.0], size=k)  # noqa: E731
    sd = {"stem.weight": f32(rng.standard_normal((C, 5, 3, 3)) * np.sqrt(2.0 / 45))}
    for name in bn_modules(B):
        sd[f"{name}.weight"] = f32(rng.uniform(0.25, 0.75, C) if decided else rng.uniform(0.5, 1.5, C))
        sd[f"{name}.bias"] = f32(sign(C) if decided else rng.standard_normal(C) * 0.5)
        sd[f"{name}.running_mean"] = f32(rng.standard_normal(C) * 0.1)
        sd[f"{name}.running_var"] = f32(rng.uniform(0.5, 1.5, C))
    for b in range(B):
        for conv in ("conv1", "conv2"):
            sd[f"blocks.{b}.{conv}.weight"] = f32(rng.standard_normal((C, C, 3, 3)) * np.sqrt(2.0 / (9 * C)))
    scale = 0.1 if decided else 1.0
    sd["player_encoder.0.weight"] = f32(rng.standard_normal((PD, 3)) * np.sqrt(2.0 / 3) * scale)
    sd["player_encoder.0.bias"] = f32(sign(PD) if decided else rng.standard_normal(PD) * 0.5)
    sd["combiner.0.weight"] = f32(rng.standard_normal((HD, C + PD)) * np.sqrt(2.0 / (C + PD)) * scale)
    sd["combiner.0.bias"] = f32(sign(HD) if decided else rng.standard_normal(HD) * 0.5)
    sd["policy_head.linear.weight"] = f32(rng.standard_normal((5, 2 * HD)) * 0.2)
    sd["policy_head.linear.bias"] = f32(rng.standard_normal(5) * 0.1)
    sd["value_head.linear.weight"] = f32(rng.standard_normal((1, 2 * HD)) * 0.2)
    sd["value_head.linear.bias"] = f32(rng.standard_normal(1) * 0.1)
    return sd
