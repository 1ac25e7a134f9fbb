"""One training step of PyRatCNN with GPoolResBlocks and dropout, in float64 NumPy -- test infrastructure only.

tests/_train_cnn_np.py with what alpharat/nn/models/cnn/blocks.py ``GPoolResBlock`` adds to a block -- ``pool =
pool_conv(relu(pool_bn(x)))``, ``pool_cat = [pool.mean((2, 3)) | pool.amax((2, 3))]``, ``out = regular +
pool_linear(pool_cat)[:, :, None, None] + identity`` -- and with ``nn.Dropout`` in training mode behind the ReLU of
``player_encoder`` and of ``combiner`` (alpharat/nn/models/cnn/model.py), the mask given from outside as in
tests/_train_dropout_np.py. ``amax``'s backward shares the gradient evenly among the cells that equal the maximum, as torch
does. The helpers and the layout (channels-last activations, torch's weight shapes) are tests/_train_cnn_np.py's. It is
tied to the reference by tests/golden/train_gpool (tools/gen_train_gpool_golden.py); tests/test_train_gpool_np.py checks every
array, and that a network of ResBlocks without masks gives tests/_train_cnn_np.py's own result exactly.

A *case* is tests/_train_cnn_np.py's; a block is a gpool block iff the state dict has its ``pool_conv.weight``. With
dropout it also has ``masks`` -- four bool arrays, tests/_dropout_np.py CNN_CALLS: ``player_encoder`` on P1's and P2's rows
``(n, PD)``, ``combiner`` on P1's and P2's rows ``(n, HD)`` -- and ``scale`` (1 / (1 - p) as the library rounds it).
"""
from __future__ import annotations

import numpy as np

import _dropout_np as D
import _train_cnn_np as NC
from _train_cnn_np import LOSS_KEYS, MOMENTUM, OUT_KEYS, _bn2_backward, _bn2_forward, _f64, _log_softmax, _softplus, conv3, conv3_backward

POOL_KEYS = ("pool_bn.weight", "pool_bn.bias", "pool_conv.weight", "pool_linear.weight", "pool_linear.bias")
CNN_CALLS = ("player_encoder/p1", "player_encoder/p2", "combiner/p1", "combiner/p2")  # the dropout's call indices


def blocks_of(sd: dict) -> tuple:
    """gpool_channels per block, 0 for a ResBlock"""
    return tuple(int(sd[f"blocks.{b}.pool_conv.weight"].shape[0]) if f"blocks.{b}.pool_conv.weight" in sd else 0
                 for b in range(NC.n_blocks_of(sd)))


def param_keys(blocks) -> tuple:
    plain = NC.param_keys(0)
    return (plain[:3] + tuple(f"blocks.{b}.{k}" for b, g in enumerate(blocks) for k in NC.BLOCK_KEYS + (POOL_KEYS if g else ()))
            + plain[3:])


def bn_modules(blocks) -> tuple:
    return ("stem_bn",) + tuple(f"blocks.{b}.{bn}" for b, g in enumerate(blocks) for bn in ("bn1", "bn2") + (("pool_bn",) if g else ()))


def running_keys(blocks) -> tuple:
    return tuple(f"{bn}.{s}" for bn in bn_modules(blocks) for s in ("running_mean", "running_var"))


def layer_weight(key: str) -> str:
    """the weight whose gradient sets the floor of a tensor's tolerance: the same layer's, so ``pool_bn.weight`` for
    ``pool_bn.*``, ``pool_conv.weight`` for itself and ``pool_linear.weight`` for ``pool_linear.*``"""
    return key.rsplit(".", 1)[0] + ".weight"


def with_masks(case: dict, seed: int, step: int, p: float) -> dict:
    """the case with the masks of (seed, step) at rate p and the library's scale"""
    n, sd = len(case["observation"]), case["sd"]
    PD, HD = sd["player_encoder.0.weight"].shape[0], sd["combiner.0.weight"].shape[0]
    masks = [D.mask(seed, step, call, n, PD if call < 2 else HD, p) for call in range(4)]
    return dict(case, masks=masks, scale=float(D.scale(p)), p=float(np.float32(p)), dropout_seed=int(seed), dropout_step=int(step))


def step(case: dict) -> dict:
    """tests/_train_cnn_np.py ``step`` with gpool blocks and masks. ``pre``: every array in front of a ReLU (stem_bn, per
    block bn1, bn2 and pool_bn, then the encoder's and the combiner's pre-activations); ``pz``: every gpool block's
    ``pool_conv`` output ``(n, hw, G)``, what the maximum is taken over; ``pool_back``: per gpool block, from the last one
    down, ``dcat (n, 2G)``, pool_bn's ``xhat (n, hw, C)`` and ``pool_conv.weight`` as ``wc (G, C)``."""
    sd = {k: _f64(v) for k, v in case["sd"].items() if np.issubdtype(np.asarray(v).dtype, np.floating)}
    blocks = blocks_of(sd)
    B = len(blocks)
    x = _f64(case["observation"])
    t = [_f64(case["policy_p1"]), _f64(case["policy_p2"])]
    y = [_f64(case["value_p1"]).reshape(-1), _f64(case["value_p2"]).reshape(-1)]
    pw, vw = float(case["policy_weight"]), float(case["value_weight"])
    n, width, height = len(x), int(case["width"]), int(case["height"])
    hw = width * height
    if case.get("masks") is not None:
        drop = [np.asarray(m, np.float64) * float(case["scale"]) for m in case["masks"]]
    else:
        drop = [1.0] * 4
    spatial, sides, masks = NC.parse_obs(x, width, height)
    lin = lambda name, a: a @ sd[f"{name}.weight"].T + sd[f"{name}.bias"]  # noqa: E731
    bn = lambda name, z: _bn2_forward(z, sd[f"{name}.weight"], sd[f"{name}.bias"])  # noqa: E731
    caches, pre, pzs, pool_back = {}, [], [], []
    zs = conv3(spatial, sd["stem.weight"])
    ys, caches["stem_bn"] = bn("stem_bn", zs)
    pre.append(ys)
    xs = [np.maximum(ys, 0.0)]
    saved = []
    for b in range(B):
        name = f"blocks.{b}"
        y1, caches[f"{name}.bn1"] = bn(f"{name}.bn1", xs[b])
        a1 = np.maximum(y1, 0.0)
        z1 = conv3(a1, sd[f"{name}.conv1.weight"])
        y2, caches[f"{name}.bn2"] = bn(f"{name}.bn2", z1)
        a2 = np.maximum(y2, 0.0)
        out = conv3(a2, sd[f"{name}.conv2.weight"])
        pre += [y1, y2]
        pool = None
        if blocks[b]:
            G = blocks[b]
            yp, caches[f"{name}.pool_bn"] = bn(f"{name}.pool_bn", xs[b])
            ap = np.maximum(yp, 0.0)
            wc = sd[f"{name}.pool_conv.weight"].reshape(G, -1)
            pz = (ap @ wc.T).reshape(n, hw, G)
            mx = pz.max(axis=1)
            cat = np.concatenate([pz.mean(axis=1), mx], axis=1)
            po = lin(f"{name}.pool_linear", cat)
            out = out + po[:, None, None, :]
            pre.append(yp)
            pzs.append(pz)
            pool = (yp, ap, pz, mx, cat)
        xs.append(out + xs[b])
        saved.append((y1, a1, y2, a2, pool))
    feat = xs[B].reshape(n, hw, -1)
    C = feat.shape[2]
    f = [(feat * masks[i][:, :, None]).sum(axis=1) for i in (0, 1)]
    ze = [lin("player_encoder.0", sides[i]) for i in (0, 1)]
    cat = [np.concatenate([f[i], np.maximum(ze[i], 0.0) * drop[i]], axis=1) for i in (0, 1)]
    zc = [lin("combiner.0", cat[i]) for i in (0, 1)]
    pre += [ze[0], ze[1], zc[0], zc[1]]
    hh = [np.maximum(zc[i], 0.0) * drop[2 + i] for i in (0, 1)]
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
    # backward: the heads
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
    dzc = [dh[i] * drop[2 + i] * (zc[i] > 0) for i in (0, 1)]
    g["combiner.0.weight"] = dzc[0].T @ cat[0] + dzc[1].T @ cat[1]
    g["combiner.0.bias"] = dzc[0].sum(axis=0) + dzc[1].sum(axis=0)
    dcat = [dzc[i] @ sd["combiner.0.weight"] for i in (0, 1)]
    dze = [dcat[i][:, C:] * drop[i] * (ze[i] > 0) for i in (0, 1)]
    g["player_encoder.0.weight"] = dze[0].T @ sides[0] + dze[1].T @ sides[1]
    g["player_encoder.0.bias"] = dze[0].sum(axis=0) + dze[1].sum(axis=0)
    grad = (masks[0][:, :, None] * dcat[0][:, None, :C] + masks[1][:, :, None] * dcat[1][:, None, :C]).reshape(n, height, width, C)
    # the trunk
    for b in range(B - 1, -1, -1):
        y1, a1, y2, a2, pool = saved[b]
        name = f"blocks.{b}"
        da2, g[f"{name}.conv2.weight"] = conv3_backward(grad, a2, sd[f"{name}.conv2.weight"])
        dz1, g[f"{name}.bn2.weight"], g[f"{name}.bn2.bias"] = _bn2_backward(da2 * (y2 > 0), sd[f"{name}.bn2.weight"], caches[f"{name}.bn2"])
        da1, g[f"{name}.conv1.weight"] = conv3_backward(dz1, a1, sd[f"{name}.conv1.weight"])
        dx, g[f"{name}.bn1.weight"], g[f"{name}.bn1.bias"] = _bn2_backward(da1 * (y1 > 0), sd[f"{name}.bn1.weight"], caches[f"{name}.bn1"])
        total = grad + dx
        if pool is not None:
            yp, ap, pz, mx, pcat = pool
            G = blocks[b]
            dpo = grad.reshape(n, hw, C).sum(axis=1)
            g[f"{name}.pool_linear.weight"] = dpo.T @ pcat
            g[f"{name}.pool_linear.bias"] = dpo.sum(axis=0)
            dpcat = dpo @ sd[f"{name}.pool_linear.weight"]
            is_max = pz == mx[:, None, :]
            dpz = dpcat[:, None, :G] / hw + is_max * (dpcat[:, G:] / is_max.sum(axis=1))[:, None, :]
            wc = sd[f"{name}.pool_conv.weight"].reshape(G, -1)
            g[f"{name}.pool_conv.weight"] = (dpz.reshape(-1, G).T @ ap.reshape(-1, C)).reshape(sd[f"{name}.pool_conv.weight"].shape)
            dap = (dpz.reshape(-1, G) @ wc).reshape(ap.shape)
            pool_back.append(dict(block=b, dcat=dpcat, xhat=caches[f"{name}.pool_bn"][0].reshape(n, hw, C), wc=wc))
            dxp, g[f"{name}.pool_bn.weight"], g[f"{name}.pool_bn.bias"] = _bn2_backward(dap * (yp > 0), sd[f"{name}.pool_bn.weight"],
                                                                                       caches[f"{name}.pool_bn"])
            total = total + dxp
        grad = total
    dzs, g["stem_bn.weight"], g["stem_bn.bias"] = _bn2_backward(grad * (ys > 0), sd["stem_bn.weight"], caches["stem_bn"])
    _, g["stem.weight"] = conv3_backward(dzs, spatial, sd["stem.weight"])
    R = n * hw
    running = {}
    for name in bn_modules(blocks):
        c = caches[name]
        running[f"{name}.running_mean"] = (1 - MOMENTUM) * sd[f"{name}.running_mean"] + MOMENTUM * c[2]
        running[f"{name}.running_var"] = (1 - MOMENTUM) * sd[f"{name}.running_var"] + MOMENTUM * c[3] * R / (R - 1)
    return dict(losses=dict(zip(LOSS_KEYS, (loss_p[0], loss_p[1], loss_v[0], loss_v[1], loss_value, loss))),
                logits_p1=l[0], logits_p2=l[1], value_p1=v[0], value_p2=v[1], grads=g, running=running, pre=pre, pz=pzs,
                pool_back=pool_back)


def relu_margin(result: dict) -> float:
    """the smallest |value| in front of any ReLU"""
    return float(min(np.abs(a).min() for a in result["pre"]))


def max_gap(pzs) -> float:
    """the smallest gap, over every (row, channel) of every gpool block, between the largest and the second largest pz of
    the row's cells: how far every maximum is from moving to another cell (inf without a gpool block)"""
    gap = np.inf
    for pz in pzs:
        top = np.sort(np.asarray(pz, np.float64), axis=1)[:, -2:, :]
        gap = min(gap, float((top[:, 1] - top[:, 0]).min()))
    return gap


def random_gpool_cnn(width: int, height: int, C: int, PD: int, HD: int, blocks, seed: int, decided: bool = True) -> dict:
    """tests/_train_cnn_np.py ``random_cnn`` with the pool modules of the gpool blocks (``blocks``: gpool_channels, 0 for a
    ResBlock), drawn from a generator of their own so that the other tensors are that function's"""
    sd = NC.random_cnn(width, height, C, PD, HD, len(blocks), seed, decided)
    rng = np.random.default_rng([seed, 77])
    f32 = lambda a: np.asarray(a, np.float32)  # noqa: E731
    for b, G in enumerate(blocks):
        if not G:
            continue
        name = f"blocks.{b}"
        sd[f"{name}.pool_bn.weight"] = f32(rng.uniform(0.25, 0.75, C) if decided else rng.uniform(0.5, 1.5, C))
        sd[f"{name}.pool_bn.bias"] = f32(rng.choice([-4.0, 4.0], size=C) if decided else rng.standard_normal(C) * 0.5)
        sd[f"{name}.pool_bn.running_mean"] = f32(rng.standard_normal(C) * 0.1)
        sd[f"{name}.pool_bn.running_var"] = f32(rng.uniform(0.5, 1.5, C))
        sd[f"{name}.pool_conv.weight"] = f32(rng.standard_normal((G, C, 1, 1)) * np.sqrt(2.0 / C))
        sd[f"{name}.pool_linear.weight"] = f32(rng.standard_normal((C, 2 * G)) * np.sqrt(1.0 / (2 * G)))
        sd[f"{name}.pool_linear.bias"] = f32(rng.standard_normal(C) * 0.1)
    return sd
