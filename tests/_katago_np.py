"""KataGoCNN (architecture ``cnn_katago``) in eval mode, in numpy (float64 unless ``dtype`` says float32), from the tensors of a weight blob.

A statement of the network the HIP kernel evaluates (k_cnn_mfma's KataGo instantiation): the seven input planes
(maze 4, cheese, p1 one-hot, p2 one-hot), the six scalars in the flat layout's order added to the stem through the
scalar encoder, the PyRatCNN trunk blocks, mean and max over the board, pool_mlp, and one policy row of 10 logits
(P1: 0-4, P2: 5-9) plus two value logits through softplus. Used on CPU to pin the plane order, the scalar order
and the head split against the golden vectors before any GPU run."""
from __future__ import annotations

import numpy as np


def _bn(t, p, x):
    a = t[p + ".weight"] / np.sqrt(t[p + ".running_var"] + t[p + ".running_var"].dtype.type(1e-5))
    c = t[p + ".bias"] - t[p + ".running_mean"] * a
    return x * a[None, :, None, None] + c[None, :, None, None]


def _conv3x3(x, w):
    n, ci, h, wd = x.shape
    xp = np.zeros((n, ci, h + 2, wd + 2), x.dtype)
    xp[:, :, 1:-1, 1:-1] = x
    out = np.zeros((n, w.shape[0], h, wd), x.dtype)
    for dy in range(3):
        for dx in range(3):
            out += np.einsum("nchw,oc->nohw", xp[:, :, dy:dy + h, dx:dx + wd], w[:, :, dy, dx])
    return out


def _relu(x):
    return np.maximum(x, x.dtype.type(0))


def forward(tensors: dict, width: int, height: int, obs: np.ndarray, dtype=np.float64, taps: dict | None = None) -> dict:
    """`taps`, if given, receives the heads' inputs per player: taps["policy"], taps["value"] = [p1's, p2's]"""
    t = {k: np.asarray(v, dtype) for k, v in tensors.items()}
    obs = np.asarray(obs, dtype)
    n, hw = obs.shape[0], width * height
    maze = obs[:, : hw * 4].reshape(n, height, width, 4).transpose(0, 3, 1, 2)
    p1 = obs[:, hw * 4: hw * 5].reshape(n, 1, height, width)
    p2 = obs[:, hw * 5: hw * 6].reshape(n, 1, height, width)
    cheese = obs[:, hw * 6: hw * 7].reshape(n, 1, height, width)
    planes = np.concatenate([maze, cheese, p1, p2], axis=1)
    scalars = obs[:, hw * 7: hw * 7 + 6]
    x = _conv3x3(planes, t["stem.weight"])
    x = x + (scalars @ t["scalar_encoder.weight"].T + t["scalar_encoder.bias"])[:, :, None, None]
    x = _relu(_bn(t, "stem_bn", x))
    i = 0
    while f"blocks.{i}.conv1.weight" in t:
        p = f"blocks.{i}"
        r = _conv3x3(_relu(_bn(t, p + ".bn1", x)), t[p + ".conv1.weight"])
        r = _conv3x3(_relu(_bn(t, p + ".bn2", r)), t[p + ".conv2.weight"])
        if p + ".pool_conv.weight" in t:
            u = np.einsum("nchw,gc->nghw", _relu(_bn(t, p + ".pool_bn", x)), t[p + ".pool_conv.weight"][:, :, 0, 0])
            cat = np.concatenate([u.mean(axis=(2, 3)), u.max(axis=(2, 3))], axis=1)
            r = r + (cat @ t[p + ".pool_linear.weight"].T + t[p + ".pool_linear.bias"])[:, :, None, None]
        x = r + x
        i += 1
    pooled = np.concatenate([x.mean(axis=(2, 3)), x.max(axis=(2, 3))], axis=1)
    hid = _relu(pooled @ t["pool_mlp.0.weight"].T + t["pool_mlp.0.bias"])
    if taps is not None:
        taps["policy"] = taps["value"] = [hid, hid]
    pol = hid @ t["policy_head.weight"].T + t["policy_head.bias"]
    val = hid @ t["value_head.weight"].T + t["value_head.bias"]

    def softmax(z):
        e = np.exp(z - z.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)

    return dict(logits_p1=pol[:, :5], logits_p2=pol[:, 5:], policy_p1=softmax(pol[:, :5]),
                policy_p2=softmax(pol[:, 5:]), value_p1=np.logaddexp(val.dtype.type(0), val[:, 0]),
                value_p2=np.logaddexp(val.dtype.type(0), val[:, 1]))
