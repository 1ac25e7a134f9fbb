"""PyRatCNN (architecture ``cnn``) in eval mode, in numpy (float64 unless ``dtype`` says float32), from the tensors
of a weight blob.

A statement of the network k_cnn / k_cnn_mfma evaluate, after alpharat/nn/models/cnn/model.py (PyRatCNN.forward,
_parse_obs), blocks.py (ResBlock, GPoolResBlock) and heads.py (MLPPolicyHead, PointValueHead, PooledValueHead):

- five input planes (maze 4, cheese) through the bias-free 3x3 stem, stem_bn, ReLU (model.py:182);
- pre-activation blocks ``BN ReLU conv BN ReLU conv + x`` (blocks.py:23-29); a block with ``pool_conv`` adds
  ``pool_linear([mean, max] of pool_conv(ReLU(pool_bn(x))))`` to every cell (blocks.py:58-79);
- the trunk's features at each player's cell (the one-hot position mask times the feature map, model.py:188-190);
- player_encoder over [score, mud, progress], combiner over [features, encoding], both ReLU (model.py:193-198);
- DeepSet heads over [h_i, h_1 + h_2]: policy_head.linear (heads.py:21), and either value_head.linear
  (PointValueHead, heads.py:37) or value_head.mlp over [mean, max of the trunk, h_i, agg] (PooledValueHead,
  heads.py:63-67), both through softplus.

The oracle's forward keeps f32 activations; this is the float64 side the GPU tests at saturated outputs compare both
against. Pinned on CPU against every tests/golden/nets/cnn_*.npz (tests/test_saturated_nets_cpu.py)."""
from __future__ import annotations

import numpy as np

from _katago_np import _bn, _conv3x3, _relu


def forward(tensors: dict, width: int, height: int, obs: np.ndarray, dtype=np.float64, taps: dict | None = None) -> dict:
    """`taps`, if given, receives the heads' inputs per player: taps["policy"], taps["value"] = [p1's, p2's]; the value
    head's input is that of its last layer"""
    t = {k: np.asarray(v, dtype) for k, v in tensors.items()}
    obs = np.asarray(obs, dtype)
    n, hw = obs.shape[0], width * height
    maze = obs[:, : hw * 4].reshape(n, height, width, 4).transpose(0, 3, 1, 2)
    mask = [obs[:, hw * 4: hw * 5], obs[:, hw * 5: hw * 6]]
    cheese = obs[:, hw * 6: hw * 7].reshape(n, 1, height, width)
    sc = obs[:, hw * 7: hw * 7 + 6]  # score diff, progress, p1 mud, p2 mud, p1 score, p2 score

    x = _relu(_bn(t, "stem_bn", _conv3x3(np.concatenate([maze, cheese], axis=1), t["stem.weight"])))
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

    flat = x.reshape(n, x.shape[1], hw)
    h = []
    for pl in range(2):
        f = (flat * mask[pl][:, None, :]).sum(axis=2)
        side = np.stack([sc[:, 4 + pl], sc[:, 2 + pl], sc[:, 1]], axis=1)
        e = _relu(side @ t["player_encoder.0.weight"].T + t["player_encoder.0.bias"])
        h.append(_relu(np.concatenate([f, e], axis=1) @ t["combiner.0.weight"].T + t["combiner.0.bias"]))
    agg = h[0] + h[1]
    pool = np.concatenate([x.mean(axis=(2, 3)), x.max(axis=(2, 3))], axis=1)

    cat = [np.concatenate([h[pl], agg], axis=1) for pl in range(2)]
    last = "value_head.linear" if "value_head.linear.weight" in t else "value_head.mlp.2"
    vin = cat if last == "value_head.linear" else [
        _relu(np.concatenate([pool, c], axis=1) @ t["value_head.mlp.0.weight"].T + t["value_head.mlp.0.bias"]) for c in cat]
    if taps is not None:
        taps["policy"], taps["value"] = cat, vin
    val = [(v @ t[last + ".weight"].T + t[last + ".bias"])[:, 0] for v in vin]

    def softmax(z):
        e = np.exp(z - z.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)

    lg = [c @ t["policy_head.linear.weight"].T + t["policy_head.linear.bias"] for c in cat]
    zero = obs.dtype.type(0)
    return dict(logits_p1=lg[0], logits_p2=lg[1], policy_p1=softmax(lg[0]), policy_p2=softmax(lg[1]),
                value_p1=np.logaddexp(zero, val[0]), value_p2=np.logaddexp(zero, val[1]))
