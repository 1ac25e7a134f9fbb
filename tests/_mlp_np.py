"""PyRatMLP (``mlp``) and SymmetricMLP (``symmetric``) in eval mode, in numpy, from the tensors of a weight blob.

Statements of the networks k_mlp_mfma / k_mlp and k_symmetric_mfma2 / k_symmetric evaluate, over the flat observation
(maze[hw*4] p1[hw] p2[hw] cheese[hw], scalars: score diff, progress, p1 mud, p2 mud, p1 score, p2 score). Used on CPU
to pin the oracle's forward, the reference of the GPU tests, on boards the golden vectors do not cover.

``dtype`` (default float64) is the type every tensor, the observation and so every intermediate is held in: float32
gives an evaluation at the reference's own precision, whose distance from the float64 one is the yardstick of
tests/test_gpu_saturated_nets.py."""
from __future__ import annotations

import numpy as np


def _lin(t, p, x):
    return x @ t[p + ".weight"].T + t[p + ".bias"]


def _bn(t, p, x):
    eps = t[p + ".running_var"].dtype.type(1e-5)
    return (x - t[p + ".running_mean"]) / np.sqrt(t[p + ".running_var"] + eps) * t[p + ".weight"] + t[p + ".bias"]


def _block(t, lin, bn, x):
    return np.maximum(_bn(t, bn, _lin(t, lin, x)), 0.0)


def _outputs(l1, l2, v1, v2):
    def softmax(z):
        e = np.exp(z - z.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)

    return dict(logits_p1=l1, logits_p2=l2, policy_p1=softmax(l1), policy_p2=softmax(l2), value_p1=np.logaddexp(v1.dtype.type(0), v1),
                value_p2=np.logaddexp(v2.dtype.type(0), v2))


def mlp_forward(tensors: dict, obs: np.ndarray, dtype=np.float64, taps: dict | None = None) -> dict:
    """`taps`, if given, receives the heads' inputs per player: taps["policy"], taps["value"] = [p1's, p2's]"""
    t = {k: np.asarray(v, dtype) for k, v in tensors.items()}
    x = _block(t, "trunk.4", "trunk.5", _block(t, "trunk.0", "trunk.1", np.asarray(obs, dtype)))
    if taps is not None:
        taps["policy"] = taps["value"] = [x, x]
    v = _lin(t, "value_head", x)
    return _outputs(_lin(t, "policy_p1_head", x), _lin(t, "policy_p2_head", x), v[:, 0], v[:, 1])


def symmetric_forward(tensors: dict, width: int, height: int, obs: np.ndarray, dtype=np.float64,
                      taps: dict | None = None) -> dict:
    t = {k: np.asarray(v, dtype) for k, v in tensors.items()}
    obs = np.asarray(obs, dtype)
    hw = width * height
    sc = obs[:, hw * 7:]
    shared = _block(t, "shared_encoder.0", "shared_encoder.1",
                    np.concatenate([obs[:, : hw * 4], obs[:, hw * 6: hw * 7], sc[:, 1:2]], axis=1))
    h = []
    for p in range(2):
        pe = _block(t, "player_encoder.0", "player_encoder.1",
                    np.concatenate([obs[:, hw * (4 + p): hw * (5 + p)], sc[:, 2 + p: 3 + p], sc[:, 4 + p: 5 + p]], axis=1))
        x = _block(t, "trunk.0", "trunk.1", np.concatenate([shared, pe], axis=1))
        h.append(_block(t, "trunk.4", "trunk.5", x))
    agg = h[0] + h[1]
    cat = [np.concatenate([h[p], agg], axis=1) for p in range(2)]
    if taps is not None:
        taps["policy"] = taps["value"] = cat
    return _outputs(_lin(t, "policy_head", cat[0]), _lin(t, "policy_head", cat[1]), _lin(t, "value_head", cat[0])[:, 0],
                    _lin(t, "value_head", cat[1])[:, 0])
