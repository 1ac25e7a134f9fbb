"""The ownership head of LocalValueMLP and its loss in float64 numpy -- test infrastructure only.

Restates, for the tests of ar_rows_validate_lv:
  alpharat/nn/models/local_value.py:103-107, 182-193   ownership_head, ownership_value      -> head_forward, row_terms
  alpharat/nn/losses/ownership.py:26-46                compute_ownership_loss               -> loss_ownership
  alpharat/nn/training/loop.py (GPUMetricsAccumulator) batch means weighted by batch size   -> batch_weighted
tests/test_ownership_np.py ties these to the reference's own numbers under tests/golden/ownership.

Targets are the rows' ``cheese_outcomes`` as a shard holds them: the game's outcome where the position still has the
cheese, -1 elsewhere. Cells are row-major (y * width + x), four class logits each.
"""
from __future__ import annotations

import numpy as np

import _mlp_np

OWN_KEYS = ("ownership_head.0.weight", "ownership_head.0.bias", "ownership_head.2.weight", "ownership_head.2.bias")
OUTCOME_VALUES = np.array([1.0, 0.0, 0.0, -1.0])


def random_ownership(w: int, h: int, H: int, seed) -> dict:
    """The four tensors of an ownership head whose logits tell classes and cells apart: weights with std 1/sqrt(H) in the
    first layer and 2/sqrt(H) in the second, biases with std 0.5. (The reference initialises the head with std 0.01, which
    gives near-uniform logits: a permuted class or cell would go unnoticed.)"""
    rng = np.random.default_rng(seed)
    n_out = w * h * 4
    return {OWN_KEYS[0]: (rng.standard_normal((H, H)) / np.sqrt(H)).astype(np.float32),
            OWN_KEYS[1]: (rng.standard_normal(H) * 0.5).astype(np.float32),
            OWN_KEYS[2]: (rng.standard_normal((n_out, H)) * 2.0 / np.sqrt(H)).astype(np.float32),
            OWN_KEYS[3]: (rng.standard_normal(n_out) * 0.5).astype(np.float32)}


def trunk_features(tensors: dict, obs: np.ndarray) -> np.ndarray:
    """the trunk's output (eval mode), the input of every head"""
    t = {k: np.asarray(v, np.float64) for k, v in tensors.items() if k.startswith("trunk.")}
    return _mlp_np._block(t, "trunk.4", "trunk.5", _mlp_np._block(t, "trunk.0", "trunk.1", np.asarray(obs, np.float64)))


def head_forward(tensors: dict, features: np.ndarray) -> np.ndarray:
    """ownership logits (n, hw, 4)"""
    t = {k: np.asarray(tensors[k], np.float64) for k in OWN_KEYS}
    hid = np.maximum(features @ t[OWN_KEYS[0]].T + t[OWN_KEYS[1]], 0.0)
    out = hid @ t[OWN_KEYS[2]].T + t[OWN_KEYS[3]]
    return out.reshape(len(out), -1, 4)


def forward(tensors: dict, obs: np.ndarray) -> np.ndarray:
    return head_forward(tensors, trunk_features(tensors, obs))


def cell_terms(logits: np.ndarray, targets: np.ndarray):
    """per cell: cross-entropy against the target class (0 where the target is -1) and softmax . [1, 0, 0, -1]"""
    l = np.asarray(logits, np.float64)
    t = np.asarray(targets).astype(np.int64)
    m = l.max(axis=-1, keepdims=True)
    e = np.exp(l - m)
    s = e.sum(axis=-1, keepdims=True)
    lse = (m + np.log(s))[..., 0]
    lt = np.take_along_axis(l, np.clip(t, 0, 3)[..., None], axis=-1)[..., 0]
    active = t >= 0
    return np.where(active, lse - lt, 0.0), np.where(active, ((e / s) * OUTCOME_VALUES).sum(axis=-1), 0.0)


def row_terms(logits: np.ndarray, targets: np.ndarray):
    """(ce, cells, value) of every row: sums over its active cells. logits (n, hw, 4) or (n, h, w, 4), targets to match"""
    n = len(logits)
    l = np.asarray(logits, np.float64).reshape(n, -1, 4)
    t = np.asarray(targets).reshape(n, -1)
    ce, ev = cell_terms(l, t)
    return ce.sum(axis=1), (t >= 0).sum(axis=1).astype(np.int64), ev.sum(axis=1)


def batch_weighted(ce_rows, cells_rows, batch_rows: int) -> float:
    """sum over consecutive batches of B_b * ce_b / cells_b, 0.0 for a batch without an active cell (ownership.py:35-37)"""
    ce_rows, cells_rows = np.asarray(ce_rows, np.float64), np.asarray(cells_rows, np.int64)
    total = 0.0
    for lo in range(0, len(ce_rows), batch_rows):
        c, k = ce_rows[lo:lo + batch_rows].sum(), int(cells_rows[lo:lo + batch_rows].sum())
        total += len(ce_rows[lo:lo + batch_rows]) * (c / k if k else 0.0)
    return float(total)


def loss_ownership(ce_rows, cells_rows, batch_rows: int = 0) -> float:
    """the reference's logged number: batch means averaged by batch size; batch_rows == 0: one batch"""
    n = len(ce_rows)
    return batch_weighted(ce_rows, cells_rows, batch_rows if batch_rows else max(n, 1)) / n
