"""Validation of a checkpoint over a device-resident ``RowSet``: the validation pass of the reference's training loop
(alpharat/nn/training/loop.py:306-361) without observations, target arrays or a PyTorch model.

The reference runs the model in eval mode over the validation shards batch by batch, takes the architecture's loss
(``architectures/*/loss.py``: soft-target cross-entropy per player, MSE per value), keeps every batch's logits and
computes the detailed metrics of ``alpharat/nn/metrics.py`` over their concatenation. Here ``ar_rows_validate`` writes
evaluator requests from the stored position records, runs the evaluator a ``Net`` already is, and reduces the terms of
every row to the sums of ``ValSums``; ``ValSums.metrics`` turns the sums into the numbers the reference logs under
``val/``.

    train, val = RowDataset(rowset).split(0.1, seed)
    metrics = val.validate(net).metrics()

Sums are additive: results over disjoint rows (chunks, sets, ranks) add with ``+`` to the result over their union.

The ``local_value`` architecture (LocalValueMLP) adds ``ownership_weight * loss_ownership`` to its loss
(``architectures/local_value/loss.py:55-59``). ``validate_lv`` is ``validate`` for such a checkpoint, loaded from a blob
that kept the ownership head (``checkpoint_to_blob(pt, keep_ownership=True)``): ``ar_rows_validate_lv`` also runs the head
on the trunk output of every row and reduces the masked cross-entropy against the stored cheese outcomes to ``OwnSums``;
``local_value_metrics`` gives the reference's ``val/`` numbers for that architecture, ``loss_ownership`` and the ``loss``
that decides ``best_model.pt`` included.

    net = Net(checkpoint_to_blob(pt, keep_ownership=True))
    sums, own = val.validate_lv(net, loss_batch_rows=batch_size)
    metrics = local_value_metrics(sums, own, policy_weight, value_weight, ownership_weight)

Not reproduced: AMP autocast (the evaluator is f32 throughout); BatchNorm is in eval mode, as in the reference's pass.

Top-k accuracy with ties: the target action is the *first* index of the largest target probability, as ``argmax`` gives;
among equal logits the lower index ranks first. ``torch.topk`` leaves the order among equal logits undefined, so on a row
with an exact logit tie at the target action this is this library's rule (include/alpharat_hip.h).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, fields

import numpy as np

from . import _lib

_PAIRS = ("ce", "sq_err", "ent_pred", "ent_target", "top1", "top2", "sum_pred", "sum_target", "sum_pred2", "sum_target2",
          "sum_pred_target")
DEFAULT_CHUNK_ROWS = 65536  # ar_rows_validate's chunk_rows == 0: a workspace of about 10 MB
#                             (ar_rows_validate_lv: plus chunk_rows * hidden_dim floats, 64 MB at hidden_dim 256)


@dataclass(frozen=True)
class ValSums:
    """``ArValSums``: sums over rows, a pair (P1, P2) each. ``top1`` / ``top2`` are counts."""
    n: int = 0
    ce: tuple = (0.0, 0.0)
    sq_err: tuple = (0.0, 0.0)
    ent_pred: tuple = (0.0, 0.0)
    ent_target: tuple = (0.0, 0.0)
    top1: tuple = (0, 0)
    top2: tuple = (0, 0)
    sum_pred: tuple = (0.0, 0.0)
    sum_target: tuple = (0.0, 0.0)
    sum_pred2: tuple = (0.0, 0.0)
    sum_target2: tuple = (0.0, 0.0)
    sum_pred_target: tuple = (0.0, 0.0)

    def __add__(self, other: "ValSums") -> "ValSums":
        if not isinstance(other, ValSums):
            return NotImplemented
        return ValSums(self.n + other.n, **{k: (getattr(self, k)[0] + getattr(other, k)[0],
                                                getattr(self, k)[1] + getattr(other, k)[1]) for k in _PAIRS})

    @classmethod
    def _from_c(cls, s: "_lib.ArValSums") -> "ValSums":
        conv = lambda k: int if k in ("top1", "top2") else float  # noqa: E731
        return cls(int(s.n), **{k: (conv(k)(getattr(s, k)[0]), conv(k)(getattr(s, k)[1])) for k in _PAIRS})

    def metrics(self, policy_weight: float = 1.0, value_weight: float = 1.0) -> dict:
        """The keys the reference logs under ``val/``. Means are sums over ``n`` (the reference's batch-size-weighted
        average of batch means is the same number); ``loss_value = 0.5 (v1 + v2)`` and
        ``loss = policy_weight (p1 + p2) + value_weight loss_value`` as in every ``architectures/*/loss.py``. Explained
        variance (metrics.py:65-90) uses unbiased variances: 0.0 when the target's is below 1e-8, else
        ``max(-1, 1 - Var(y - v) / Var(y))``; nan for ``n == 1``, as the reference gives. Correlation (metrics.py:93-116)
        is 0.0 when its denominator is below 1e-8. ``n == 0`` raises ``ValueError``."""
        n = self.n
        if n == 0:
            raise ValueError("no rows were validated: the metrics of an empty set are undefined")
        m = {}
        m["loss_p1"], m["loss_p2"] = self.ce[0] / n, self.ce[1] / n
        m["loss_value_p1"], m["loss_value_p2"] = self.sq_err[0] / n, self.sq_err[1] / n
        m["loss_value"] = 0.5 * (m["loss_value_p1"] + m["loss_value_p2"])
        m["loss"] = policy_weight * (m["loss_p1"] + m["loss_p2"]) + value_weight * m["loss_value"]
        for p, name in enumerate(("p1", "p2")):
            m[f"{name}/top1_accuracy"] = self.top1[p] / n
            m[f"{name}/top2_accuracy"] = self.top2[p] / n
            m[f"{name}/entropy_pred"] = self.ent_pred[p] / n
            m[f"{name}/entropy_target"] = self.ent_target[p] / n
            sv, sy = self.sum_pred[p], self.sum_target[p]
            # centred second moments: sum (v - mean v)^2, sum (y - mean y)^2, sum (v - mean v)(y - mean y)
            cvv = self.sum_pred2[p] - sv * sv / n
            cyy = self.sum_target2[p] - sy * sy / n
            cvy = self.sum_pred_target[p] - sv * sy / n
            if n == 1:
                ev = math.nan  # torch's unbiased variance of one element
            else:
                var_y = max(cyy, 0.0) / (n - 1)
                # Var(y - v) = (sum (y - v)^2 - (sum (y - v))^2 / n) / (n - 1)
                var_r = max(self.sq_err[p] - (sy - sv) * (sy - sv) / n, 0.0) / (n - 1)
                ev = 0.0 if var_y < 1e-8 else max(-1.0, 1.0 - var_r / var_y)
            den = math.sqrt(max(cvv, 0.0) * max(cyy, 0.0))
            m[f"value/{name}_explained_variance"] = ev
            m[f"value/{name}_correlation"] = 0.0 if den < 1e-8 else cvy / den
        return m


def validate(rowset, net, rows, chunk_rows: int = 0, return_rows: bool = False):
    """``ar_rows_validate``: ``net`` (an ``alpharat_amd.nets.Net``) over the stored positions ``rows`` of ``rowset`` (any
    order, repeats allowed). ``chunk_rows``: rows per evaluator launch, 0 = ``DEFAULT_CHUNK_ROWS``. Returns ``ValSums``;
    with ``return_rows`` also a dict of the per-row ``logits_p1`` / ``logits_p2`` ``(n, 5)`` and ``value_p1`` /
    ``value_p2`` ``(n,)`` in request order (the reference's "detailed outputs", loop.py:343-354). Blocks until the sums are
    on the host. A row beyond the set, a net built for another board size or on another device raises ``RuntimeError``
    and leaves the set and the net as they were."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    if rows.ndim != 1:
        raise ValueError("rows must be one-dimensional")
    if chunk_rows < 0:
        raise ValueError("chunk_rows must not be negative")
    if not getattr(net, "handle", None):
        raise RuntimeError("the net is closed")
    n = len(rows)
    out = None
    ptrs = None
    if return_rows:
        out = dict(logits_p1=np.zeros((n, 5), np.float32), logits_p2=np.zeros((n, 5), np.float32),
                   value_p1=np.zeros(n, np.float32), value_p2=np.zeros(n, np.float32))
        ptrs = C.byref(_lib.ArValRows(*[out[k].ctypes.data for k in ("logits_p1", "logits_p2", "value_p1", "value_p2")]))
    sums = _lib.ArValSums()
    rc = _lib.load().ar_rows_validate(rowset._handle(), net.handle, rows.ctypes.data if n else None, n, int(chunk_rows),
                                      C.byref(sums), ptrs)
    if rc == _lib.AR_E_INVALID:
        raise RuntimeError(_lib.last_error())
    _lib.check(rc)
    res = ValSums._from_c(sums)
    return (res, out) if return_rows else res


@dataclass(frozen=True)
class OwnSums:
    """``ArOwnSums``: the ownership loss of ``local_value`` over ``n`` rows. ``ce`` / ``cells``: the cross-entropy summed
    over active cells and their number, additive over rows. ``batch_weighted``: with ``batch_rows > 0`` the sum over
    consecutive batches of that many rows of ``B_b * ce_b / cells_b`` (0.0 for a batch without an active cell), the
    reference's batch-size-weighted accumulation; additive over requests that are whole numbers of batches."""
    n: int = 0
    cells: int = 0
    ce: float = 0.0
    batch_weighted: float = 0.0
    batch_rows: int = 0

    def __add__(self, other: "OwnSums") -> "OwnSums":
        if not isinstance(other, OwnSums):
            return NotImplemented
        if self.batch_rows != other.batch_rows:
            raise ValueError(f"sums over batches of {self.batch_rows} and of {other.batch_rows} rows do not add")
        return OwnSums(self.n + other.n, self.cells + other.cells, self.ce + other.ce,
                       self.batch_weighted + other.batch_weighted, self.batch_rows)

    @classmethod
    def _from_c(cls, s: "_lib.ArOwnSums") -> "OwnSums":
        return cls(int(s.n), int(s.cells), float(s.ce), float(s.batch_weighted), int(s.batch_rows))

    def metrics(self) -> dict:
        """``loss_ownership``: ``batch_weighted / n`` when ``batch_rows > 0``, the reference's number (per batch the mean
        over its active cells, ``losses/ownership.py:35-46``, batches averaged by size); else ``ce / cells``, the mean over
        all active cells, which is the reference's when one batch covers the request (0.0 without an active cell).
        ``n == 0`` raises ``ValueError``."""
        if self.n == 0:
            raise ValueError("no rows were validated: the metrics of an empty set are undefined")
        if self.batch_rows > 0:
            return {"loss_ownership": self.batch_weighted / self.n}
        return {"loss_ownership": self.ce / self.cells if self.cells else 0.0}


def local_value_metrics(valsums: ValSums, ownsums: OwnSums, policy_weight: float = 1.0, value_weight: float = 1.0,
                        ownership_weight: float = 1.0) -> dict:
    """The reference's ``val/`` numbers of a ``local_value`` checkpoint: ``ValSums.metrics()`` plus ``loss_ownership``, and
    ``loss = policy_weight (p1 + p2) + value_weight loss_value + ownership_weight loss_ownership``
    (``architectures/local_value/loss.py:55-59``)."""
    if valsums.n != ownsums.n:
        raise ValueError(f"the sums are over {valsums.n} and {ownsums.n} rows")
    m = valsums.metrics(policy_weight, value_weight)
    m.update(ownsums.metrics())
    m["loss"] = m["loss"] + ownership_weight * m["loss_ownership"]
    return m


def validate_lv(rowset, net, rows, chunk_rows: int = 0, loss_batch_rows: int = 0, return_rows: bool = False):
    """``ar_rows_validate_lv``: ``validate`` for a net with LocalValueMLP's ownership head (``net.has_ownership``).
    Returns ``(ValSums, OwnSums)``, the first being what ``validate`` returns; ``loss_batch_rows``: the reference's
    validation batch size, 0 = one pooled mean (``OwnSums``). ``chunk_rows`` is rounded up to a multiple of it. With
    ``return_rows`` a third value, ``validate``'s dict plus the per-row ``own_ce`` ``(n,)`` float64, ``own_cells`` ``(n,)``
    uint32, ``own_value`` ``(n,)`` (the reference's ``ownership_value`` under ``cheese_mask = cheese_outcomes >= 0``) and
    ``own_logits`` ``(n, height, width, 4)``. The workspace is ``validate``'s plus ``chunk_rows * hidden_dim`` floats (64 MB
    at the default chunk and 256). A net without the head raises ``RuntimeError``, like ``validate``'s refusals."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    if rows.ndim != 1:
        raise ValueError("rows must be one-dimensional")
    if chunk_rows < 0 or loss_batch_rows < 0:
        raise ValueError("chunk_rows and loss_batch_rows must not be negative")
    if not getattr(net, "handle", None):
        raise RuntimeError("the net is closed")
    n = len(rows)
    out = None
    ptrs = own_ptrs = None
    if return_rows:
        h, w = rowset.height, rowset.width
        out = dict(logits_p1=np.zeros((n, 5), np.float32), logits_p2=np.zeros((n, 5), np.float32),
                   value_p1=np.zeros(n, np.float32), value_p2=np.zeros(n, np.float32), own_ce=np.zeros(n, np.float64),
                   own_cells=np.zeros(n, np.uint32), own_value=np.zeros(n, np.float32),
                   own_logits=np.zeros((n, h, w, 4), np.float32))
        ptrs = C.byref(_lib.ArValRows(*[out[k].ctypes.data for k in ("logits_p1", "logits_p2", "value_p1", "value_p2")]))
        own_ptrs = C.byref(_lib.ArOwnRows(*[out[k].ctypes.data for k in ("own_ce", "own_cells", "own_value", "own_logits")]))
    sums, own = _lib.ArValSums(), _lib.ArOwnSums()
    rc = _lib.load().ar_rows_validate_lv(rowset._handle(), net.handle, rows.ctypes.data if n else None, n, int(chunk_rows),
                                         int(loss_batch_rows), C.byref(sums), C.byref(own), ptrs, own_ptrs)
    if rc == _lib.AR_E_INVALID:
        raise RuntimeError(_lib.last_error())
    _lib.check(rc)
    res = (ValSums._from_c(sums), OwnSums._from_c(own))
    return (*res, out) if return_rows else res


assert tuple(f.name for f in fields(ValSums))[1:] == _PAIRS
