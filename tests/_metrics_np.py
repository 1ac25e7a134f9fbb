"""The reference's validation numbers in float64 NumPy -- test infrastructure only.

A restatement, written from their text, of
  alpharat/nn/architectures/*/loss.py     F.cross_entropy (soft targets), F.mse_loss, the weighted total  -> metrics()
  alpharat/nn/metrics.py:15-31            top_k_accuracy            -> ranks()
  alpharat/nn/metrics.py:34-62            policy_entropy, target_entropy
  alpharat/nn/metrics.py:65-116           explained_variance, value_correlation
  alpharat/nn/training/loop.py:306-361    means over the validation rows
It is tied to the reference by tests/golden/metrics (tools/gen_metrics_golden.py runs the reference's own functions). It is
the comparison partner of alpharat_amd.validate: ``sums`` gives what ``ar_rows_validate`` sums, ``metrics`` what
``ValSums.metrics`` derives -- computed here from the rows directly, with centred moments, not from the sums.

A case is a dict of arrays: logits_p1, logits_p2 (n, 5); pred_v1, pred_v2 (n,); policy_p1, policy_p2 (n, 5); value_p1,
value_p2 (n,).
"""
from __future__ import annotations

import numpy as np

PLAYERS = (("logits_p1", "pred_v1", "policy_p1", "value_p1"), ("logits_p2", "pred_v2", "policy_p2", "value_p2"))
SUM_KEYS = ("ce", "sq_err", "ent_pred", "ent_target", "sum_pred", "sum_target", "sum_pred2", "sum_target2", "sum_pred_target")
COUNT_KEYS = ("top1", "top2")


def _f64(case: dict, p: int):
    lk, vk, tk, yk = PLAYERS[p]
    return (np.asarray(case[lk], np.float64).reshape(-1, 5), np.asarray(case[vk], np.float64).reshape(-1),
            np.asarray(case[tk], np.float64).reshape(-1, 5), np.asarray(case[yk], np.float64).reshape(-1))


def log_softmax(l: np.ndarray) -> np.ndarray:
    m = l.max(axis=-1, keepdims=True)
    return l - (m + np.log(np.exp(l - m).sum(axis=-1, keepdims=True)))


def ranks(l: np.ndarray, t: np.ndarray) -> np.ndarray:
    """The rank of the target action among the logits: a = first index of the largest target (argmax);
    rank = #{k : l_k > l_a} + #{k < a : l_k == l_a} (among equal logits the lower index first)."""
    a = t.argmax(axis=-1)
    la = np.take_along_axis(l, a[:, None], axis=-1)
    k = np.arange(l.shape[1])[None, :]
    return (l > la).sum(axis=-1) + ((l == la) & (k < a[:, None])).sum(axis=-1)


def row_terms(case: dict, p: int) -> dict:
    """per-row terms of player p, float64 (n,) each; top1 / top2 bool"""
    l, v, t, y = _f64(case, p)
    ls = log_softmax(l)
    r = ranks(l, t)
    return dict(ce=-(t * ls).sum(-1), sq_err=(v - y) ** 2, ent_pred=-(np.exp(ls) * ls).sum(-1),
                ent_target=-(t * np.log(np.maximum(t, 1e-8))).sum(-1), top1=r < 1, top2=r < 2, sum_pred=v, sum_target=y,
                sum_pred2=v * v, sum_target2=y * y, sum_pred_target=v * y)


def sums(case: dict) -> dict:
    """What ar_rows_validate sums: n, and a pair (P1, P2) per key (float for SUM_KEYS, int for COUNT_KEYS)."""
    per = [row_terms(case, p) for p in (0, 1)]
    out = dict(n=len(per[0]["ce"]))
    for k in SUM_KEYS:
        out[k] = tuple(float(per[p][k].sum()) for p in (0, 1))
    for k in COUNT_KEYS:
        out[k] = tuple(int(per[p][k].sum()) for p in (0, 1))
    return out


def metrics(case: dict, policy_weight: float = 1.0, value_weight: float = 1.0) -> dict:
    """The numbers the reference logs under val/ for these rows."""
    m = {}
    n = len(np.asarray(case["pred_v1"]).reshape(-1))
    for p, name in enumerate(("p1", "p2")):
        l, v, t, y = _f64(case, p)
        rt = row_terms(case, p)
        m[f"loss_{name}"] = rt["ce"].mean()                      # F.cross_entropy, reduction mean
        m[f"loss_value_{name}"] = rt["sq_err"].mean()            # F.mse_loss
        m[f"{name}/top1_accuracy"] = rt["top1"].mean()
        m[f"{name}/top2_accuracy"] = rt["top2"].mean()
        m[f"{name}/entropy_pred"] = rt["ent_pred"].mean()
        m[f"{name}/entropy_target"] = rt["ent_target"].mean()
        if n == 1:
            ev = np.nan                                          # torch.var of one element
        else:
            var_y = y.var(ddof=1)                                # metrics.py:83
            ev = 0.0 if var_y < 1e-8 else max(-1.0, 1.0 - (y - v).var(ddof=1) / var_y)  # :84-90
        vc, yc = v - v.mean(), y - y.mean()                      # :106-107
        den = np.sqrt((vc ** 2).sum() * (yc ** 2).sum())         # :110
        m[f"value/{name}_explained_variance"] = float(ev)
        m[f"value/{name}_correlation"] = 0.0 if den < 1e-8 else float((vc * yc).sum() / den)  # :112-116
    m["loss_value"] = 0.5 * (m["loss_value_p1"] + m["loss_value_p2"])
    m["loss"] = policy_weight * (m["loss_p1"] + m["loss_p2"]) + value_weight * m["loss_value"]
    return {k: float(x) for k, x in m.items()}


def case_from_rows(rows: dict, logits_p1, logits_p2, v1, v2, index=None) -> dict:
    """A case from the targets of tests/_rows_np.py stack_rows (all rows, or those of `index`) and per-row outputs."""
    take = (lambda a: np.asarray(a)) if index is None else (lambda a: np.asarray(a)[np.asarray(index, np.int64)])
    return dict(logits_p1=np.asarray(logits_p1), logits_p2=np.asarray(logits_p2), pred_v1=np.asarray(v1), pred_v2=np.asarray(v2),
                policy_p1=take(rows["policy_p1"]), policy_p2=take(rows["policy_p2"]),
                value_p1=take(rows["value_p1"]).reshape(-1), value_p2=take(rows["value_p2"]).reshape(-1))
