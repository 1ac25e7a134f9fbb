"""Boards, networks and the driver of tests/hostsim_validate for the validation tests -- test infrastructure only.

The rows are the oracle games of tests/_rows.py BOARDS. A network is named as in CASES; ``network`` gives its blob and the
expected forward in float64 (tests/_mlp_np.py, tests/_katago_np.py, the oracle's forward for PyRatCNN) over the flat
observations of tests/_rows_np.py stack_rows.
"""
from __future__ import annotations

import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

import _katago_np
import _metrics_np as M
import _mlp_np
import _oracle as O
import _rows as T
import _rows_np as R
from _random_nets import random_mlp, random_symmetric

HERE = Path(__file__).resolve().parent / "hostsim_validate"
GOLD = Path(__file__).resolve().parent / "golden"
BOARDS = {b[0]: b for b in T.BOARDS}
SEED = 5

RANDOM_NETS = ("random_mlp_h64", "random_mlp_h40", "random_symmetric_h64")  # k_mlp_mfma, k_mlp, k_symmetric_mfma2 / k_symmetric
CASES = [(board, net) for net in RANDOM_NETS for board in BOARDS] + [
    ("7x5", "nets/cnn_gpool_7x5_c16"), ("7x5", "nets_katago/katago_7x5_c32"), ("7x7", "nets/mlp_7x7_h256"),
    # logit spreads above 104 and pre-softplus values from -90 to 200 (tests/_saturated_nets.py): the cross-entropy has to
    # come from the log-softmax, not from log(p) of a p that underflowed
    ("5x5 open", "saturated_mlp_5x5_h32")]
CASE_IDS = [f"{net.split('/')[-1]}-on-{board.replace(' ', '_')}" for board, net in CASES]


@functools.lru_cache(maxsize=None)
def board(name: str):
    """(games, stack_rows(games)) of a board, played once"""
    games = T.board_games(*BOARDS[name])
    return games, R.stack_rows(games)


def network(name: str, w: int, h: int, tmp_dir=None):
    """(blob path or None without tmp_dir, forward(obs) -> dict of float64 logits_p1, logits_p2, value_p1, value_p2)"""
    from alpharat_amd.weights import read_blob, write_blob

    if name.startswith("saturated_"):
        import _saturated_nets as S

        arch, bw, bh, _ = S.ARCHS[name[len("saturated_"):]]
        assert (arch, bw, bh) == ("mlp", w, h), name
        t = S.family(name[len("saturated_"):], "policy+value")
        blob = write_blob(Path(tmp_dir) / f"{name}.arnet", arch, w, h, t) if tmp_dir is not None else None
        fwd = lambda obs: _mlp_np.mlp_forward(t, obs)  # noqa: E731
    elif name.startswith("random_"):
        kind, H = name[len("random_"):].split("_h")
        t = (random_mlp if kind == "mlp" else random_symmetric)(w, h, int(H), SEED)
        blob = write_blob(Path(tmp_dir) / f"{name}_{w}x{h}.arnet", kind, w, h, t) if tmp_dir is not None else None
        fwd = (lambda obs: _mlp_np.mlp_forward(t, obs)) if kind == "mlp" else (lambda obs: _mlp_np.symmetric_forward(t, w, h, obs))
    else:
        blob = GOLD / f"{name}.arnet"
        arch, bw, bh, t = read_blob(blob)
        assert (bw, bh) == (w, h), (name, bw, bh)
        if arch == "cnn_katago":
            fwd = lambda obs: _katago_np.forward(t, w, h, obs)  # noqa: E731
        elif arch == "mlp":
            fwd = lambda obs: _mlp_np.mlp_forward(t, obs)  # noqa: E731
        else:
            net = O.Net(blob)
            fwd = net.forward
    keys = ("logits_p1", "logits_p2", "value_p1", "value_p2")

    def forward(obs):
        out = fwd(obs)
        return {k: np.asarray(out[k], np.float64) for k in keys}

    return blob, forward


def expected_case(rows: dict, want: dict, index=None) -> dict:
    """the case of tests/_metrics_np.py for the rows' targets and the outputs `want` (per-row, already in request order)"""
    return M.case_from_rows(rows, want["logits_p1"], want["logits_p2"], want["value_p1"], want["value_p2"], index)


def ambiguous(logits: np.ndarray, target: np.ndarray) -> np.ndarray:
    """rows where some other logit is within 2 (1e-5 + 1e-5 max|l|) of the logit at the target's argmax: an evaluator
    within the project's tolerance of `logits` may rank the target action differently"""
    l = np.asarray(logits, np.float64)
    a = np.asarray(target).argmax(axis=-1)
    la = np.take_along_axis(l, a[:, None], axis=-1)
    gap = np.abs(l - la)
    gap[np.arange(len(l)), a] = np.inf
    return gap.min(axis=-1) <= 2 * (1e-5 + 1e-5 * np.abs(l).max(axis=-1))


def scores(games) -> tuple:
    """(score at the position of P1, P2, final score of P1, P2) of every row, float32, in stack_rows order"""
    s1 = np.concatenate([np.asarray(g["p1_score"], np.float32) for g in games])
    s2 = np.concatenate([np.asarray(g["p2_score"], np.float32) for g in games])
    f1 = np.concatenate([np.full(int(g["n"]), g["final_p1_score"], np.float32) for g in games])
    f2 = np.concatenate([np.full(int(g["n"]), g["final_p2_score"], np.float32) for g in games])
    return s1, s2, f1, f2


# ---- tests/hostsim_validate ----------------------------------------------------------------------------------------------
TERMS = np.dtype([("ce", np.float32, 2), ("ent_pred", np.float32, 2), ("ent_target", np.float32, 2), ("top1", np.uint32, 2),
                  ("top2", np.uint32, 2), ("pred", np.float32, 2), ("target", np.float32, 2)])
_sim = None


def sim() -> C.CDLL:
    global _sim
    if _sim is None:
        subprocess.run(["make", "-s", "-C", str(HERE)], check=True)
        L = C.CDLL(str(HERE / "libvalidatesim.so"))
        L.vs_run.restype = None
        L.vs_run.argtypes = [C.c_int, C.c_uint64] + [C.c_void_p] * 12
        L.vs_terms_words.restype = C.c_int
        assert L.vs_terms_words() * 4 == TERMS.itemsize
        _sim = L
    return _sim


def sim_run(nw, s1, s2, f1, f2, pol1, pol2, logits_p1, logits_p2, v1, v2):
    """dev_validate.h over rows on the CPU: (sums as tests/_metrics_np.py sums() gives them, the rows' ValTerms)"""
    f = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    n = len(s1)
    logits = f(np.concatenate([f(logits_p1).reshape(n, 5), f(logits_p2).reshape(n, 5)], axis=1))
    arrs = [f(s1), f(s2), f(f1), f(f2), f(pol1), f(pol2), logits, f(v1), f(v2)]
    terms = np.zeros(n, TERMS)
    d, c = np.zeros(18, np.float64), np.zeros(4, np.uint64)
    sim().vs_run(nw, n, *[a.ctypes.data for a in arrs], terms.ctypes.data, d.ctypes.data, c.ctypes.data)
    out = dict(n=n)
    for j, k in enumerate(M.SUM_KEYS):
        out[k] = (float(d[j]), float(d[9 + j]))
    out["top1"], out["top2"] = (int(c[0]), int(c[1])), (int(c[2]), int(c[3]))
    return out, terms


def assert_sums_close(got: dict, want: dict, rel: float, what="") -> None:
    """counts equal; every double sum within rel of the want, relative to the sum of magnitudes it could have lost"""
    assert got["n"] == want["n"], (what, got["n"], want["n"])
    for k in M.COUNT_KEYS:
        assert tuple(got[k]) == tuple(want[k]), (what, k, got[k], want[k])
    for k in M.SUM_KEYS:
        for p in (0, 1):
            assert abs(got[k][p] - want[k][p]) <= rel * abs(want[k][p]) + 1e-300, (what, k, p, got[k][p], want[k][p])


def sums_of(valsums) -> dict:
    """an alpharat_amd.validate.ValSums as the dict of tests/_metrics_np.py sums()"""
    return dict(n=valsums.n, **{k: tuple(getattr(valsums, k)) for k in M.SUM_KEYS + M.COUNT_KEYS})
