"""Fixtures of the training-step tests, shared by the CPU and the GPU side, and the driver of tests/hostsim_train -- test
infrastructure only.

Every fixture a gradient is compared on is named here, so that tests/test_train_np.py can assert the ReLU guard for exactly
the list tests/test_gpu_train.py runs: a BatchNorm output within rounding of zero flips its ReLU mask between two correct
float32 implementations and moves that row's whole gradient contribution, so every fixture must have ``relu_margin >=
MARGIN`` in the float64 restatement, with no exception. The network seeds below were picked on the CPU until that holds.
"""
from __future__ import annotations

import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

import _augment_np as A
import _rows as T
import _rows_np as R
import _train_np as N
from _random_nets import random_mlp

HERE = Path(__file__).resolve().parent / "hostsim_train"
GOLD = Path(__file__).resolve().parent / "golden" / "train"
GOLDEN = ("mlp_5x5_h32_n2", "mlp_5x5_h32_n33", "mlp_7x5_h64_n70")
BOARDS = {b[0]: b for b in T.BOARDS}
MARGIN = 1e-4
WEIGHTS = dict(policy_weight=1.0, value_weight=0.5)

# (board, H, n, network seed): the shapes of the device test
SHAPES = [("5x5 open", 32, 2, 1), ("5x5 open", 32, 33, 1), ("7x5", 64, 129, 2), ("7x7", 256, 300, 12785),
          ("15x11 maze", 96, 40, 1), ("16x16", 32, 17, 1)]
SHAPE_IDS = [f"{b.replace(' ', '_')}-h{H}-n{n}" for b, H, n, _ in SHAPES]
# one order of 120 rows, three windows of it
WINDOW_BOARD, WINDOW_H, WINDOW_ROWS, WINDOW_SEED = "7x5", 64, 120, 3
WINDOWS = [(0, 50), (50, 50), (100, 20)]
# the same rows unswapped and all swapped
SWAP_BOARD, SWAP_H, SWAP_ROWS, SWAP_SEED = "5x5 open", 32, 40, 1
# five steps of SGD
TRAJ_BOARD, TRAJ_H, TRAJ_BATCH, TRAJ_STEPS, TRAJ_LR, TRAJ_SEED, TRAJ_PLAN_SEED = "7x7", 64, 64, 5, 0.05, 72, 7


@functools.lru_cache(maxsize=None)
def board(name: str):
    """(games, stack_rows(games)) of a board of tests/_rows.py, played once"""
    games = T.board_games(*BOARDS[name])
    return games, R.stack_rows(games)


def repeated_order(total: int, n: int, seed: int):
    """(order, swap) of n rows over `total` stored ones: the rows in one shuffled turn, again and again; a row that comes
    again is seen by the other player than the time before. (Shuffled, because neighbouring positions of a game differ in a
    few inputs only: two of them as a batch of two have column variances far below the BatchNorm's eps, where
    (z - mu) * rsqrt(var + eps) amplifies the rounding of z several hundred times in any float32 implementation.)"""
    rng = np.random.default_rng(seed)
    order = np.tile(rng.permutation(total), -(-n // total))[:n]
    swap = rng.random(n) < 0.5
    for i in range(total, n):
        swap[i] = not swap[i - total]
    return order.astype(np.int64), swap


def make_case(board_name: str, sd: dict, order, swap) -> dict:
    """the case of tests/_train_np.py for rows `order` of the board's stacked rows, swapped where `swap` is set"""
    _, plain = board(board_name)
    w, h = BOARDS[board_name][1], BOARDS[board_name][2]
    rows = A.swap_rows(R.take(plain, order), swap, w, h)
    return dict(sd=sd, board=board_name, order=np.asarray(order, np.int64), swap=np.asarray(swap, bool), width=w, height=h,
                observation=rows["observation"], policy_p1=rows["policy_p1"], policy_p2=rows["policy_p2"],
                value_p1=rows["value_p1"].reshape(-1), value_p2=rows["value_p2"].reshape(-1), **WEIGHTS)


def shape_case(board_name: str, H: int, n: int, seed: int) -> dict:
    _, plain = board(board_name)
    w, h = BOARDS[board_name][1], BOARDS[board_name][2]
    order, swap = repeated_order(len(plain["value_p1"]), n, seed)
    return make_case(board_name, random_mlp(w, h, H, seed), order, swap)


# the ``value`` family's head (tests/_saturated_nets.py) on its PyRatMLP: pre-softplus outputs on both sides of 20, above 89
# and below -90, so the step's softplus and its derivative take the linear branch, the threshold and the underflowing one
VALUE_BOARD, VALUE_NET, VALUE_ROWS, VALUE_SEED = "5x5 open", "mlp_5x5_h32", 33, 1


def value_family_case() -> dict:
    import _saturated_nets as S

    _, plain = board(VALUE_BOARD)
    order, swap = repeated_order(len(plain["value_p1"]), VALUE_ROWS, VALUE_SEED)
    return make_case(VALUE_BOARD, S.family(VALUE_NET, "value"), order, swap)


def window_cases() -> list:
    """the whole order's case (rows, swap, network) and one case per window"""
    whole = shape_case(WINDOW_BOARD, WINDOW_H, WINDOW_ROWS, WINDOW_SEED)
    return whole, [make_case(WINDOW_BOARD, whole["sd"], whole["order"][f:f + n], whole["swap"][f:f + n]) for f, n in WINDOWS]


def swap_cases() -> tuple:
    """(unswapped, all swapped) over the same rows and network"""
    _, plain = board(SWAP_BOARD)
    w, h = BOARDS[SWAP_BOARD][1], BOARDS[SWAP_BOARD][2]
    order = np.arange(SWAP_ROWS) % len(plain["value_p1"])
    sd = random_mlp(w, h, SWAP_H, SWAP_SEED)
    return (make_case(SWAP_BOARD, sd, order, np.zeros(SWAP_ROWS, bool)), make_case(SWAP_BOARD, sd, order, np.ones(SWAP_ROWS, bool)))


def golden_case(name: str) -> dict:
    """a golden as a case, with the reference's results under "f32" and "f64" (losses, outputs, grads, running)"""
    with np.load(GOLD / f"{name}.npz") as z:
        a = {k: z[k] for k in z.files}
    case = dict(sd={k[3:]: v for k, v in a.items() if k.startswith("sd/")}, board=str(a["board"]), order=a["order"], swap=a["swap"],
                width=int(a["width"]), height=int(a["height"]), hidden=int(a["hidden"]), policy_weight=float(a["weights"][0]),
                value_weight=float(a["weights"][1]),
                **{k: a[k] for k in ("observation", "policy_p1", "policy_p2", "value_p1", "value_p2")})
    for tag in ("f32", "f64"):
        case[tag] = dict(losses={k: a[f"{tag}/{k}"] for k in N.LOSS_KEYS}, **{k: a[f"{tag}/{k}"] for k in N.OUT_KEYS},
                         grads={k: a[f"{tag}/grad/{k}"] for k in N.PARAM_KEYS},
                         running={k: a[f"{tag}/running/{k}"] for k in N.RUNNING_KEYS})
    return case


# ---- the five steps of SGD ----------------------------------------------------------------------------------------------
def trajectory_plan() -> list:
    """[(epoch, order, mask)] for as many epochs of alpharat_amd.dataset.epoch_plan as TRAJ_STEPS batches need, and the
    (epoch, first) of every step: the batches grad_iter and epoch_iter cut (drop_last)"""
    from alpharat_amd.dataset import batch_windows, epoch_plan

    _, plain = board(TRAJ_BOARD)
    total = len(plain["value_p1"])
    steps, epochs, epoch = [], [], 0
    while len(steps) < TRAJ_STEPS:
        order, mask = epoch_plan(total, TRAJ_PLAN_SEED, epoch)
        epochs.append((epoch, order, mask))
        steps += [(epoch, first) for first, n in batch_windows(total, TRAJ_BATCH, True)]
        epoch += 1
        assert epoch < 50, "the board has fewer rows than a batch"
    return epochs, steps[:TRAJ_STEPS]


def trajectory_cases_f64() -> list:
    """the float64 trajectory: per step its case (the network before the step) and the result of tests/_train_np.py step;
    plain SGD, running statistics carried along. The last entry's "after" is the final state dict."""
    w, h = BOARDS[TRAJ_BOARD][1], BOARDS[TRAJ_BOARD][2]
    epochs, steps = trajectory_plan()
    plans = {e: (o, m) for e, o, m in epochs}
    sd = {k: np.asarray(v, np.float64) for k, v in random_mlp(w, h, TRAJ_H, TRAJ_SEED).items()}
    out = []
    for epoch, first in steps:
        order, mask = plans[epoch]
        idx = order[first:first + TRAJ_BATCH]
        case = make_case(TRAJ_BOARD, dict(sd), idx, mask[idx])
        res = N.step(case)
        sd = dict(sd)
        for k in N.PARAM_KEYS:
            sd[k] = sd[k] - TRAJ_LR * res["grads"][k]
        sd.update(res["running"])
        out.append(dict(case=case, result=res, after=sd))
    return out


# ---- the gradient tolerance ---------------------------------------------------------------------------------------------
def grad_bounds(g64: dict, gref32: dict) -> dict:
    """per tensor: 8 * max(e_ref, 2^-23 * max|g64 of the layer's weight|), e_ref = max|gref32 - g64|: the library may be
    eight times as far from the float64 gradient as the reference's own float32 evaluation is; the second term is the floor
    for tensors whose true value is zero (the two trunk biases)"""
    out = {}
    for k in g64:
        e_ref = float(np.abs(np.asarray(gref32[k], np.float64) - g64[k]).max())
        out[k] = 8.0 * max(e_ref, 2.0 ** -23 * float(np.abs(g64[N.LAYER_WEIGHT[k]]).max()))
    return out


def assert_grads_within(got: dict, g64: dict, gref32: dict, what: str = "", skip=()) -> None:
    bounds = grad_bounds(g64, gref32)
    bad = []
    for k in g64:
        if k in skip:
            continue
        err = float(np.abs(np.asarray(got[k], np.float64) - g64[k]).max())
        print(f"{what} {k}: err {err:.3e} bound {bounds[k]:.3e} (max|g| {np.abs(g64[k]).max():.3e})")
        if not err <= bounds[k]:
            bad.append((k, err, bounds[k]))
    assert not bad, (what, bad)


# ---- tests/hostsim_train ------------------------------------------------------------------------------------------------
TERMS = np.dtype([("ce", np.float32, 2), ("v", np.float32, 2), ("sq", np.float32, 2), ("dout", np.float32, 12)])
_sim = None


def sim() -> C.CDLL:
    global _sim
    if _sim is None:
        subprocess.run(["make", "-s", "-C", str(HERE)], check=True)
        L = C.CDLL(str(HERE / "libtrainsim.so"))
        L.ts_heads.restype = None
        L.ts_heads.argtypes = [C.c_uint64] + [C.c_void_p] * 5 + [C.c_float, C.c_float, C.c_void_p]
        L.ts_bn_forward.restype = None
        L.ts_bn_forward.argtypes = [C.c_uint64, C.c_uint32] + [C.c_void_p] * 7
        L.ts_bn_backward.restype = None
        L.ts_bn_backward.argtypes = [C.c_uint64, C.c_uint32] + [C.c_void_p] * 7
        L.ts_terms_words.restype = C.c_int
        L.ts_cols.restype = L.ts_split.restype = None
        L.ts_cols.argtypes = [C.c_int, C.c_int, C.c_void_p]
        L.ts_split.argtypes = [C.c_int, C.c_void_p]
        assert L.ts_terms_words() * 4 == TERMS.itemsize
        _sim = L
    return _sim


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def sim_heads(head_out, t1, t2, y1, y2, pw_n: float, vw_n: float) -> np.ndarray:
    """dev_train.h train_head_terms over rows: the rows' TERMS"""
    arrs = [_f32(head_out), _f32(t1), _f32(t2), _f32(y1).reshape(-1), _f32(y2).reshape(-1)]
    terms = np.zeros(len(arrs[0]), TERMS)
    sim().ts_heads(len(terms), *[a.ctypes.data for a in arrs], pw_n, vw_n, terms.ctypes.data)
    return terms


def sim_bn_forward(z, mu, var, gamma, beta):
    arrs = [_f32(z), np.ascontiguousarray(mu, np.float64), _f32(var), _f32(gamma), _f32(beta)]
    y, xhat = np.zeros_like(arrs[0]), np.zeros_like(arrs[0])
    sim().ts_bn_forward(arrs[0].shape[0], arrs[0].shape[1], *[a.ctypes.data for a in arrs], y.ctypes.data, xhat.ctypes.data)
    return y, xhat


def sim_bn_backward(dy, xhat, var, gamma, mean_dy, mean_dyx):
    arrs = [_f32(dy), _f32(xhat), _f32(var), _f32(gamma), _f32(mean_dy), _f32(mean_dyx)]
    dz = np.zeros_like(arrs[0])
    sim().ts_bn_backward(arrs[0].shape[0], arrs[0].shape[1], *[a.ctypes.data for a in arrs], dz.ctypes.data)
    return dz


def sim_cols(n: int, H: int) -> tuple:
    """dev_train.h train_cols: (P, rpp)"""
    out = np.zeros(2, np.int32)
    sim().ts_cols(n, H, out.ctypes.data)
    return int(out[0]), int(out[1])


def sim_split(rows: int) -> tuple:
    """dev_train.h train_split: (S, kps)"""
    out = np.zeros(2, np.int32)
    sim().ts_split(rows, out.ctypes.data)
    return int(out[0]), int(out[1])
