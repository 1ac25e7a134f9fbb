"""Fixtures of the SymmetricMLP training-step tests, shared by the CPU and the GPU side, and the driver of
tests/hostsim_train_sym -- test infrastructure only.

As in tests/_train.py, every fixture a gradient is compared on is named here, so that tests/test_train_sym_np.py can assert
the ReLU guard for exactly the list tests/test_gpu_train_sym.py runs: each of the seven BatchNorm outputs of the float64
restatement is at least ``MARGIN`` from zero. The network seeds were picked on the CPU until that holds.

The tolerance is tests/_train.py's ``grad_bounds`` itself: its table of layer weights (tests/_train_np.py ``LAYER_WEIGHT``)
gains SymmetricMLP's names here, by the same rule (a tensor's layer weight is ``<module>.weight``).
"""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import _train as TR
import _train_np as N
import _train_sym_np as NS
from _random_nets import random_symmetric
from _train import BOARDS, MARGIN, WEIGHTS, board, make_case, repeated_order  # noqa: F401

assert all(N.LAYER_WEIGHT.get(k, v) == v for k, v in NS.LAYER_WEIGHT.items())
N.LAYER_WEIGHT.update(NS.LAYER_WEIGHT)

HERE = Path(__file__).resolve().parent / "hostsim_train_sym"
GOLD = Path(__file__).resolve().parent / "golden" / "train_sym"
GOLDEN = ("sym_5x5_h32_n2", "sym_5x5_h32_n33", "sym_7x5_h64_n70")

# (board, H, n, seed): the shapes of the device test; the seed gives both repeated_order and random_symmetric
SHAPES = [("5x5 open", 32, 2, 1), ("5x5 open", 32, 33, 1), ("7x5", 64, 129, 29), ("7x7", 64, 300, 257), ("7x7", 256, 40, 164),
          ("15x11 maze", 96, 40, 8), ("16x16", 32, 17, 1)]
SHAPE_IDS = [f"{b.replace(' ', '_')}-h{H}-n{n}" for b, H, n, _ in SHAPES]
# one order of 120 rows, three windows of it
WINDOW_BOARD, WINDOW_H, WINDOW_ROWS, WINDOW_SEED = "7x5", 64, 120, 4
WINDOWS = [(0, 50), (50, 50), (100, 20)]
# the same rows unswapped and all swapped
SWAP_BOARD, SWAP_H, SWAP_ROWS, SWAP_SEED = "5x5 open", 32, 40, 3
# five steps of SGD
TRAJ_BOARD, TRAJ_H, TRAJ_BATCH, TRAJ_STEPS, TRAJ_LR, TRAJ_SEED, TRAJ_PLAN_SEED = "7x7", 64, 64, 5, 0.05, 271, 7


def shape_case(board_name: str, H: int, n: int, seed: int) -> dict:
    _, plain = board(board_name)
    w, h = BOARDS[board_name][1], BOARDS[board_name][2]
    order, swap = repeated_order(len(plain["value_p1"]), n, seed)
    return make_case(board_name, random_symmetric(w, h, H, seed), order, swap)


def window_cases() -> tuple:
    """the whole order's case (rows, swap, network) and one case per window"""
    whole = shape_case(WINDOW_BOARD, WINDOW_H, WINDOW_ROWS, WINDOW_SEED)
    return whole, [make_case(WINDOW_BOARD, whole["sd"], whole["order"][f:f + n], whole["swap"][f:f + n]) for f, n in WINDOWS]


def swap_cases() -> tuple:
    """(unswapped, all swapped) over the same rows and network"""
    _, plain = board(SWAP_BOARD)
    w, h = BOARDS[SWAP_BOARD][1], BOARDS[SWAP_BOARD][2]
    order = np.arange(SWAP_ROWS) % len(plain["value_p1"])
    sd = random_symmetric(w, h, SWAP_H, SWAP_SEED)
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
        case[tag] = dict(losses={k: a[f"{tag}/{k}"] for k in NS.LOSS_KEYS}, **{k: a[f"{tag}/{k}"] for k in NS.OUT_KEYS},
                         grads={k: a[f"{tag}/grad/{k}"] for k in NS.PARAM_KEYS},
                         running={k: a[f"{tag}/running/{k}"] for k in NS.RUNNING_KEYS})
    return case


def trajectory_plan() -> tuple:
    """tests/_train.py trajectory_plan for this file's board, batch and plan seed"""
    from alpharat_amd.dataset import batch_windows, epoch_plan

    _, plain = board(TRAJ_BOARD)
    total = len(plain["value_p1"])
    steps, epochs, epoch = [], [], 0
    while len(steps) < TRAJ_STEPS:
        order, mask = epoch_plan(total, TRAJ_PLAN_SEED, epoch, True, False)  # augment=False: the reference's NoAugmentation
        epochs.append((epoch, order, mask))
        steps += [(epoch, first) for first, n in batch_windows(total, TRAJ_BATCH, True)]
        epoch += 1
        assert epoch < 50, "the board has fewer rows than a batch"
    return epochs, steps[:TRAJ_STEPS]


def trajectory_cases_f64(seed: int = TRAJ_SEED) -> list:
    """the float64 trajectory: per step its case (the network before the step) and the result of tests/_train_sym_np.py
    step; plain SGD, running statistics carried along. The last entry's "after" is the final state dict."""
    w, h = BOARDS[TRAJ_BOARD][1], BOARDS[TRAJ_BOARD][2]
    epochs, steps = trajectory_plan()
    plans = {e: (o, m) for e, o, m in epochs}
    sd = {k: np.asarray(v, np.float64) for k, v in random_symmetric(w, h, TRAJ_H, seed).items()}
    out = []
    for epoch, first in steps:
        order, mask = plans[epoch]
        idx = order[first:first + TRAJ_BATCH]
        case = make_case(TRAJ_BOARD, dict(sd), idx, mask[idx])
        res = NS.step(case)
        sd = dict(sd)
        for k in NS.PARAM_KEYS:
            sd[k] = sd[k] - TRAJ_LR * res["grads"][k]
        sd.update(res["running"])
        out.append(dict(case=case, result=res, after=sd))
    return out


# ---- the tolerance of everything that is not a gradient --------------------------------------------------------------------
def value_bound(want, ref32) -> float:
    """grad_bounds' form for an output, a loss or a running statistic: 8 * max(e_ref, 2^-23 * max|f64 array|)"""
    want = np.asarray(want, np.float64)
    e_ref = float(np.abs(np.asarray(ref32, np.float64) - want).max())
    return 8.0 * max(e_ref, 2.0 ** -23 * float(np.abs(want).max()))


def assert_values_within(got: dict, want: dict, ref32: dict, keys, what: str = "") -> None:
    bad = []
    for k in keys:
        err = float(np.abs(np.asarray(got[k], np.float64) - np.asarray(want[k], np.float64)).max())
        bound = value_bound(want[k], ref32[k])
        print(f"{what} {k}: err {err:.3e} bound {bound:.3e} (max|f64| {np.abs(np.asarray(want[k], np.float64)).max():.3e})")
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, (what, bad)


assert_grads_within = TR.assert_grads_within

# ---- tests/hostsim_train_sym -----------------------------------------------------------------------------------------------
_sim = None


def sim() -> C.CDLL:
    global _sim
    if _sim is None:
        subprocess.run(["make", "-s", "-C", str(HERE)], check=True)
        L = C.CDLL(str(HERE / "libtrainsymsim.so"))
        L.tss_split.restype = None
        L.tss_split.argtypes = [C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tss_pack.restype = None
        L.tss_pack.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p]
        L.tss_head_dy.restype = None
        L.tss_head_dy.argtypes = [C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        _sim = L
    return _sim


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def sim_split(x, width: int, height: int):
    """dev_train_sym.h sym_shared_src / sym_player_src over rows: shared_raw (n, 5hw + 1), p_raw (2n, hw + 2), P1's rows first"""
    x = _f32(x)
    n, hw = len(x), width * height
    xs, xp = np.zeros((n, 5 * hw + 1), np.float32), np.zeros((2 * n, hw + 2), np.float32)
    sim().tss_split(n, hw, x.ctypes.data, xs.ctypes.data, xp.ctypes.data)
    return xs, xp


def sim_pack(dout):
    """sym_head_pack over rows: the packed dOut rows (2n, 12), P1's rows first"""
    dout = _f32(dout)
    d12 = np.zeros((2 * len(dout), 12), np.float32)
    sim().tss_pack(len(dout), dout.ctypes.data, d12.ctypes.data)
    return d12


def sim_head_dy(d12, wh):
    """sym_head_dy of every element: (rows, H) from packed rows (rows, 12) and Wh (6, 2H)"""
    d12, wh = _f32(d12), _f32(wh)
    H = wh.shape[1] // 2
    dy = np.zeros((len(d12), H), np.float32)
    sim().tss_head_dy(len(d12), H, d12.ctypes.data, wh.ctypes.data, dy.ctypes.data)
    return dy
