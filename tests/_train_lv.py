"""Fixtures of the LocalValueMLP training-step tests, shared by the CPU and the GPU side, and the driver of
tests/hostsim_train_lv -- test infrastructure only.

As in tests/_train.py, every fixture a gradient is compared on is named here, so that tests/test_train_lv_np.py can assert
the ReLU guard for exactly the list tests/test_gpu_train_lv.py runs: both BatchNorm outputs of the trunk and the ownership
head's hidden pre-activation of the float64 restatement are at least ``MARGIN`` from zero. The trunk and the three heads of a
fixture are tests/_train.py's own network for the same shape and seed (``random_mlp``), whose BatchNorm outputs pass that
file's guard over the same rows; the ownership head is drawn from a seed of its own, picked on the CPU until its hidden
layer passes too. The trajectory's pair of seeds was picked the same way over all five steps.

The tolerance is tests/_train.py's ``grad_bounds`` itself: its table of layer weights (tests/_train_np.py ``LAYER_WEIGHT``)
gains the ownership head's names here, by the same rule (a tensor's layer weight is ``<module>.weight``).
"""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import _augment_np as A
import _rows_np as R
import _train as TR
import _train_np as N
import _train_lv_np as NL
from _random_nets import random_mlp
from _train import BOARDS, MARGIN, board, repeated_order  # noqa: F401
from _train_sym import assert_values_within, value_bound  # noqa: F401  (the rule for what is not a gradient)

assert all(N.LAYER_WEIGHT.get(k, v) == v for k, v in NL.LAYER_WEIGHT.items())
N.LAYER_WEIGHT.update(NL.LAYER_WEIGHT)

HERE = Path(__file__).resolve().parent / "hostsim_train_lv"
GOLD = Path(__file__).resolve().parent / "golden" / "train_lv"
GOLDEN = ("lv_5x5_h32_n2", "lv_5x5_h32_n33", "lv_7x5_h64_n70")
WEIGHTS = dict(policy_weight=1.0, value_weight=0.5, ownership_weight=0.25)

# (board, H, n, seed, ownership head's seed): the shapes of the device test; board, H, n and seed are tests/_train.py SHAPES
OWN_SEEDS = (0, 0, 4, 79, 2, 0)
SHAPES = [s + (o,) for s, o in zip(TR.SHAPES, OWN_SEEDS)]
SHAPE_IDS = TR.SHAPE_IDS
# one order of 120 rows, three windows of it
WINDOW_BOARD, WINDOW_H, WINDOW_ROWS, WINDOW_SEED, WINDOWS = TR.WINDOW_BOARD, TR.WINDOW_H, TR.WINDOW_ROWS, TR.WINDOW_SEED, TR.WINDOWS
WINDOW_OWN_SEED = 0
# the same rows unswapped and all swapped
SWAP_BOARD, SWAP_H, SWAP_ROWS, SWAP_SEED, SWAP_OWN_SEED = TR.SWAP_BOARD, TR.SWAP_H, TR.SWAP_ROWS, TR.SWAP_SEED, 1
# five steps of SGD
TRAJ_BOARD, TRAJ_H, TRAJ_BATCH, TRAJ_STEPS, TRAJ_LR, TRAJ_PLAN_SEED = "7x7", 64, 64, 5, 0.05, 7
TRAJ_SEED, TRAJ_OWN_SEED = 29, 29


def random_lv(w: int, h: int, H: int, seed: int, own_seed: int) -> dict:
    """LocalValueMLP (architecture ``local_value``): tests/_random_nets.py ``random_mlp(w, h, H, seed)`` and the ownership
    head, drawn so that its logits tell classes and cells apart (weights std 1 / sqrt(H) and 2 / sqrt(H), biases std 0.5, as
    tools/gen_ownership_golden.py draws them)"""
    t = random_mlp(w, h, H, seed)
    rng = np.random.default_rng([own_seed, 0x6F776E])
    t["ownership_head.0.weight"] = (rng.standard_normal((H, H)) / np.sqrt(H)).astype(np.float32)
    t["ownership_head.0.bias"] = (0.5 * rng.standard_normal(H)).astype(np.float32)
    t["ownership_head.2.weight"] = (rng.standard_normal((4 * w * h, H)) * 2.0 / np.sqrt(H)).astype(np.float32)
    t["ownership_head.2.bias"] = (0.5 * rng.standard_normal(4 * w * h)).astype(np.float32)
    return t


def make_case(board_name: str, sd: dict, order, swap, weights: dict = WEIGHTS) -> dict:
    """tests/_train.py make_case with the rows' swapped cheese outcomes and the third weight"""
    _, plain = board(board_name)
    w, h = BOARDS[board_name][1], BOARDS[board_name][2]
    rows = A.swap_rows(R.take(plain, order), swap, w, h)
    return dict(sd=sd, board=board_name, order=np.asarray(order, np.int64), swap=np.asarray(swap, bool), width=w, height=h,
                observation=rows["observation"], policy_p1=rows["policy_p1"], policy_p2=rows["policy_p2"],
                value_p1=rows["value_p1"].reshape(-1), value_p2=rows["value_p2"].reshape(-1),
                cheese_outcomes=np.asarray(rows["cheese_outcomes"], np.int8), **weights)


def mlp_case(case: dict) -> dict:
    """the case of tests/_train_np.py over the same rows and the same trunk and heads"""
    return {k: v for k, v in case.items() if k not in ("cheese_outcomes", "ownership_weight")}


def shape_case(board_name: str, H: int, n: int, seed: int, own_seed: int) -> dict:
    _, plain = board(board_name)
    w, h = BOARDS[board_name][1], BOARDS[board_name][2]
    order, swap = repeated_order(len(plain["value_p1"]), n, seed)
    return make_case(board_name, random_lv(w, h, H, seed, own_seed), order, swap)


def window_cases() -> tuple:
    """the whole order's case (rows, swap, network) and one case per window"""
    whole = shape_case(WINDOW_BOARD, WINDOW_H, WINDOW_ROWS, WINDOW_SEED, WINDOW_OWN_SEED)
    return whole, [make_case(WINDOW_BOARD, whole["sd"], whole["order"][f:f + n], whole["swap"][f:f + n]) for f, n in WINDOWS]


def swap_cases() -> tuple:
    """(unswapped, all swapped) over the same rows and network"""
    _, plain = board(SWAP_BOARD)
    w, h = BOARDS[SWAP_BOARD][1], BOARDS[SWAP_BOARD][2]
    order = np.arange(SWAP_ROWS) % len(plain["value_p1"])
    sd = random_lv(w, h, SWAP_H, SWAP_SEED, SWAP_OWN_SEED)
    return (make_case(SWAP_BOARD, sd, order, np.zeros(SWAP_ROWS, bool)), make_case(SWAP_BOARD, sd, order, np.ones(SWAP_ROWS, bool)))


def golden_case(name: str) -> dict:
    """a golden as a case, with the reference's results under "f32" and "f64" (losses, outputs, grads, running)"""
    with np.load(GOLD / f"{name}.npz") as z:
        a = {k: z[k] for k in z.files}
    case = dict(sd={k[3:]: v for k, v in a.items() if k.startswith("sd/")}, board=str(a["board"]), order=a["order"], swap=a["swap"],
                width=int(a["width"]), height=int(a["height"]), hidden=int(a["hidden"]), policy_weight=float(a["weights"][0]),
                value_weight=float(a["weights"][1]), ownership_weight=float(a["weights"][2]),
                **{k: a[k] for k in ("observation", "policy_p1", "policy_p2", "value_p1", "value_p2", "cheese_outcomes")})
    for tag in ("f32", "f64"):
        case[tag] = dict(losses={k: a[f"{tag}/{k}"] for k in NL.LOSS_KEYS}, **{k: a[f"{tag}/{k}"] for k in NL.OUT_KEYS},
                         grads={k: a[f"{tag}/grad/{k}"] for k in NL.PARAM_KEYS},
                         running={k: a[f"{tag}/running/{k}"] for k in NL.RUNNING_KEYS})
    return case


def trajectory_plan() -> tuple:
    """tests/_train.py trajectory_plan for this file's board, batch and plan seed: the player swap at 0.5, the reference's
    augmentation for this architecture"""
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


def trajectory_cases_f64(seed: int = TRAJ_SEED, own_seed: int = TRAJ_OWN_SEED) -> list:
    """the float64 trajectory: per step its case (the network before the step) and the result of tests/_train_lv_np.py step;
    plain SGD, running statistics carried along. The last entry's "after" is the final state dict."""
    w, h = BOARDS[TRAJ_BOARD][1], BOARDS[TRAJ_BOARD][2]
    epochs, steps = trajectory_plan()
    plans = {e: (o, m) for e, o, m in epochs}
    sd = {k: np.asarray(v, np.float64) for k, v in random_lv(w, h, TRAJ_H, seed, own_seed).items()}
    out = []
    for epoch, first in steps:
        order, mask = plans[epoch]
        idx = order[first:first + TRAJ_BATCH]
        case = make_case(TRAJ_BOARD, dict(sd), idx, mask[idx])
        res = NL.step(case)
        sd = dict(sd)
        for k in NL.PARAM_KEYS:
            sd[k] = sd[k] - TRAJ_LR * res["grads"][k]
        sd.update(res["running"])
        out.append(dict(case=case, result=res, after=sd))
    return out


assert_grads_within = TR.assert_grads_within

# ---- tests/hostsim_train_lv ------------------------------------------------------------------------------------------------
CELL = np.dtype([("ce", np.float32), ("dl", np.float32, 4)])
_sim = None


def sim() -> C.CDLL:
    global _sim
    if _sim is None:
        subprocess.run(["make", "-s", "-C", str(HERE)], check=True)
        L = C.CDLL(str(HERE / "libtrainlvsim.so"))
        L.tls_cells.restype = None
        L.tls_cells.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
        L.tls_scale.restype = C.c_float
        L.tls_scale.argtypes = [C.c_float, C.c_uint32]
        L.tls_loss.restype = C.c_double
        L.tls_loss.argtypes = [C.c_double, C.c_uint32]
        L.tls_parts.restype = None
        L.tls_parts.argtypes = [C.c_int, C.c_int, C.c_void_p]
        L.tls_cell_words.restype = C.c_int
        assert L.tls_cell_words() * 4 == CELL.itemsize
        _sim = L
    return _sim


def sim_cells(logits, targets, scale: float) -> np.ndarray:
    """dev_train_lv.h lv_cell_terms over cells: logits (cells, 4), targets (cells,) int8; the cells' CELL records"""
    l = np.ascontiguousarray(logits, np.float32).reshape(-1, 4)
    t = np.ascontiguousarray(targets, np.int8).reshape(-1)
    assert len(l) == len(t)
    out = np.zeros(len(t), CELL)
    sim().tls_cells(len(t), l.ctypes.data, t.ctypes.data, scale, out.ctypes.data)
    return out


def sim_scale(ow: float, cells: int) -> float:
    """dev_train_lv.h lv_own_scale"""
    return float(sim().tls_scale(ow, cells))


def sim_loss(ce_sum: float, cells: int) -> float:
    """dev_train_lv.h lv_own_loss"""
    return float(sim().tls_loss(ce_sum, cells))


def sim_parts(n: int, hw: int) -> tuple:
    """dev_train_lv.h lv_cells: (B, rpb)"""
    out = np.zeros(2, np.int32)
    sim().tls_parts(n, hw, out.ctypes.data)
    return int(out[0]), int(out[1])
