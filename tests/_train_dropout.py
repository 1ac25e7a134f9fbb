"""Fixtures of the dropout tests of the three training steps, shared by the CPU and the GPU side, and the driver of
tests/hostsim_dropout -- test infrastructure only.

The cases are those of tests/_train.py, tests/_train_sym.py and tests/_train_lv.py -- the same boards, rows, networks and
loss weights -- with the masks of tests/_dropout_np.py on top (tests/_train_dropout_np.py ``with_masks``). As there, every
fixture a gradient is compared on is named here, so that tests/test_train_dropout_np.py can assert the ReLU guard for exactly
the list tests/test_gpu_train_dropout.py runs. A mask changes every value behind the first dropout, so the guard was found
again with the masks applied: the network and the rows of a shape stay the ones whose first layer already passes, and the
dropout seed is the first, from 0 on, for which every pre-ReLU value of the float64 restatement is at least ``MARGIN`` from
zero (``find_dropout_seed``; run on the CPU once, the results are the tables below).
"""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import _dropout_np as D
import _train as TR
import _train_dropout_np as ND
import _train_lv as TL
import _train_lv_np as NL
import _train_np as N
import _train_sym as TS
import _train_sym_np as NS
from _train import MARGIN  # noqa: F401

HERE = Path(__file__).resolve().parent / "hostsim_dropout"
GOLD = Path(__file__).resolve().parent / "golden" / "train_dropout"
ARCHS = ("mlp", "symmetric", "local_value")
FIXTURES = dict(mlp=TR, symmetric=TS, local_value=TL)
KEYS = dict(mlp=N, symmetric=NS, local_value=NL)
N_CALLS = dict(mlp=2, symmetric=7, local_value=2)
# name -> architecture (tools/gen_train_dropout_golden.py)
GOLDEN = {"mlp_5x5_h32_n33_p10": "mlp", "mlp_7x5_h64_n70_p50": "mlp", "sym_5x5_h32_n2_p10": "symmetric",
          "sym_5x5_h32_n33_p10": "symmetric", "lv_5x5_h32_n33_p10": "local_value"}

P = 0.1
STEP = 0
# Per architecture, the entries of its own SHAPES with n = 2, 33, 129 and 300 (and H = 256: SymmetricMLP's list has the
# full width at n = 40 and n = 300 at H = 64, both are taken: at 300 x 256 its seven BatchNorm calls have 537 600 pre-ReLU
# values, of which 23 to 63, 43 on average, lay within MARGIN of zero for each of the network seeds 1 .. 8, so no seed
# within reach passes the guard) and, per entry, the dropout seed found for it.
SHAPE_INDEX = dict(mlp=(0, 1, 2, 3), symmetric=(0, 1, 2, 3, 4), local_value=(0, 1, 2, 3))
SHAPE_DROPOUT_SEED = dict(mlp=(0, 0, 0, 13), symmetric=(0, 0, 1, 293, 11), local_value=(0, 0, 3, 13))
# LocalValueMLP's trunk is PyRatMLP's network of the same shape, so the full-width shape takes that one's dropout seed, and
# the ownership head's seed is the first for which its hidden layer, fed the masked trunk output, passes as well
LV_OWN_SEED = {3: 804}
SHAPES = [(arch, i, s) for arch in ARCHS for i, s in zip(SHAPE_INDEX[arch], SHAPE_DROPOUT_SEED[arch])]
SHAPE_IDS = [f"{arch}-{FIXTURES[arch].SHAPE_IDS[i]}" for arch, i, _ in SHAPES]
# two windows of one order through grad_iter, steps 0 and 1 of one seed: (architecture, board, H, batch, network seed
# [, ownership head's seed]), then the dropout seed found for both windows
ITER_BOARD, ITER_H, ITER_BATCH, ITER_PLAN_SEED = "7x5", 64, 32, 5
ITER_NET_SEED = dict(mlp=(2,), symmetric=(3,), local_value=(2, 0))
ITER_DROPOUT_SEED = dict(mlp=1, symmetric=5, local_value=1)


def plain_shape_case(arch: str, index: int) -> dict:
    fx = FIXTURES[arch]
    shape = fx.SHAPES[index]
    if arch == "local_value" and index in LV_OWN_SEED:
        shape = shape[:4] + (LV_OWN_SEED[index],)
    return fx.shape_case(*shape)


def shape_case(arch: str, index: int, dropout_seed: int, step: int = STEP, p: float = P) -> dict:
    """the architecture's own shape case with the masks of (dropout_seed, step)"""
    return ND.with_masks(plain_shape_case(arch, index), dropout_seed, step, p, N_CALLS[arch])


def find_dropout_seed(arch: str, cases, steps=(STEP,), p: float = P, limit: int = 100000) -> int:
    """the first dropout seed whose masks keep every case (case i at step steps[i]) at least MARGIN from every ReLU's zero"""
    for seed in range(limit):
        if all(ND.relu_margin(arch, ND.with_masks(c, seed, s, p, N_CALLS[arch])) >= MARGIN for c, s in zip(cases, steps)):
            return seed
    raise RuntimeError("no seed found")


def iter_cases(arch: str) -> list:
    """the two batches grad_iter cuts from epoch 0 of the plan over ITER_BOARD, as plain cases in step order"""
    from alpharat_amd.dataset import batch_windows, epoch_plan

    fx = FIXTURES[arch]
    _, plain = TR.board(ITER_BOARD)
    w, h = TR.BOARDS[ITER_BOARD][1], TR.BOARDS[ITER_BOARD][2]
    total = len(plain["value_p1"])
    order, mask = epoch_plan(total, ITER_PLAN_SEED, 0)  # grad_iter's defaults
    windows = batch_windows(total, ITER_BATCH, True)[:2]
    assert len(windows) == 2
    if arch == "mlp":
        from _random_nets import random_mlp

        sd = random_mlp(w, h, ITER_H, *ITER_NET_SEED[arch])
    elif arch == "symmetric":
        from _random_nets import random_symmetric

        sd = random_symmetric(w, h, ITER_H, *ITER_NET_SEED[arch])
    else:
        sd = TL.random_lv(w, h, ITER_H, *ITER_NET_SEED[arch])
    return [fx.make_case(ITER_BOARD, sd, order[f:f + n], mask[order[f:f + n]]) for f, n in windows]


def golden_case(name: str) -> dict:
    """a golden as a case of tests/_train_dropout_np.py, with the reference's results under "f32" and "f64"; its ``scale`` is
    the float64 1 / (1 - p) the generator's hooks divide by"""
    arch = GOLDEN[name]
    K = KEYS[arch]
    with np.load(GOLD / f"{name}.npz") as z:
        a = {k: z[k] for k in z.files}
    assert str(a["architecture"]) == arch
    rows = ("observation", "policy_p1", "policy_p2", "value_p1", "value_p2") + (("cheese_outcomes",) if arch == "local_value" else ())
    case = dict(arch=arch, sd={k[3:]: v for k, v in a.items() if k.startswith("sd/")}, board=str(a["board"]), order=a["order"],
                swap=a["swap"], width=int(a["width"]), height=int(a["height"]), hidden=int(a["hidden"]),
                policy_weight=float(a["weights"][0]), value_weight=float(a["weights"][1]), p=float(a["p"]),
                dropout_seed=int(a["dropout_seed"]), dropout_step=int(a["dropout_step"]),
                masks=[a[f"mask/{c}"].astype(bool) for c in range(N_CALLS[arch])], scale=1.0 / (1.0 - float(a["p"])),
                **{k: a[k] for k in rows})
    if arch == "local_value":
        case["ownership_weight"] = float(a["weights"][2])
    for tag in ("f32", "f64"):
        case[tag] = dict(losses={k: a[f"{tag}/{k}"] for k in K.LOSS_KEYS}, **{k: a[f"{tag}/{k}"] for k in K.OUT_KEYS},
                         grads={k: a[f"{tag}/grad/{k}"] for k in K.PARAM_KEYS},
                         running={k: a[f"{tag}/running/{k}"] for k in K.RUNNING_KEYS})
    return case


# ---- tests/hostsim_dropout ----------------------------------------------------------------------------------------------
_sim = None


def sim() -> C.CDLL:
    global _sim
    if _sim is None:
        subprocess.run(["make", "-s", "-C", str(HERE)], check=True)
        L = C.CDLL(str(HERE / "libdropoutsim.so"))
        L.ds_key.restype = L.ds_thr.restype = L.ds_mix.restype = C.c_uint64
        L.ds_key.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
        L.ds_thr.argtypes = [C.c_float]
        L.ds_mix.argtypes = [C.c_uint64]
        L.ds_scale.restype = C.c_float
        L.ds_scale.argtypes = [C.c_float]
        L.ds_mask.restype = None
        L.ds_mask.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
        _sim = L
    return _sim


def sim_mask(seed: int, step: int, call: int, n: int, H: int, p: float, with_bits: bool = False):
    """dev_dropout.h over a call's [n][H] array: the bool mask (and the elements' 64 bits)"""
    keep = np.zeros((n, H), np.uint8)
    bits = np.zeros((n, H), np.uint64) if with_bits else None
    sim().ds_mask(seed & (2 ** 64 - 1), step & (2 ** 64 - 1), call, n, H, float(p), keep.ctypes.data,
                  bits.ctypes.data if with_bits else None)
    return (keep.astype(bool), bits) if with_bits else keep.astype(bool)
