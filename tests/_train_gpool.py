"""Fixtures of the tests of PyRatCNN's training step with GPoolResBlocks and dropout, shared by the CPU and the GPU side, and
the driver of tests/hostsim_train_gpool -- test infrastructure only.

tests/_train_cnn.py's two kinds of case, under two guards. The ReLU guard is that file's. Its twin for the maximum: per
(row, channel) of every gpool block the largest ``pz`` of the row's cells is at least ``GUARD_FACTOR`` times ``max|pz32 -
pz64|`` above the second largest, so a float32 and a float64 evaluation pick the same cell and a tolerance means something.
The goldens (tests/golden/train_gpool, the reference's own model) store both pairs of numbers; the seeds of the shape cases
below were searched under both guards, and tests/test_train_gpool_np.py asserts them for exactly the list the GPU test
runs. The tie cases have exact ties on purpose and are held to the ReLU guard alone.

A gpool block as block 0 sees x_0, which is the same at two cells whose 3x3 neighbourhoods of the input are the same: on an
open board wider than five cells such cells exist (two cells of the second row with no cheese near them), and their pz tie
exactly. The cases with a gpool block first therefore use the 5x5 board, where every cell's neighbourhood is its own, or --
the 7x5 golden -- rows drawn from the positions no two cells of which see the same input (``distinct_neighbourhoods``).
"""
from __future__ import annotations

import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

import _train_cnn_np as NC
import _train_gpool_np as NG
import _train_np as N
from _train import BOARDS, WEIGHTS, assert_grads_within, board, make_case, repeated_order  # noqa: F401
from _train_cnn import DECIDED_MARGIN, GUARD_FACTOR, assert_values_within  # noqa: F401

HERE = Path(__file__).resolve().parent / "hostsim_train_gpool"
GOLD = Path(__file__).resolve().parent / "golden" / "train_gpool"
# name, board, C, blocks, n, dropout (PD 32, HD 64: CNNModelConfig's defaults); the dropout's (seed, step)
GOLDEN_CASES = [("gpool_5x5_c32_g32_n2", "5x5 open", 32, (32,), 2, 0.0), ("gpool_5x5_c32_r_g16_n12_p10", "5x5 open", 32, (0, 16), 12, 0.1),
                ("gpool_7x5_c32_g32_r_n8", "7x5", 32, (32, 0), 8, 0.0)]
GOLDEN = tuple(c[0] for c in GOLDEN_CASES)
GOLDEN_DROPOUT = (11, 2)

# (board, C, blocks, n, PD, HD, seed): the shapes of the device test, each the smallest that reaches one thing
SHAPES = [("5x5 open", 32, (0, 8), 3, 32, 64, 1),         # G = 8: below a tile
          ("5x5 open", 32, (0, 36), 3, 32, 64, 2),        # 2G = 72 is no multiple of the k chunk, G none of a tile
          ("5x5 open", 256, (256,), 2, 32, 64, 3),        # the full widths
          ("5x5 open", 32, (16, 0), 4, 32, 64, 4),        # a gpool block as block 0, a block behind it: a dense g
          ("5x5 open", 32, (16, 32), 3, 32, 64, 105),       # two gpool blocks in a row
          ("7x7", 64, (0, 0, 32), 4, 32, 64, 6),          # the shipped network (configs/train_cnn_7x7.yaml)
          ("2x1", 32, (8,), 5, 32, 64, 7),                # a 2-cell board, the smallest hw
          ("16x16", 32, (0, 16), 2, 32, 64, 108),           # the 256-cell reduction
          ("7x5", 32, (0, 16), 33, 32, 64, 109)]            # 1155 rows: several parts and split ranges, none a multiple of 64
SHAPE_IDS = [f"{b.replace(' ', '_')}-c{Ch}-{'_'.join(f'g{g}' if g else 'r' for g in blocks)}-n{n}" for b, Ch, blocks, n, *_ in SHAPES]
# the windows, the swap and the player-cell fixtures of tests/_train_cnn.py, with this trunk
FIXTURE_BLOCKS, FIXTURE_SEED = (0, 16), 32
# ties: every cell of every channel (pool_bn.weight = 0), and the channels whose pool_conv row is zero
TIE_SHAPE = ("5x5 open", 32, (0, 16), 4, 32, 64, 41)
# dropout: (seed, rate) of the device tests, over SHAPES[5] and the trajectory
DROPOUT_SEED, DROPOUT_P = 5, 0.1
# two steps of AdamW
TRAJ_BOARD, TRAJ_DIMS, TRAJ_BLOCKS, TRAJ_BATCH, TRAJ_STEPS, TRAJ_LR, TRAJ_SEED, TRAJ_PLAN_SEED = "5x5 open", (32, 32, 64), (0, 16), 16, 2, 1e-3, 21, 7


TINY_BOARD = "2x1"


@functools.lru_cache(maxsize=None)
def tiny_board_games() -> tuple:
    """(games, stacked rows) of a 2x1 set: three scripted games of three turns, both players on the cell beside the cheese;
    in the last turn P1, P2 or both step onto it, so the value targets are 1 / 0, 0 / 1 and 0.5 / 0.5. (Games nobody scores
    in have targets of 0, and loss_value would be the square of a softplus tail: a quantity whose relative error is twice the
    absolute error of the value logit, which says nothing about the step.)"""
    import _oracle as O
    import _rows as T
    import _rows_np as R

    right, left, stay = 1, 3, 4
    scripts = (((0, 0), (1, 0), (right, stay)), ((1, 0), (0, 0), (stay, left)), ((0, 0), (1, 0), (right, right)))
    games = [T.scripted(O.Game(2, 1, 3, p1=p, p2=p, cheese=[c]), [(stay, stay)] * 2 + [last], index=i)
             for i, (p, c, last) in enumerate(scripts)]
    return games, R.stack_rows(games)


def board_rows(name: str) -> tuple:
    """tests/_train.py ``board`` with the 2x1 set: (games, stacked rows, width, height)"""
    if name == TINY_BOARD:
        return tiny_board_games() + (2, 1)
    return board(name) + (BOARDS[name][1], BOARDS[name][2])


def distinct_neighbourhoods(observation, width: int, height: int) -> bool:
    """no two cells of any row see the same 3x3 neighbourhood of the stem's five input planes"""
    spatial = NC.parse_obs(np.asarray(observation, np.float64), width, height)[0]
    padded = np.pad(spatial, ((0, 0), (1, 1), (1, 1), (0, 0)), constant_values=-1.0)
    for row in padded:
        seen = {row[y:y + 3, x:x + 3].tobytes() for y in range(height) for x in range(width)}
        if len(seen) != width * height:
            return False
    return True


def use_layer_weights(blocks) -> None:
    """tests/_train.py grad_bounds reads tests/_train_np.py LAYER_WEIGHT: the names of this trunk"""
    N.LAYER_WEIGHT.update({k: NG.layer_weight(k) for k in NG.param_keys(blocks)})


def shape_case(board_name: str, Ch: int, blocks, n: int, PD: int, HD: int, seed: int) -> dict:
    _, plain, w, h = board_rows(board_name)
    order, swap = repeated_order(len(plain["value_p1"]), n, seed)
    sd = NG.random_gpool_cnn(w, h, Ch, PD, HD, blocks, seed)
    if board_name != TINY_BOARD:
        return make_case(board_name, sd, order, swap)
    import _augment_np as A
    import _rows_np as R

    rows = A.swap_rows(R.take(plain, order), swap, w, h)
    return dict(sd=sd, board=board_name, order=order, swap=swap, width=w, height=h, observation=rows["observation"],
                policy_p1=rows["policy_p1"], policy_p2=rows["policy_p2"], value_p1=rows["value_p1"].reshape(-1),
                value_p2=rows["value_p2"].reshape(-1), **WEIGHTS)


def dims_of(case: dict) -> tuple:
    sd = case["sd"]
    return (sd["stem.weight"].shape[0], sd["player_encoder.0.weight"].shape[0], sd["combiner.0.weight"].shape[0], NC.n_blocks_of(sd))


def with_trunk(case: dict, blocks=FIXTURE_BLOCKS, seed: int = FIXTURE_SEED) -> dict:
    """a case of tests/_train_cnn.py (5x5 or 7x5, C = 32 or 64) with a network of this trunk instead of its own"""
    Ch, PD, HD, _ = (int(v) for v in (case["sd"]["stem.weight"].shape[0], case["sd"]["player_encoder.0.weight"].shape[0],
                                     case["sd"]["combiner.0.weight"].shape[0], 0))
    return dict(case, sd=NG.random_gpool_cnn(int(case["width"]), int(case["height"]), Ch, PD, HD, blocks, seed))


def tie_cases() -> tuple:
    """(every cell ties, some channels tie): TIE_SHAPE's network with ``pool_bn.weight = 0`` and ``pool_bn.bias = 4`` in the
    gpool block -- ap is then the constant 4 and every cell of every channel holds the maximum, exactly in every precision
    (pz is the same sum of the same numbers at every cell) --, and with the first five rows of ``pool_conv.weight`` zero,
    whose channels are 0 at every cell"""
    base = shape_case(*TIE_SHAPE)
    b = [i for i, g in enumerate(TIE_SHAPE[2]) if g][0]
    every = dict(base, sd=dict(base["sd"]))
    every["sd"][f"blocks.{b}.pool_bn.weight"] = np.zeros_like(base["sd"][f"blocks.{b}.pool_bn.weight"])
    every["sd"][f"blocks.{b}.pool_bn.bias"] = np.full_like(base["sd"][f"blocks.{b}.pool_bn.bias"], 4.0)
    some = dict(base, sd=dict(base["sd"]))
    wc = base["sd"][f"blocks.{b}.pool_conv.weight"].copy()
    wc[:5] = 0.0
    some["sd"][f"blocks.{b}.pool_conv.weight"] = wc
    return every, some


def guards(case: dict, r64: dict | None = None, r32: dict | None = None) -> dict:
    """the four guard numbers of a case: ``pre_min`` and ``pre_err`` of tests/_train_cnn.py, and ``max_gap`` (the smallest
    gap between the largest and the second largest pz of a (row, channel) in float64) and ``pz_err`` (max|pz32 - pz64|);
    float64 is the NumPy step, float32 the autograd restatement on the CPU"""
    import torch

    import _gpool_train_torch as GT

    r64 = r64 if r64 is not None else NG.step(case)
    r32 = r32 if r32 is not None else GT.step(case, torch.float32, "cpu")
    nhwc = lambda a: a if a.ndim != 4 else np.transpose(a, (0, 2, 3, 1))  # noqa: E731
    pre_err = max(float(np.abs(nhwc(a).astype(np.float64) - b).max()) for a, b in zip(r32["pre"], r64["pre"]))
    pz_err = max((float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(r32["pz"], r64["pz"])), default=0.0)
    return dict(pre_min=NG.relu_margin(r64), pre_err=pre_err, max_gap=NG.max_gap(r64["pz"]), pz_err=pz_err)


def guards_hold(g: dict, with_max: bool = True) -> bool:
    return g["pre_min"] >= GUARD_FACTOR * g["pre_err"] and (not with_max or g["max_gap"] >= GUARD_FACTOR * g["pz_err"])


def golden_case(name: str) -> dict:
    """a golden as a case, with the reference's results under "f32" and "f64" (losses, outputs, grads, running), the
    generator's four guard numbers and, for a dropout case, the masks and the float64 1 / (1 - p) its hooks divide by"""
    a = {}
    for file in (f"{name}.npz", f"{name}.f64.npz"):
        with np.load(GOLD / file) as z:
            a.update({k: z[k] for k in z.files})
    sd = {k[3:]: v for k, v in a.items() if k.startswith("sd/")}
    blocks = NG.blocks_of(sd)
    case = dict(sd=sd, board=str(a["board"]), order=a["order"], swap=a["swap"], width=int(a["width"]), height=int(a["height"]),
                policy_weight=float(a["weights"][0]), value_weight=float(a["weights"][1]),
                **{k: float(a[k]) for k in ("pre_err", "pre_min", "pz_err", "max_gap")},
                **{k: a[k] for k in ("observation", "policy_p1", "policy_p2", "value_p1", "value_p2")})
    if float(a["p"]) != 0:
        case.update(masks=[a[f"mask/{c}"].astype(bool) for c in range(4)], p=float(a["p"]), scale=1.0 / (1.0 - float(a["p"])),
                    dropout_seed=int(a["dropout_seed"]), dropout_step=int(a["dropout_step"]))
    for tag in ("f32", "f64"):
        case[tag] = dict(losses={k: a[f"{tag}/{k}"] for k in NC.LOSS_KEYS}, **{k: a[f"{tag}/{k}"] for k in NC.OUT_KEYS},
                         grads={k: a[f"{tag}/grad/{k}"] for k in NG.param_keys(blocks)},
                         running={k: a[f"{tag}/running/{k}"] for k in NG.running_keys(blocks)})
    return case


def trajectory_plan() -> tuple:
    """tests/_train_cnn.py trajectory_plan for this file's board, batch and plan seed"""
    from alpharat_amd.dataset import batch_windows, epoch_plan

    _, plain = board(TRAJ_BOARD)
    total = len(plain["value_p1"])
    steps, epochs, epoch = [], [], 0
    while len(steps) < TRAJ_STEPS:
        order, mask = epoch_plan(total, TRAJ_PLAN_SEED, epoch, True, False)
        epochs.append((epoch, order, mask))
        steps += [(epoch, first) for first, n in batch_windows(total, TRAJ_BATCH, True)]
        epoch += 1
        assert epoch < 50, "the board has fewer rows than a batch"
    return epochs, steps[:TRAJ_STEPS]


# ---- tests/hostsim_train_gpool -----------------------------------------------------------------------------------------------
_sim = None


def sim() -> C.CDLL:
    global _sim
    if _sim is None:
        subprocess.run(["make", "-s", "-C", str(HERE)], check=True)
        L = C.CDLL(str(HERE / "libtraingpoolsim.so"))
        L.tgs_reduce.restype = L.tgs_dpz.restype = None
        L.tgs_reduce.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p]
        L.tgs_dpz.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_float, C.c_float, C.c_void_p]
        _sim = L
    return _sim


def sim_reduce(z, stride: int = 1) -> tuple:
    """dev_train_gpool.h gpool_reduce over z[0], z[stride], ...: (mean, max, count)"""
    z = np.ascontiguousarray(z, np.float32)
    mm, count = np.zeros(2, np.float32), np.zeros(1, np.int32)
    sim().tgs_reduce(z.ctypes.data, len(z) // stride, stride, mm.ctypes.data, count.ctypes.data)
    return float(mm[0]), float(mm[1]), int(count[0])


def sim_dpz(z, dmean: float, dmax: float, stride: int = 1) -> np.ndarray:
    """gpool_dpz of every cell of one (row, channel), from gpool_reduce's maximum and count"""
    z = np.ascontiguousarray(z, np.float32)
    out = np.zeros(len(z) // stride, np.float32)
    sim().tgs_dpz(z.ctypes.data, len(out), stride, dmean, dmax, out.ctypes.data)
    return out
