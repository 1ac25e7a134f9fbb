"""Fixtures of the PyRatCNN training-step tests, shared by the CPU and the GPU side, and the driver of
tests/hostsim_train_cnn -- test infrastructure only.

Two kinds of case. The goldens (tests/golden/train_cnn, the reference's own model) are small enough that a weight seed
exists whose every pre-ReLU value is at least eight times as far from zero as float32 and float64 differ there; the
generator stores both numbers and tests/test_train_cnn_np.py asserts the inequality. The shape cases are too large for
any seed (a convolutional BatchNorm has n hw C outputs), so their networks have decided ReLU signs
(tests/_train_cnn_np.py ``random_cnn``): the CPU test asserts ``relu_margin >= DECIDED_MARGIN`` for exactly the list the
GPU test runs.

The tolerance is tests/_train.py's ``grad_bounds`` and tests/_train_sym.py's ``assert_values_within``; the table of layer
weights gains PyRatCNN's names for the block count at hand (``use_layer_weights``).
"""
from __future__ import annotations

import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

import _train_cnn_np as NC
import _train_np as N
from _train import BOARDS, WEIGHTS, assert_grads_within, board, make_case, repeated_order  # noqa: F401
from _train_sym import assert_values_within, value_bound  # noqa: F401

HERE = Path(__file__).resolve().parent / "hostsim_train_cnn"
GOLD = Path(__file__).resolve().parent / "golden" / "train_cnn"
# name, board, C, B, n (PD 32, HD 64: CNNModelConfig's defaults)
GOLDEN_CASES = [("cnn_5x5_c32_b1_n2", "5x5 open", 32, 1, 2), ("cnn_5x5_c32_b2_n12", "5x5 open", 32, 2, 12),
                ("cnn_7x5_c64_b1_n8", "7x5", 64, 1, 8)]
GOLDEN = tuple(c[0] for c in GOLDEN_CASES)
GUARD_FACTOR = 8.0      # a golden's min|pre64| is at least this many times max|pre32 - pre64|
DECIDED_MARGIN = 0.25   # a decided network's min|pre64|

# (board, C, B, n, PD, HD, seed): the shapes of the device test; n = None: the smallest n whose n hw rows are over both caps
# of the partitions (read through the hostsim)
SHAPES = [("5x5 open", 32, 0, 3, 32, 64, 1),     # the stem alone
          ("5x5 open", 32, 1, 2, 32, 64, 2),     # 50 rows: one part, every tail
          ("7x5", 64, 2, 33, 32, 64, 3),         # 1155 rows: several parts and splits, none a multiple of 64
          ("7x7", 96, 1, 5, 32, 64, 4),          # a column-tile tail, K = 864
          ("5x5 open", 256, 1, 3, 32, 64, 5),    # the full width
          ("16x16", 32, 1, 2, 32, 64, 6),        # the largest board
          ("5x5 open", 32, 8, 2, 32, 64, 8),     # every block slot (seed 7 has a value 0.07 from zero)
          ("5x5 open", 32, 1, 4, 24, 32, 8),     # PD = 24, HD = 32
          ("5x5 open", 32, 1, None, 32, 64, 9)]  # both caps of the partitions
SHAPE_IDS = [f"{b.replace(' ', '_')}-c{Ch}-b{B}-n{n if n is not None else 'caps'}-pd{PD}-hd{HD}" for b, Ch, B, n, PD, HD, _ in SHAPES]
# one order of 30 rows, three windows of it
WINDOW_BOARD, WINDOW_DIMS, WINDOW_ROWS, WINDOW_SEED = "7x5", (64, 32, 64, 1), 30, 11
WINDOWS = [(0, 12), (12, 12), (24, 6)]
# five steps: two are asked for, AdamW
TRAJ_BOARD, TRAJ_DIMS, TRAJ_BATCH, TRAJ_STEPS, TRAJ_LR, TRAJ_SEED, TRAJ_PLAN_SEED = "5x5 open", (32, 32, 64, 1), 16, 2, 1e-3, 21, 7


def use_layer_weights(n_blocks: int) -> None:
    """tests/_train.py grad_bounds reads tests/_train_np.py LAYER_WEIGHT: PyRatCNN's names for this many blocks"""
    N.LAYER_WEIGHT.update({k: NC.layer_weight(k) for k in NC.param_keys(n_blocks)})


def caps_rows(hw: int) -> int:
    """the smallest n whose n * hw rows are over both caps: more than CNN_MAX_PARTS parts of CNN_PART_ROWS rows and more than
    CNN_MAX_SPLITS ranges of CNN_SPLIT_ROWS rows would be needed"""
    max_parts, part_rows, max_splits, split_rows = sim_caps()
    return max(max_parts * part_rows, max_splits * split_rows) // hw + 1


def shape_case(board_name: str, Ch: int, B: int, n, PD: int, HD: int, seed: int) -> dict:
    _, plain = board(board_name)
    w, h = BOARDS[board_name][1], BOARDS[board_name][2]
    if n is None:
        n = caps_rows(w * h)
    order, swap = repeated_order(len(plain["value_p1"]), n, seed)
    return make_case(board_name, NC.random_cnn(w, h, Ch, PD, HD, B, seed), order, swap)


def dims_of(case: dict) -> tuple:
    sd = case["sd"]
    return (sd["stem.weight"].shape[0], sd["player_encoder.0.weight"].shape[0], sd["combiner.0.weight"].shape[0], NC.n_blocks_of(sd))


def window_cases() -> tuple:
    """the whole order's case (rows, swap, network) and one case per window"""
    _, plain = board(WINDOW_BOARD)
    w, h = BOARDS[WINDOW_BOARD][1], BOARDS[WINDOW_BOARD][2]
    order, swap = repeated_order(len(plain["value_p1"]), WINDOW_ROWS, WINDOW_SEED)
    Ch, PD, HD, B = WINDOW_DIMS
    whole = make_case(WINDOW_BOARD, NC.random_cnn(w, h, Ch, PD, HD, B, WINDOW_SEED), order, swap)
    return whole, [make_case(WINDOW_BOARD, whole["sd"], whole["order"][f:f + n], whole["swap"][f:f + n]) for f, n in WINDOWS]


def swap_cases() -> tuple:
    """(unswapped, all swapped) over the same rows and network"""
    name, rows, seed = "5x5 open", 10, 12
    _, plain = board(name)
    order = np.random.default_rng(seed).permutation(len(plain["value_p1"]))[:rows]
    sd = NC.random_cnn(5, 5, 32, 32, 64, 1, seed)
    return make_case(name, sd, order, np.zeros(rows, bool)), make_case(name, sd, order, np.ones(rows, bool))


@functools.lru_cache(maxsize=None)
def player_cell_games() -> tuple:
    """(games, stacked rows, picked rows) of a 5x5 set of its own: the played games of "5x5 open" and two scripted ones whose
    players stand still in the four corners; the picks cover both players on one cell and a player in each corner"""
    import _oracle as O
    import _rows as T
    import _rows_np as R

    games = list(board("5x5 open")[0])
    for i, (p1, p2) in enumerate((((4, 0), (0, 4)), ((0, 0), (4, 4)))):
        og = O.Game(5, 5, 2, p1=p1, p2=p2, cheese=[(2, 2), (1, 3), (3, 1)])
        games.append(T.scripted(og, [(4, 4), (4, 4)], index=len(games)))
    plain = R.stack_rows(games)
    obs = plain["observation"]
    c1, c2 = obs[:, 100:125].argmax(axis=1), obs[:, 125:150].argmax(axis=1)
    same = np.flatnonzero(c1 == c2)
    assert len(same), "no position has both players on one cell"
    picks = [int(same[0])]
    for corner in (0, 4, 20, 24):
        at = np.flatnonzero((c1 == corner) | (c2 == corner))
        assert len(at), f"no position has a player on cell {corner}"
        picks.append(int(at[-1]))
    return games, plain, np.asarray(picks, np.int64)


def player_cell_case() -> dict:
    """the picks of player_cell_games and a few more rows, half of them swapped"""
    import _augment_np as A
    import _rows_np as R

    seed = 13
    _, plain, picks = player_cell_games()
    rng = np.random.default_rng(seed)
    order = np.concatenate([picks, rng.permutation(len(plain["value_p1"]))[:3]])
    swap = np.arange(len(order)) % 2 == 1
    rows = A.swap_rows(R.take(plain, order), swap, 5, 5)
    return dict(sd=NC.random_cnn(5, 5, 32, 32, 64, 1, seed), board="player cells", order=order, swap=swap, width=5, height=5,
                observation=rows["observation"], policy_p1=rows["policy_p1"], policy_p2=rows["policy_p2"],
                value_p1=rows["value_p1"].reshape(-1), value_p2=rows["value_p2"].reshape(-1), **WEIGHTS)


def golden_case(name: str) -> dict:
    """a golden as a case, with the reference's results under "f32" and "f64" (losses, outputs, grads, running) and the
    generator's two guard numbers"""
    a = {}
    for file in (f"{name}.npz", f"{name}.f64.npz"):  # the case and the float32 results; the float64 results
        with np.load(GOLD / file) as z:
            a.update({k: z[k] for k in z.files})
    sd = {k[3:]: v for k, v in a.items() if k.startswith("sd/")}
    B = NC.n_blocks_of(sd)
    case = dict(sd=sd, board=str(a["board"]), order=a["order"], swap=a["swap"], width=int(a["width"]), height=int(a["height"]),
                policy_weight=float(a["weights"][0]), value_weight=float(a["weights"][1]),
                pre_err=float(a["pre_err"]), pre_min=float(a["pre_min"]),
                **{k: a[k] for k in ("observation", "policy_p1", "policy_p2", "value_p1", "value_p2")})
    for tag in ("f32", "f64"):
        case[tag] = dict(losses={k: a[f"{tag}/{k}"] for k in NC.LOSS_KEYS}, **{k: a[f"{tag}/{k}"] for k in NC.OUT_KEYS},
                         grads={k: a[f"{tag}/grad/{k}"] for k in NC.param_keys(B)},
                         running={k: a[f"{tag}/running/{k}"] for k in NC.running_keys(B)})
    return case


def trajectory_plan() -> tuple:
    """tests/_train_sym.py trajectory_plan for this file's board, batch and plan seed"""
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


# ---- tests/hostsim_train_cnn -------------------------------------------------------------------------------------------------
_sim = None


def sim() -> C.CDLL:
    global _sim
    if _sim is None:
        subprocess.run(["make", "-s", "-C", str(HERE)], check=True)
        L = C.CDLL(str(HERE / "libtraincnnsim.so"))
        L.tcs_nbr.restype = L.tcs_mirror.restype = C.c_int
        L.tcs_nbr.argtypes = [C.c_int] * 4
        L.tcs_mirror.argtypes = [C.c_int]
        L.tcs_split.restype = L.tcs_cols.restype = L.tcs_rows_split.restype = L.tcs_caps.restype = None
        L.tcs_split.argtypes = [C.c_uint64, C.c_int] + [C.c_void_p] * 4
        L.tcs_cols.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.tcs_rows_split.argtypes = [C.c_int, C.c_int, C.c_void_p]
        L.tcs_caps.argtypes = [C.c_void_p]
        _sim = L
    return _sim


def sim_nbr(cell: int, tap: int, bw: int, bh: int) -> int:
    return int(sim().tcs_nbr(cell, tap, bw, bh))


def sim_mirror(tap: int) -> int:
    return int(sim().tcs_mirror(tap))


def sim_split(x, width: int, height: int):
    """dev_train_cnn.h over rows: x5 (n hw, 5), side (2n, 3), cells (2n,), P1's rows first"""
    x = np.ascontiguousarray(x, np.float32)
    n, hw = len(x), width * height
    x5, side, cells = np.zeros((n * hw, 5), np.float32), np.zeros((2 * n, 3), np.float32), np.zeros(2 * n, np.int32)
    sim().tcs_split(n, hw, x.ctypes.data, x5.ctypes.data, side.ctypes.data, cells.ctypes.data)
    return x5, side, cells


def sim_cols(n: int, hw: int, Ch: int) -> tuple:
    """cnn_cols: (P, rpp)"""
    out = np.zeros(2, np.int32)
    sim().tcs_cols(n, hw, Ch, out.ctypes.data)
    return int(out[0]), int(out[1])


def sim_rows_split(n: int, hw: int) -> tuple:
    """cnn_split: (S, kps)"""
    out = np.zeros(2, np.int32)
    sim().tcs_rows_split(n, hw, out.ctypes.data)
    return int(out[0]), int(out[1])


@functools.lru_cache(maxsize=None)
def sim_caps() -> tuple:
    """(CNN_MAX_PARTS, CNN_PART_ROWS, CNN_MAX_SPLITS, CNN_SPLIT_ROWS)"""
    out = np.zeros(4, np.int32)
    sim().tcs_caps(out.ctypes.data)
    return tuple(int(v) for v in out)
