"""Training shards from self-play records, built on the MI355X.

``prepare_training_set_with_split`` / ``prepare_training_set`` follow the reference's sharding step
(alpharat/data/sharding.py:73-385): games are split into train and val, the positions of each split are shuffled, and
``shard_NNNN.npz`` files with the eight ``BatchKey`` arrays (alpharat/nn/training/keys.py:52-62) are written beside a
``manifest.json``. Where the reference builds every row in a Python loop (``FlatObservationBuilder.build`` and
``build_targets`` once per position), the rows here come from ``ar_rows_build``: the games sit in a device-resident
``RowSet`` -- appended on the device by a session the set is attached to, or uploaded from records and bundles -- and the
shuffle is the gather index of the kernel that writes the rows.
"""
from __future__ import annotations

import ctypes as C
import json
import uuid
import weakref
from dataclasses import dataclass
from datetime import datetime, timezone
from pathlib import Path
from typing import Callable, Sequence

import numpy as np

from . import _lib

KEYS = ("observation", "policy_p1", "policy_p2", "value_p1", "value_p2", "action_p1", "action_p2", "cheese_outcomes")
BUILDER_VERSION = "flat_v2"  # alpharat/nn/builders/flat.py:117-120

# the 26 arrays of a bundle (crates/alpharat-sampling/src/recording.rs:23-162): per game, then per position
_BUNDLE_GAME = ("maze", "initial_cheese", "cheese_outcomes", "max_turns", "result", "final_p1_score", "final_p2_score")
_BUNDLE_POS = ("p1_pos", "p2_pos", "p1_score", "p2_score", "p1_mud", "p2_mud", "cheese_mask", "turn", "value_p1", "value_p2",
               "visit_counts_p1", "visit_counts_p2", "prior_p1", "prior_p2", "policy_p1", "policy_p2", "action_p1",
               "action_p2")
_U8 = ("p1_pos", "p2_pos", "p1_mud", "p2_mud", "cheese_mask", "action_p1", "action_p2")
_F32 = ("p1_score", "p2_score", "value_p1", "value_p2", "visit_counts_p1", "visit_counts_p2", "prior_p1", "prior_p2",
        "policy_p1", "policy_p2")


def read_bundle(path) -> list[dict]:
    """The games of one ``bundle_<uuid>.npz`` in file order, as record dicts (the keys of ``sampling.record_to_dict``;
    a bundle carries no game index: ``game_index`` is absent)."""
    with np.load(path) as z:
        if "game_lengths" not in z.files:  # the reference's single-game files (sharding.py:435-436) are not read here
            raise ValueError(f"{path} is not a bundle (no game_lengths array): only bundle_<uuid>.npz files are read")
        a = {k: z[k] for k in z.files}
    lengths = a["game_lengths"]
    h, w = a["maze"].shape[1:3]
    ends = np.cumsum(lengths)
    games = []
    for i in range(len(lengths)):
        lo, hi = int(ends[i] - lengths[i]), int(ends[i])
        g = dict(width=int(w), height=int(h), n=hi - lo)
        for k in _BUNDLE_GAME:
            g[k] = a[k][i]
        for k in _BUNDLE_POS:
            g[k] = a[k][lo:hi]
        g["max_turns"], g["result"] = int(g["max_turns"]), int(g["result"])
        g["cheese_mask"] = g["cheese_mask"].reshape(hi - lo, h * w)
        games.append(g)
    return games


def read_bundle_dirs(dirs: Sequence) -> list[dict]:
    """Every game of the bundles under the given batch directories (``<dir>/games/*.npz`` as the reference lays batches
    out, sharding.py:423-428, else ``<dir>/*.npz``), directories in the order given, files by name."""
    games: list[dict] = []
    for d in dirs:
        d = Path(d)
        src = d / "games" if (d / "games").is_dir() else d
        for f in sorted(src.glob("*.npz")):
            games.extend(read_bundle(f))
    return games


def _view_of(game: dict, keep: list) -> _lib.ArGameRecordView:
    v = _lib.ArGameRecordView()
    v.width, v.height, v.max_turns = int(game["width"]), int(game["height"]), int(game["max_turns"])
    v.game_index = int(game.get("game_index", 0))
    v.n_positions = len(np.asarray(game["turn"]))
    v.final_p1_score, v.final_p2_score = float(game["final_p1_score"]), float(game["final_p2_score"])
    v.result = int(game.get("result", 0))

    def ptr(key, dt, ct):
        a = np.array(game[key], dtype=dt, order="C", copy=True)
        keep.append(a)
        return a.ctypes.data_as(C.POINTER(ct))

    v.maze = ptr("maze", np.int8, C.c_int8)
    v.initial_cheese = ptr("initial_cheese", np.uint8, C.c_uint8)
    v.cheese_outcomes = ptr("cheese_outcomes", np.uint8, C.c_uint8)
    for k in _U8:
        setattr(v, k, ptr(k, np.uint8, C.c_uint8))
    v.turn = ptr("turn", np.uint16, C.c_uint16)
    for k in _F32:
        setattr(v, k, ptr(k, np.float32, C.c_float))
    return v


def row_shapes(width: int, height: int) -> dict:
    """The shape of one row of each of the eight arrays."""
    return dict(observation=(width * height * 7 + 6,), policy_p1=(5,), policy_p2=(5,), value_p1=(), value_p2=(),
                action_p1=(), action_p2=(), cheese_outcomes=(height, width))


def check_out_tensors(out: dict, n: int, width: int, height: int, device) -> None:
    """``RowSet.build_into``'s conditions on its output tensors (``ValueError``); no device and no library is needed."""
    import torch

    shapes = row_shapes(width, height)
    for k in KEYS:
        if k not in out:
            raise ValueError(f"out has no {k!r}")
        t, want = out[k], (torch.int8 if k in ("action_p1", "action_p2", "cheese_outcomes") else torch.float32)
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{k} is not a torch tensor")
        if t.dtype != want:
            raise ValueError(f"{k} has dtype {t.dtype}, not {want}")
        if not t.is_contiguous():
            raise ValueError(f"{k} is not contiguous")
        row = tuple(t.shape[1:])
        if t.dim() < 1 or not (row == shapes[k] or (shapes[k] == () and row == (1,))):
            raise ValueError(f"{k} has shape {tuple(t.shape)}, not (rows, {', '.join(map(str, shapes[k]))})")
        if t.shape[0] < n:
            raise ValueError(f"{k} has {t.shape[0]} rows, {n} are asked for")
    for k in KEYS:
        t = out[k]
        if t.device != device:
            raise ValueError(f"{k} is on {t.device}, the row set on {device}")


# PyRatMLP's state_dict keys (alpharat/nn/models/mlp.py), in the order of ArMlpTensors (_lib.MLP_TENSORS)
MLP_PARAM_KEYS = ("trunk.0.weight", "trunk.0.bias", "trunk.1.weight", "trunk.1.bias", "trunk.4.weight", "trunk.4.bias",
                  "trunk.5.weight", "trunk.5.bias", "policy_p1_head.weight", "policy_p1_head.bias", "policy_p2_head.weight",
                  "policy_p2_head.bias", "value_head.weight", "value_head.bias")
MLP_RUNNING_KEYS = ("trunk.1.running_mean", "trunk.1.running_var", "trunk.5.running_mean", "trunk.5.running_var")
TRAIN_OUT_KEYS = ("losses", "logits_p1", "logits_p2", "value_p1", "value_p2")


def mlp_param_shapes(width: int, height: int, hidden_dim: int) -> dict:
    """The shape of every tensor of ``MLP_PARAM_KEYS`` and ``MLP_RUNNING_KEYS``."""
    D, H = width * height * 7 + 6, hidden_dim
    shapes = {"trunk.0.weight": (H, D), "trunk.4.weight": (H, H), "policy_p1_head.weight": (5, H), "policy_p1_head.bias": (5,),
              "policy_p2_head.weight": (5, H), "policy_p2_head.bias": (5,), "value_head.weight": (2, H), "value_head.bias": (2,)}
    for k in MLP_PARAM_KEYS + MLP_RUNNING_KEYS:
        shapes.setdefault(k, (H,))
    return shapes


# SymmetricMLP's parameters (alpharat/nn/models/symmetric.py) in torch's named_parameters() order, which is the order of
# ArSymTensors (_lib.SYM_TENSORS); its running statistics in the order of ArSymBnStats
SYM_PARAM_KEYS = ("shared_encoder.0.weight", "shared_encoder.0.bias", "shared_encoder.1.weight", "shared_encoder.1.bias",
                  "player_encoder.0.weight", "player_encoder.0.bias", "player_encoder.1.weight", "player_encoder.1.bias",
                  "trunk.0.weight", "trunk.0.bias", "trunk.1.weight", "trunk.1.bias", "trunk.4.weight", "trunk.4.bias",
                  "trunk.5.weight", "trunk.5.bias", "policy_head.weight", "policy_head.bias", "value_head.weight",
                  "value_head.bias")
SYM_BN_MODULES = ("shared_encoder.1", "player_encoder.1", "trunk.1", "trunk.5")
SYM_RUNNING_KEYS = tuple(f"{bn}.{s}" for bn in SYM_BN_MODULES for s in ("running_mean", "running_var"))


def sym_param_shapes(width: int, height: int, hidden_dim: int) -> dict:
    """The shape of every tensor of ``SYM_PARAM_KEYS`` and ``SYM_RUNNING_KEYS``."""
    hw, H = width * height, hidden_dim
    shapes = {"shared_encoder.0.weight": (H, 5 * hw + 1), "player_encoder.0.weight": (H, hw + 2), "trunk.0.weight": (H, 2 * H),
              "trunk.4.weight": (H, H), "policy_head.weight": (5, 2 * H), "policy_head.bias": (5,), "value_head.weight": (1, 2 * H),
              "value_head.bias": (1,)}
    for k in SYM_PARAM_KEYS + SYM_RUNNING_KEYS:
        shapes.setdefault(k, (H,))
    return shapes


# LocalValueMLP's parameters (alpharat/nn/models/local_value.py) in torch's named_parameters() order, which is the order of
# ArLvTensors (_lib.LV_TENSORS): PyRatMLP's fourteen, then the ownership head's four. Its running statistics are the MLP's.
LV_PARAM_KEYS = MLP_PARAM_KEYS + ("ownership_head.0.weight", "ownership_head.0.bias", "ownership_head.2.weight",
                                  "ownership_head.2.bias")
LV_TRAIN_OUT_KEYS = TRAIN_OUT_KEYS + ("ownership_logits",)


def lv_param_shapes(width: int, height: int, hidden_dim: int) -> dict:
    """The shape of every tensor of ``LV_PARAM_KEYS`` and ``MLP_RUNNING_KEYS``."""
    shapes = mlp_param_shapes(width, height, hidden_dim)
    shapes.update({"ownership_head.0.weight": (hidden_dim, hidden_dim), "ownership_head.0.bias": (hidden_dim,),
                   "ownership_head.2.weight": (4 * width * height, hidden_dim), "ownership_head.2.bias": (4 * width * height,)})
    return shapes


# PyRatCNN's parameters (alpharat/nn/models/cnn/model.py with ResBlocks, MLPPolicyHead and PointValueHead) in torch's
# named_parameters() order, which is the order of ArCnnTensors (_lib.CNN_TENSORS, whose eight block slots a model of fewer
# blocks fills from the front); its running statistics in the order of ArCnnBnStats. Both depend on the number of blocks.
def cnn_param_keys(n_blocks: int) -> tuple:
    blocks = tuple(f"blocks.{b}.{k}" for b in range(int(n_blocks))
                   for k in ("bn1.weight", "bn1.bias", "conv1.weight", "bn2.weight", "bn2.bias", "conv2.weight"))
    return (("stem.weight", "stem_bn.weight", "stem_bn.bias") + blocks
            + ("player_encoder.0.weight", "player_encoder.0.bias", "combiner.0.weight", "combiner.0.bias",
               "policy_head.linear.weight", "policy_head.linear.bias", "value_head.linear.weight", "value_head.linear.bias"))


def cnn_bn_modules(n_blocks: int) -> tuple:
    return ("stem_bn",) + tuple(f"blocks.{b}.{bn}" for b in range(int(n_blocks)) for bn in ("bn1", "bn2"))


def cnn_running_keys(n_blocks: int) -> tuple:
    return tuple(f"{bn}.{s}" for bn in cnn_bn_modules(n_blocks) for s in ("running_mean", "running_var"))


def cnn_param_shapes(width: int, height: int, dims) -> dict:
    """The shape of every tensor of ``cnn_param_keys`` and ``cnn_running_keys``; ``dims`` is ``(channels, player_dim,
    hidden_dim, n_blocks)``."""
    Ch, PD, HD, B = (int(v) for v in dims)
    shapes = {"stem.weight": (Ch, 5, 3, 3), "player_encoder.0.weight": (PD, 3), "player_encoder.0.bias": (PD,),
              "combiner.0.weight": (HD, Ch + PD), "combiner.0.bias": (HD,), "policy_head.linear.weight": (5, 2 * HD),
              "policy_head.linear.bias": (5,), "value_head.linear.weight": (1, 2 * HD), "value_head.linear.bias": (1,)}
    for b in range(B):
        shapes[f"blocks.{b}.conv1.weight"] = shapes[f"blocks.{b}.conv2.weight"] = (Ch, Ch, 3, 3)
    for k in cnn_param_keys(B) + cnn_running_keys(B):
        shapes.setdefault(k, (Ch,))
    return shapes


# PyRatCNN with GPoolResBlocks among its blocks (ar_rows_grad_cnn_gpool). ``blocks`` is a tuple of gpool_channels, one per
# block, 0 for a ResBlock: a gpool block has five parameters and one BatchNorm module more, behind the ResBlock's own, in
# torch's named_parameters() order.
_CNN_BLOCK_KEYS = ("bn1.weight", "bn1.bias", "conv1.weight", "bn2.weight", "bn2.bias", "conv2.weight")
CNN_POOL_KEYS = ("pool_bn.weight", "pool_bn.bias", "pool_conv.weight", "pool_linear.weight", "pool_linear.bias")


def _gpool_blocks(blocks) -> tuple:
    blocks = tuple(int(g) for g in blocks)
    if len(blocks) > _lib.CNN_MAX_BLOCKS or any(g < 0 for g in blocks):
        raise ValueError(f"blocks must be at most {_lib.CNN_MAX_BLOCKS} gpool_channels, 0 for a ResBlock (got {blocks})")
    return blocks


def cnn_gpool_param_keys(blocks) -> tuple:
    blocks = _gpool_blocks(blocks)
    plain = cnn_param_keys(0)
    return (plain[:3] + tuple(f"blocks.{b}.{k}" for b, g in enumerate(blocks) for k in _CNN_BLOCK_KEYS + (CNN_POOL_KEYS if g else ()))
            + plain[3:])


def cnn_gpool_bn_modules(blocks) -> tuple:
    return ("stem_bn",) + tuple(f"blocks.{b}.{bn}" for b, g in enumerate(_gpool_blocks(blocks))
                                for bn in ("bn1", "bn2") + (("pool_bn",) if g else ()))


def cnn_gpool_running_keys(blocks) -> tuple:
    return tuple(f"{bn}.{s}" for bn in cnn_gpool_bn_modules(blocks) for s in ("running_mean", "running_var"))


def cnn_gpool_param_shapes(width: int, height: int, dims) -> dict:
    """The shape of every tensor of ``cnn_gpool_param_keys`` and ``cnn_gpool_running_keys``; ``dims`` is ``(channels,
    player_dim, hidden_dim, blocks)``."""
    Ch, PD, HD = (int(v) for v in dims[:3])
    blocks = _gpool_blocks(dims[3])
    shapes = cnn_param_shapes(width, height, (Ch, PD, HD, len(blocks)))
    for b, g in enumerate(blocks):
        if g:
            shapes[f"blocks.{b}.pool_conv.weight"] = (g, Ch, 1, 1)
            shapes[f"blocks.{b}.pool_linear.weight"] = (Ch, 2 * g)
    for k in cnn_gpool_param_keys(blocks) + cnn_gpool_running_keys(blocks):
        shapes.setdefault(k, (Ch,))
    return shapes


def _cnn_slots(keys: tuple, n_blocks: int, head: int, per_block: int) -> list:
    """where the tensors of a model of ``n_blocks`` blocks go among the pointers of a struct with eight block slots"""
    used = head + per_block * n_blocks
    return list(range(used)) + [head + per_block * _lib.CNN_MAX_BLOCKS + i for i in range(len(keys) - used)]


# What a training step is made of, per architecture: the key tuples and shapes that check_grad_tensors holds the caller's
# tensors to, the two ctypes structs and the symbol that RowSet._grad_into hands them to, and its outputs: their struct,
# their keys and the number of losses. With a dropout the symbol is this one with "_dropout" behind it.
_GRAD_STEPS = {
    "mlp": (MLP_PARAM_KEYS, MLP_RUNNING_KEYS, mlp_param_shapes, _lib.ArMlpTensors, _lib.ArMlpBnStats, "ar_rows_grad_mlp",
            _lib.ArTrainOut, TRAIN_OUT_KEYS, 6),
    "symmetric": (SYM_PARAM_KEYS, SYM_RUNNING_KEYS, sym_param_shapes, _lib.ArSymTensors, _lib.ArSymBnStats,
                  "ar_rows_grad_symmetric", _lib.ArTrainOut, TRAIN_OUT_KEYS, 6),
    "local_value": (LV_PARAM_KEYS, MLP_RUNNING_KEYS, lv_param_shapes, _lib.ArLvTensors, _lib.ArMlpBnStats,
                    "ar_rows_grad_local_value", _lib.ArLvTrainOut, LV_TRAIN_OUT_KEYS, 7),
    # PyRatCNN: where the others have hidden_dim, (channels, player_dim, hidden_dim, n_blocks); its keys depend on n_blocks
    "pyrat_cnn": (cnn_param_keys, cnn_running_keys, cnn_param_shapes, _lib.ArCnnTensors, _lib.ArCnnBnStats, "ar_rows_grad_cnn",
                  _lib.ArTrainOut, TRAIN_OUT_KEYS, 6),
    # ... with gpool blocks: (channels, player_dim, hidden_dim, blocks), the keys depend on the tuple ``blocks``; its pool
    # tensors travel in structs of their own (RowSet.grad_cnn_gpool_into)
    "pyrat_cnn_gpool": (cnn_gpool_param_keys, cnn_gpool_running_keys, cnn_gpool_param_shapes, _lib.ArCnnTensors, _lib.ArCnnBnStats,
                        "ar_rows_grad_cnn_gpool", _lib.ArTrainOut, TRAIN_OUT_KEYS, 6),
}


def _grad_keys(architecture: str, widths) -> tuple:
    """(param_keys, running_keys) of a step; PyRatCNN's depend on the number of blocks (with gpool blocks: on the tuple of
    their widths), the last of its widths"""
    param_keys, running_keys = _GRAD_STEPS[architecture][:2]
    if callable(param_keys):
        return param_keys(widths[3]), running_keys(widths[3])
    return param_keys, running_keys


# What RowSet._grad_into leaves to the architecture: check_widths(widths) -> (the widths checked, as the shape function takes
# them; the entry point's argument for them), and fill_structs(architecture, widths, params, grads, running) -> the two tensor
# structs and the running statistics' (None without them). The three MLP steps share the first pair.
def _mlp_widths(hidden_dim) -> tuple:
    hidden_dim = int(hidden_dim)
    if hidden_dim <= 0:
        raise ValueError("hidden_dim must be positive")
    return hidden_dim, hidden_dim


def _flat_structs(architecture: str, widths, params: dict, grads: dict, running) -> tuple:
    Tensors, BnStats = _GRAD_STEPS[architecture][3:5]
    param_keys, running_keys = _grad_keys(architecture, widths)
    return (Tensors(*[params[k].data_ptr() for k in param_keys]), Tensors(*[grads[k].data_ptr() for k in param_keys]),
            BnStats(*[running[k].data_ptr() for k in running_keys]) if running is not None else None)


def _cnn_widths(dims) -> tuple:
    dims = tuple(int(v) for v in dims)
    if len(dims) != 4 or min(dims[:3]) <= 0 or not 0 <= dims[3] <= _lib.CNN_MAX_BLOCKS:
        raise ValueError("dims must be (channels, player_dim, hidden_dim, n_blocks), the first three positive, at most "
                         f"{_lib.CNN_MAX_BLOCKS} blocks (got {dims})")
    return dims, C.byref(_lib.ArCnnDims(*dims))


def _cnn_structs(architecture: str, dims, params: dict, grads: dict, running) -> tuple:
    """the tensors of dims[3] blocks at the front of the structs' eight block slots"""
    B = dims[3]
    param_keys, running_keys = _grad_keys(architecture, dims)
    p, g, r = _lib.ArCnnTensors(), _lib.ArCnnTensors(), _lib.ArCnnBnStats() if running is not None else None
    for slot, k in zip(_cnn_slots(param_keys, B, 3, 6), param_keys):
        setattr(p, _lib.CNN_TENSORS[slot], params[k].data_ptr())
        setattr(g, _lib.CNN_TENSORS[slot], grads[k].data_ptr())
    if r is not None:
        for slot, k in zip(_cnn_slots(running_keys, B, 2, 4), running_keys):
            setattr(r, _lib.CNN_STATS[slot], running[k].data_ptr())
    return p, g, r


def _cnn_gpool_structs(dims, blocks, params: dict, grads: dict, running) -> tuple:
    """(params, grads, pool params, pool grads, running, pool running) of ar_rows_grad_cnn_gpool: the ResBlock tensors where
    ``_cnn_structs`` puts them, a gpool block's five further tensors and two statistics in block b's slots of the pool structs"""
    B = dims[3]
    plain = {k: i for i, k in enumerate(cnn_param_keys(B))}
    plain_run = {k: i for i, k in enumerate(cnn_running_keys(B))}
    slots, run_slots = _cnn_slots(tuple(plain), B, 3, 6), _cnn_slots(tuple(plain_run), B, 2, 4)
    p, g, pp, pg = _lib.ArCnnTensors(), _lib.ArCnnTensors(), _lib.ArCnnPoolTensors(), _lib.ArCnnPoolTensors()
    for k in cnn_gpool_param_keys(blocks):
        if k in plain:
            field, a, b = _lib.CNN_TENSORS[slots[plain[k]]], p, g
        else:  # blocks.<b>.pool_*
            _, blk, mod, leaf = k.split(".")
            field, a, b = f"b{blk}_{mod}_{'w' if leaf == 'weight' else 'b'}", pp, pg
        setattr(a, field, params[k].data_ptr())
        setattr(b, field, grads[k].data_ptr())
    r = pr = None
    if running is not None:
        r, pr = _lib.ArCnnBnStats(), _lib.ArCnnPoolStats()
        for k in cnn_gpool_running_keys(blocks):
            if k in plain_run:
                setattr(r, _lib.CNN_STATS[run_slots[plain_run[k]]], running[k].data_ptr())
            else:
                _, blk, _, leaf = k.split(".")
                setattr(pr, f"b{blk}_pool_bn_{'mean' if leaf == 'running_mean' else 'var'}", running[k].data_ptr())
    return p, g, pp, pg, r, pr


_GRAD_HOOKS = {"pyrat_cnn": (_cnn_widths, _cnn_structs)}


def check_grad_tensors(params: dict, grads: dict, running, out, n: int, width: int, height: int, hidden_dim: int, device,
                       architecture: str = "mlp") -> None:
    """``RowSet.grad_mlp_into``'s conditions on its tensors (``ValueError``), in the manner of ``check_out_tensors``; no
    device and no library is needed. ``architecture="symmetric"``: ``RowSet.grad_symmetric_into``'s, over
    ``SYM_PARAM_KEYS`` and ``SYM_RUNNING_KEYS``. ``architecture="local_value"``: ``RowSet.grad_local_value_into``'s, over
    ``LV_PARAM_KEYS`` and ``MLP_RUNNING_KEYS``, with seven losses and ``ownership_logits`` ``(n, height, width, 4)``."""
    import torch

    if architecture not in _GRAD_STEPS:
        raise ValueError(f"no training step for architecture {architecture!r}")
    shapes_of = _GRAD_STEPS[architecture][2]
    out_keys, n_losses = _GRAD_STEPS[architecture][7:9]
    param_keys, running_keys = _grad_keys(architecture, hidden_dim)  # ("pyrat_cnn": hidden_dim is its four widths)
    shapes = shapes_of(width, height, hidden_dim)
    out_shapes = dict(losses=(n_losses,), logits_p1=(n, 5), logits_p2=(n, 5), value_p1=(n,), value_p2=(n,),
                      ownership_logits=(n, height, width, 4))
    groups = [("params", params, param_keys, shapes, True), ("grads", grads, param_keys, shapes, True)]
    if running is not None:
        groups.append(("running", running, running_keys, shapes, True))
    if out is not None:
        groups.append(("out", out, out_keys, out_shapes, False))
    for what, d, keys, want, required in groups:
        for k in keys:
            t = d.get(k)
            if t is None:
                if required:
                    raise ValueError(f"{what} has no {k!r}")
                continue
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{what}[{k!r}] is not a torch tensor")
            if t.dtype != torch.float32:
                raise ValueError(f"{what}[{k!r}] has dtype {t.dtype}, not torch.float32")
            if not t.is_contiguous():
                raise ValueError(f"{what}[{k!r}] is not contiguous")
            if tuple(t.shape) != tuple(want[k]):
                raise ValueError(f"{what}[{k!r}] has shape {tuple(t.shape)}, not {tuple(want[k])}")
            if t.device != device:
                raise ValueError(f"{what}[{k!r}] is on {t.device}, the row set on {device}")


class RowSet:
    """ctypes mirror of ``ArRowSet`` (include/alpharat_hip.h): finished games kept on the device until their training rows
    are built. ``capacity_positions`` is fixed here and allocated once; an append that does not fit raises ``MemoryError``
    and changes nothing. For a session, size it ``num_games * max_turns``: an upper bound, so an attached run never fills it.
    """

    def __init__(self, width: int, height: int, capacity_positions: int, device_index: int = 0) -> None:
        self.width, self.height, self.device_index = int(width), int(height), int(device_index)
        self._h = C.c_void_p()
        self._session = None
        self._order_token = None  # set by the RowDataset whose epoch the order belongs to
        _lib.check(_lib.load().ar_rows_open(self.width, self.height, int(capacity_positions), int(device_index),
                                            C.byref(self._h)))

    def _handle(self):
        if not self._h:
            raise RuntimeError("row set is closed")
        return self._h

    def add_games(self, games: Sequence[dict]) -> None:
        """Host records (sink dicts, or ``read_bundle`` games) to the tail of the set, in the order given."""
        if not games:
            return
        keep: list = []
        views = (_lib.ArGameRecordView * len(games))(*[_view_of(g, keep) for g in games])
        _lib.check(_lib.load().ar_rows_add_games(self._handle(), views, len(games)))

    def count(self) -> tuple[int, int]:
        g, p = C.c_uint32(0), C.c_uint64(0)
        _lib.check(_lib.load().ar_rows_count(self._handle(), C.byref(g), C.byref(p)))
        return int(g.value), int(p.value)

    def games(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(game_index, first_row, n_rows) of every stored game, in append order."""
        n = self.count()[0]
        gi, fr, nr = np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        _lib.check(_lib.load().ar_rows_games(self._handle(), gi.ctypes.data, fr.ctypes.data, nr.ctypes.data))
        return gi, fr, nr

    def build(self, rows) -> dict:
        """Output row i from stored position ``rows[i]``: the eight arrays of a shard, ``len(rows)`` rows each."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        n, w, h = len(rows), self.width, self.height
        out = dict(observation=np.empty((n, w * h * 7 + 6), np.float32), policy_p1=np.empty((n, 5), np.float32),
                   policy_p2=np.empty((n, 5), np.float32), value_p1=np.empty(n, np.float32), value_p2=np.empty(n, np.float32),
                   action_p1=np.empty(n, np.int8), action_p2=np.empty(n, np.int8), cheese_outcomes=np.empty((n, h, w), np.int8))
        ptrs = _lib.ArTrainRows(*[out[k].ctypes.data for k in KEYS])
        _lib.check(_lib.load().ar_rows_build(self._handle(), rows.ctypes.data, n, C.byref(ptrs)))
        return out

    def build_kernel_ms(self) -> float:
        """Time inside the kernels of the last ``build`` (HIP events)."""
        ms = C.c_double(0.0)
        _lib.check(_lib.load().ar_rows_build_time(self._handle(), C.byref(ms)))
        return float(ms.value)

    def set_order(self, rows, swap=None) -> None:
        """The order ``build_into`` takes its windows from, kept on the device and replaced as a whole: row i is stored
        position ``rows[i]``, seen by P2 where ``swap[i]`` is set (``None``: nowhere). A position beyond the set raises
        ``ValueError`` and the old order stays. Waits for the batches still being written from the old order."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        if rows.ndim != 1:
            raise ValueError("rows must be one-dimensional")
        if swap is not None:
            swap = np.ascontiguousarray(swap, dtype=np.uint8)
            if swap.shape != rows.shape:
                raise ValueError(f"swap has shape {swap.shape}, rows {rows.shape}")
        self._order_token = None
        _lib.check(_lib.load().ar_rows_order_set(self._handle(), rows.ctypes.data, swap.ctypes.data if swap is not None else None,
                                                 len(rows)))

    def build_into(self, first: int, n: int, out: dict, stream=None) -> None:
        """Rows ``first .. first + n`` of the order into the caller's torch tensors ``out`` (the eight ``KEYS``), on
        ``stream`` (``None``: ``torch.cuda.current_stream()`` of the set's device). Only launches: the tensors are ready
        behind that stream, as after any torch operation on it. Every tensor is on the set's device, contiguous, float32
        (int8 for the actions and cheese outcomes) and has at least ``n`` rows of its row shape (values and actions ``()``
        or ``(1,)``, cheese outcomes ``(h, w)``), else ``ValueError`` before the library is touched."""
        import torch

        first, n = int(first), int(n)
        if first < 0 or n < 0:
            raise ValueError("first and n must not be negative")
        check_out_tensors(out, n, self.width, self.height, torch.device("cuda", self.device_index))
        handle = self._handle()
        if stream is None:
            stream = torch.cuda.current_stream(self.device_index)
        ptrs = _lib.ArTrainRows(*[out[k].data_ptr() for k in KEYS])
        _lib.check(_lib.load().ar_rows_build_device(handle, first, n, C.byref(ptrs), C.c_void_p(stream.cuda_stream)))

    def grad_mlp_into(self, first: int, n: int, hidden_dim: int, params: dict, grads: dict, running, policy_weight: float,
                      value_weight: float, out, stream=None, dropout=None) -> None:
        """The loss and the gradients of PyRatMLP in training mode over rows ``first .. first + n`` of the order
        (``ar_rows_grad_mlp``), on ``stream`` (``None``: torch's current stream of the set's device). Only launches.
        ``params`` and ``grads``: the fourteen tensors under ``MLP_PARAM_KEYS``; ``grads`` is overwritten. ``running``:
        the four ``MLP_RUNNING_KEYS``, updated in place, or ``None``. ``out``: any of ``TRAIN_OUT_KEYS`` (losses ``(6,)``,
        logits ``(n, 5)``, values ``(n,)``), or ``None``. Every tensor is on the set's device, float32, contiguous and of
        the shape ``(width, height, hidden_dim)`` give, else ``ValueError`` before the library is touched. ``dropout``:
        ``None``, or ``(p, seed, step)`` for inverted dropout at rate ``p`` behind both BatchNorm -> ReLU of the trunk
        (``ar_rows_grad_mlp_dropout``): the mask is the library's own counter-based generator, a pure function of
        ``(seed, step)``, the BatchNorm call and the element, so the same triple gives the same bytes; ``p`` outside
        ``[0, 1)`` raises ``ValueError`` with nothing written, and ``p == 0`` is the call without it."""
        self._grad_into("mlp", first, n, hidden_dim, params, grads, running, policy_weight, value_weight, out, stream,
                        dropout=dropout)

    def grad_symmetric_into(self, first: int, n: int, hidden_dim: int, params: dict, grads: dict, running, policy_weight: float,
                            value_weight: float, out, stream=None, dropout=None) -> None:
        """``grad_mlp_into`` for SymmetricMLP (``ar_rows_grad_symmetric``): ``params`` and ``grads`` are the twenty tensors
        under ``SYM_PARAM_KEYS``, ``running`` the eight ``SYM_RUNNING_KEYS`` or ``None``, of the shapes
        ``sym_param_shapes(width, height, hidden_dim)`` gives; everything else as there (``dropout`` is applied behind all
        seven BatchNorm calls, each with its own mask)."""
        self._grad_into("symmetric", first, n, hidden_dim, params, grads, running, policy_weight, value_weight, out, stream,
                        dropout=dropout)

    def grad_local_value_into(self, first: int, n: int, hidden_dim: int, params: dict, grads: dict, running,
                              policy_weight: float, value_weight: float, ownership_weight: float, out, stream=None,
                              dropout=None) -> None:
        """``grad_mlp_into`` for LocalValueMLP (``ar_rows_grad_local_value``): ``params`` and ``grads`` are the eighteen
        tensors under ``LV_PARAM_KEYS``, ``running`` the four ``MLP_RUNNING_KEYS`` or ``None``, of the shapes
        ``lv_param_shapes(width, height, hidden_dim)`` gives. The loss has the third term, ``ownership_weight`` times the
        cross-entropy of the ownership head over the window's active cells. ``out``: any of ``LV_TRAIN_OUT_KEYS`` --
        ``losses`` is ``(7,)``, the six and ``loss_ownership``; ``ownership_logits`` ``(n, height, width, 4)``. The
        workspace is the MLP step's plus ``3 n H + 4 n h w`` floats (the logits alone are 268 MB at 65536 rows of 16x16).
        Everything else as there (the ownership head reads the trunk output behind the second ``dropout``)."""
        self._grad_into("local_value", first, n, hidden_dim, params, grads, running, policy_weight, value_weight, out, stream,
                        (float(ownership_weight),), dropout=dropout)

    def grad_cnn_into(self, first: int, n: int, dims, params: dict, grads: dict, running, policy_weight: float,
                      value_weight: float, out, stream=None) -> None:
        """``grad_mlp_into`` for PyRatCNN (``ar_rows_grad_cnn``): ``dims`` is ``(channels, player_dim, hidden_dim,
        n_blocks)``; ``params`` and ``grads`` are the ``11 + 6 * n_blocks`` tensors under ``cnn_param_keys(n_blocks)``,
        ``running`` the ``2 + 4 * n_blocks`` of ``cnn_running_keys(n_blocks)`` or ``None``, of the shapes
        ``cnn_param_shapes(width, height, dims)`` gives. ``channels`` and ``hidden_dim`` are multiples of 32 up to 256,
        ``player_dim`` is 1 .. 256, at most 8 blocks, a board of 2 to 256 cells and ``n * width * height <= 2**22``.
        There is no dropout. The workspace holds ``4 * n_blocks + 5`` arrays of ``n * width * height * channels`` floats."""
        self._grad_into("pyrat_cnn", first, n, dims, params, grads, running, policy_weight, value_weight, out, stream)

    def grad_cnn_gpool_into(self, first: int, n: int, dims, blocks, params: dict, grads: dict, running, policy_weight: float,
                            value_weight: float, out, stream=None, dropout=None) -> None:
        """``grad_cnn_into`` for a PyRatCNN whose trunk mixes ``ResBlock`` and ``GPoolResBlock`` (``ar_rows_grad_cnn_gpool``).
        ``dims`` is ``(channels, player_dim, hidden_dim, n_blocks)`` and ``blocks`` the ``n_blocks`` ``gpool_channels``, 0 for
        a ``ResBlock`` and 1 .. 256 for a ``GPoolResBlock``; ``params`` and ``grads`` are the tensors under
        ``cnn_gpool_param_keys(blocks)`` (11 a gpool block, 6 a res block), ``running`` those of
        ``cnn_gpool_running_keys(blocks)`` or ``None``, of the shapes ``cnn_gpool_param_shapes`` gives. ``dropout``: ``None``
        or ``(p, seed, step)``, applied behind the ReLU of ``player_encoder`` (calls 0, 1: P1's, P2's rows) and of ``combiner``
        (calls 2, 3) from the library's own mask generator, as ``grad_mlp_into`` describes. Per gpool block the workspace
        grows by ``n * width * height * (channels + gpool_channels)`` floats. Everything else, the checks included, as
        ``grad_cnn_into``."""
        import torch

        first, n = int(first), int(n)
        if first < 0 or n < 0:
            raise ValueError("first and n must not be negative")
        dims, dims_arg = _cnn_widths(dims)
        blocks = _gpool_blocks(blocks)
        if len(blocks) != dims[3]:
            raise ValueError(f"blocks has {len(blocks)} entries, dims names {dims[3]} blocks")
        if max(blocks, default=0) > 256:
            raise ValueError(f"gpool_channels must be at most 256 (got {blocks})")
        check_grad_tensors(params, grads, running, out, n, self.width, self.height, dims[:3] + (blocks,),
                           torch.device("cuda", self.device_index), architecture="pyrat_cnn_gpool")
        handle = self._handle()
        if stream is None:
            stream = torch.cuda.current_stream(self.device_index)
        p, g, pp, pg, r, pr = _cnn_gpool_structs(dims, blocks, params, grads, running)
        o = _lib.ArTrainOut(*[out[k].data_ptr() if out.get(k) is not None else None for k in TRAIN_OUT_KEYS]) if out is not None else None
        d = None
        if dropout is not None:
            rate, seed, step = dropout
            d = _lib.ArTrainDropout(float(rate), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF)
        pool_dims = _lib.ArCnnPoolDims((C.c_uint32 * _lib.CNN_MAX_BLOCKS)(*blocks))
        _lib.check(_lib.load().ar_rows_grad_cnn_gpool(
            handle, first, n, dims_arg, C.byref(pool_dims), C.byref(p), C.byref(pp), C.byref(g), C.byref(pg),
            C.byref(r) if r is not None else None, C.byref(pr) if pr is not None else None, float(policy_weight),
            float(value_weight), C.byref(o) if o is not None else None, C.byref(d) if d is not None else None,
            C.c_void_p(stream.cuda_stream)))

    def _grad_into(self, architecture: str, first, n, hidden_dim, params, grads, running, policy_weight, value_weight, out,
                   stream, more_weights: tuple = (), dropout=None) -> None:
        import torch

        first, n = int(first), int(n)
        if first < 0 or n < 0:
            raise ValueError("first and n must not be negative")
        # the two things that differ by architecture: what the widths are and how the tensors fill the structs
        check_widths, fill_structs = _GRAD_HOOKS.get(architecture, (_mlp_widths, _flat_structs))
        widths, widths_arg = check_widths(hidden_dim)
        check_grad_tensors(params, grads, running, out, n, self.width, self.height, widths,
                           torch.device("cuda", self.device_index), architecture=architecture)
        symbol, Out, out_keys = _GRAD_STEPS[architecture][5:8]
        handle = self._handle()
        if stream is None:
            stream = torch.cuda.current_stream(self.device_index)
        p, g, r = fill_structs(architecture, widths, params, grads, running)
        o = Out(*[out[k].data_ptr() if out.get(k) is not None else None for k in out_keys]) if out is not None else None
        more = ()
        if dropout is not None:
            rate, seed, step = dropout
            d = _lib.ArTrainDropout(float(rate), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF)
            symbol, more = symbol + "_dropout", (C.byref(d),)
        _lib.check(getattr(_lib.load(), symbol)(handle, first, n, widths_arg, C.byref(p), C.byref(g),
                                                C.byref(r) if r is not None else None, float(policy_weight),
                                                float(value_weight), *more_weights, C.byref(o) if o is not None else None,
                                                *more, C.c_void_p(stream.cuda_stream)))

    def validate(self, net, rows, chunk_rows: int = 0, return_rows: bool = False):
        """``net`` over the stored positions ``rows``: the sums of the reference's validation pass
        (``alpharat_amd.validate.validate``)."""
        from .validate import validate

        return validate(self, net, rows, chunk_rows, return_rows)

    def validate_lv(self, net, rows, chunk_rows: int = 0, loss_batch_rows: int = 0, return_rows: bool = False):
        """``validate`` for a ``local_value`` net with its ownership head: ``(ValSums, OwnSums[, outputs])``
        (``alpharat_amd.validate.validate_lv``)."""
        from .validate import validate_lv

        return validate_lv(self, net, rows, chunk_rows, loss_batch_rows, return_rows)

    def clear(self) -> None:
        """Forgets the games, and the order with them."""
        _lib.check(_lib.load().ar_rows_clear(self._handle()))

    def close(self) -> None:
        if not self._h:
            return
        s = self._session() if self._session is not None else None
        if s is not None and s._h:
            raise RuntimeError("close the session this row set is attached to first")
        h, self._h = self._h, C.c_void_p()
        _lib.load().ar_rows_close(h)

    def __enter__(self) -> "RowSet":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def _attach(rowset: RowSet, session) -> None:
    """``SelfPlaySession.attach_rows``: every game the session drains is appended to ``rowset`` on the device."""
    _lib.check(_lib.load().ar_rows_attach(rowset._handle(), session._h))
    rowset._session = weakref.ref(session)


@dataclass(frozen=True)
class ShardingResult:  # sharding.py:63-70
    shard_id: str
    shard_dir: str
    total_positions: int
    train_positions: int
    val_positions: int


RowBuilder = Callable[[np.ndarray], dict]


def _listing(games_or_bundle_dirs, rowset, row_builder):
    """(lengths per game in listing order, row builder over positions numbered through that listing, width, height,
    source batches, a row set to close afterwards or None)."""
    src = list(games_or_bundle_dirs) if games_or_bundle_dirs is not None else []
    own = None
    batches: list[str] = []
    if src:
        if not isinstance(src[0], dict):
            batches = [f"{Path(d).parent.name}/{Path(d).name}" for d in src]  # experiments/paths.py:134-143
            src = read_bundle_dirs(src)
            if not src:
                raise ValueError("No games found in batch directories")  # sharding.py:438-439
        lengths = np.array([len(np.asarray(g["turn"])) for g in src], np.int64)
        w, h = int(src[0]["width"]), int(src[0]["height"])
        for g in src:
            if (int(g["width"]), int(g["height"])) != (w, h):  # sharding.py:560-564
                raise ValueError(f"Dimension mismatch: expected ({w}, {h}), got ({g['width']}, {g['height']})")
        if row_builder is not None:
            return lengths, row_builder, w, h, batches, None
        if rowset is None:
            rowset = own = RowSet(w, h, max(int(lengths.sum()), 1))
        try:
            first = rowset.count()[1]
            rowset.add_games(src)
        except BaseException:
            if own is not None:
                own.close()
            raise
        stored = first + np.arange(int(lengths.sum()), dtype=np.uint64)  # appended in the order given, games of no position skipped
    elif rowset is not None:
        gi, fr, nr = rowset.games()
        order = np.argsort(gi, kind="stable")  # an attached run appends games as they finish: list them by game index
        lengths = nr[order].astype(np.int64)
        w, h = rowset.width, rowset.height
        stored = (np.concatenate([fr[g] + np.arange(nr[g], dtype=np.uint64) for g in order]) if len(order)
                  else np.zeros(0, np.uint64))
        if row_builder is not None:
            return lengths, row_builder, w, h, batches, None
    else:
        raise ValueError("batch_dirs cannot be empty")  # sharding.py:121-122, 233-234
    return lengths, (lambda index: rowset.build(stored[np.asarray(index, np.int64)])), w, h, batches, own


def _write_split(out_dir: Path, members, lengths, offsets, row_builder, positions_per_shard, seed, compress, set_id, batches,
                 w, h) -> int:
    """sharding.py:303-385 _process_game_refs_to_shards: the split's positions, shuffled, in chunks of positions_per_shard."""
    pos = (np.concatenate([offsets[g] + np.arange(lengths[g], dtype=np.int64) for g in members]) if len(members)
           else np.zeros(0, np.int64))
    total = len(pos)
    order = pos[np.random.default_rng(seed).permutation(total)]  # :345-346
    save = np.savez_compressed if compress else np.savez
    count = 0
    for start in range(0, total, positions_per_shard):  # :799-819
        rows = row_builder(order[start:start + positions_per_shard])
        save(out_dir / f"shard_{count:04d}.npz", **{k: rows[k] for k in KEYS})
        count += 1
    manifest = dict(training_set_id=set_id, created_at=datetime.now(timezone.utc).isoformat(), builder_version=BUILDER_VERSION,
                    source_batches=batches, total_positions=total, shard_count=count, positions_per_shard=positions_per_shard,
                    width=w, height=h)  # sharding.py:46-60 TrainingSetManifest
    (out_dir / "manifest.json").write_text(json.dumps(manifest, indent=2))
    return total


def prepare_training_set_with_split(games_or_bundle_dirs, output_dir, *, val_ratio: float = 0.1,
                                    positions_per_shard: int = 10000, seed: int | None = None,
                                    rowset: RowSet | None = None, compress: bool = False,
                                    row_builder: RowBuilder | None = None) -> ShardingResult:
    """sharding.py:191-300 with the rows built on the device.

    ``games_or_bundle_dirs``: record dicts (``on_game`` / ``read_bundle``) or batch directories holding bundles, taken in
    the order given and uploaded to ``rowset`` (a set of their size is opened when none is given); or ``None`` with an
    attached ``rowset``, whose games are taken in increasing ``game_index``. Games are permuted with
    ``default_rng(seed).permutation`` and the first ``int(total * val_ratio)`` form ``val/``, the rest ``train/``; the
    positions of a split are permuted with ``default_rng(seed)`` (train) and ``default_rng(seed + 1)`` (val) and built
    ``positions_per_shard`` at a time. Shards are written stored (``np.savez``); ``compress=True`` gives the reference's
    ``savez_compressed`` -- ``np.load`` reads both alike. ``row_builder(index) -> the eight arrays`` replaces the device as
    the source of rows (index numbers the positions through the listed games); it exists so that the file layout can be
    checked without a device.
    """
    if not 0.0 <= val_ratio < 1.0:
        raise ValueError(f"val_ratio must be in [0.0, 1.0), got {val_ratio}")
    if positions_per_shard <= 0:
        raise ValueError("positions_per_shard must be positive")
    lengths, build, w, h, batches, own = _listing(games_or_bundle_dirs, rowset, row_builder)
    try:
        total_games = len(lengths)
        if total_games == 0:
            raise ValueError("No games found in batch directories")
        idx = np.random.default_rng(seed).permutation(total_games)  # :244-246
        n_val = int(total_games * val_ratio)                        # :248
        val, train = idx[:n_val], idx[n_val:]
        # (sharding.py:252-253 raises "No games left for training" here; with val_ratio < 1 and at least one game,
        # int(total * val_ratio) < total, so that cannot happen: the range check above is what refuses such a ratio)
        offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
        set_id = str(uuid.uuid4())
        set_dir = Path(output_dir) / set_id
        set_dir.mkdir(parents=True, exist_ok=False)
        (set_dir / "train").mkdir()
        n_train = _write_split(set_dir / "train", train, lengths, offsets, build, positions_per_shard, seed, compress,
                               f"{set_id}_train", batches, w, h)
        n_valp = 0
        if len(val):  # :278-292
            (set_dir / "val").mkdir()
            n_valp = _write_split(set_dir / "val", val, lengths, offsets, build, positions_per_shard,
                                  seed + 1 if seed is not None else None, compress, f"{set_id}_val", batches, w, h)
        return ShardingResult(set_id, str(set_dir), n_train + n_valp, n_train, n_valp)
    finally:
        if own is not None:
            own.close()


def prepare_training_set(games_or_bundle_dirs, output_dir, *, positions_per_shard: int = 10000, seed: int | None = None,
                         rowset: RowSet | None = None, compress: bool = False,
                         row_builder: RowBuilder | None = None) -> Path:
    """sharding.py:73-188: the same procedure without the split -- every position shuffled with ``default_rng(seed)``,
    shards and manifest directly under ``output_dir/<training_set_id>``. Returns that directory."""
    if positions_per_shard <= 0:
        raise ValueError("positions_per_shard must be positive")
    lengths, build, w, h, batches, own = _listing(games_or_bundle_dirs, rowset, row_builder)
    try:
        if int(lengths.sum()) == 0:
            raise ValueError("No positions found in batch directories")  # :139-140
        offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
        set_id = str(uuid.uuid4())
        set_dir = Path(output_dir) / set_id
        set_dir.mkdir(parents=True, exist_ok=False)
        _write_split(set_dir, np.arange(len(lengths)), lengths, offsets, build, positions_per_shard, seed, compress, set_id,
                     batches, w, h)
        return set_dir
    finally:
        if own is not None:
            own.close()
