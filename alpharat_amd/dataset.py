"""Training batches straight from a device-resident ``RowSet``: the counterpart of the reference's ``GPUDataset``
(alpharat/nn/gpu_dataset.py) with the trainer's player-swap augmentation (alpharat/nn/augmentation.py:86-184) folded in.

The reference loads every shard back into device tensors, gathers eight arrays per batch with a shuffled index, clones the
batch and runs a chain of ``torch.where`` over it. Here the finished games stay in the row set as position records; an
epoch's shuffle and swap mask are uploaded once as the set's order, and every batch is one kernel (``k_rows_batch``) that
writes the rows, already shuffled and swapped, into fresh device tensors on the current stream.

Two differences from the reference, both on purpose:

* The swap mask applies to the *stored* position afresh every epoch. That is what the trainer's per-batch
  ``PlayerSwapStrategy`` does; ``GPUDataset.epoch_iter`` swaps its resident tensors in place, so its swaps accumulate over
  epochs (a row swapped in epochs 0 and 1 is back to the original in epoch 1).
* The random stream is NumPy's, not torch's: ``epoch_plan`` is a pure function of ``(seed, epoch)``, so an epoch can be
  reproduced, and checked without a device.

torch ships its own copy of the HIP runtime and a process brings up only one: import torch before anything
loads ``libalpharat_hip.so``, as a training script does anyway. ``RowDataset`` raises if torch sees no device.
"""
from __future__ import annotations

from typing import Iterator

import numpy as np

from .shards import KEYS, RowSet, row_shapes
from .train import CNNGradStep, GPoolCNNGradStep, LocalValueGradStep, MLPGradStep, SymmetricGradStep  # noqa: F401  (exported beside RowDataset)


def epoch_plan(n: int, seed: int, epoch: int, shuffle: bool = True, augment: bool = True,
               p_swap: float = 0.5) -> tuple[np.ndarray, np.ndarray]:
    """``(order, mask)`` of one epoch over ``n`` positions: epoch row ``j`` is position ``order[j]``, swapped iff
    ``mask[order[j]]``. ``rng = default_rng([seed, epoch])``; the mask ``rng.random(n) < p_swap`` is drawn first (all false
    without ``augment``), the order ``rng.permutation(n)`` second (``arange(n)`` without ``shuffle``)."""
    rng = np.random.default_rng([int(seed), int(epoch)])
    mask = rng.random(n) < p_swap if augment else np.zeros(n, bool)
    order = rng.permutation(n) if shuffle else np.arange(n)
    return order.astype(np.int64), mask


def batch_windows(n: int, batch_size: int, drop_last: bool = True) -> list[tuple[int, int]]:
    """``(first, rows)`` of every batch of an epoch over ``n`` rows; the incomplete last one only without ``drop_last``."""
    if batch_size <= 0:
        raise ValueError("batch_size must be positive")
    stop = n - n % batch_size if drop_last else n
    return [(first, min(batch_size, n - first)) for first in range(0, stop, batch_size)]


def split_games(game_index: np.ndarray, val_ratio: float, seed) -> tuple[np.ndarray, np.ndarray]:
    """``(train, val)`` members of ``prepare_training_set_with_split`` (alpharat/data/sharding.py:243-250) as numbers of
    stored games: the games are listed by ``game_index`` (stable: games without one keep their order), permuted with
    ``default_rng(seed).permutation``, and the first ``int(total * val_ratio)`` go to val."""
    if not 0.0 <= val_ratio < 1.0:
        raise ValueError(f"val_ratio must be in [0.0, 1.0), got {val_ratio}")
    listing = np.argsort(np.asarray(game_index), kind="stable")
    idx = np.random.default_rng(seed).permutation(len(listing))
    n_val = int(len(listing) * val_ratio)
    return listing[idx[n_val:]], listing[idx[:n_val]]


class RowDataset:
    """The positions of a row set -- attached or uploaded -- as training batches on its device.

    ``games``: numbers of stored games (as ``RowSet.games()`` lists them) this dataset is made of, in that order; ``None``:
    every game, listed by ``game_index``. ``split`` gives the train and val datasets over the same set, with the membership
    of the shards ``prepare_training_set_with_split`` writes for the same seed. Datasets over one set share its one order:
    an epoch of one is iterated to its end before an epoch of another begins (a batch asked for after another dataset set
    the order raises ``RuntimeError``). Games appended to the set later are not part of a dataset made before.
    """

    def __init__(self, rowset: RowSet, games=None) -> None:
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("torch sees no HIP device: import torch before alpharat_amd loads its library (INTEGRATION.md)")
        self.rowset = rowset
        gi, fr, nr = rowset.games()
        members = np.argsort(gi, kind="stable") if games is None else np.asarray(games, np.int64)
        self._game_index = gi
        self.games = members
        self._positions = (np.concatenate([fr[g] + np.arange(nr[g], dtype=np.uint64) for g in members]) if len(members)
                           else np.zeros(0, np.uint64))

    def __len__(self) -> int:
        return len(self._positions)

    @property
    def width(self) -> int:
        return self.rowset.width

    @property
    def height(self) -> int:
        return self.rowset.height

    @property
    def positions(self) -> np.ndarray:
        """The stored position of every row of this dataset, before any shuffle."""
        return self._positions

    def split(self, val_ratio: float, seed) -> tuple["RowDataset", "RowDataset"]:
        gi = self._game_index[self.games]
        train, val = split_games(gi, val_ratio, seed)
        return RowDataset(self.rowset, self.games[train]), RowDataset(self.rowset, self.games[val])

    def validate(self, net, chunk_rows: int = 0, return_rows: bool = False):
        """``net`` over this dataset's ``positions``: ``val.validate(net).metrics()`` is the reference's validation pass
        over the val half of a split (``alpharat_amd.validate``). Needs no order and disturbs none."""
        return self.rowset.validate(net, self._positions, chunk_rows, return_rows)

    def validate_lv(self, net, chunk_rows: int = 0, loss_batch_rows: int = 0, return_rows: bool = False):
        """``validate`` for a ``local_value`` net with its ownership head, over this dataset's ``positions`` in their order
        (the batches of ``loss_batch_rows`` are cut from it): ``(ValSums, OwnSums[, outputs])``."""
        return self.rowset.validate_lv(net, self._positions, chunk_rows, loss_batch_rows, return_rows)

    def epoch_iter(self, batch_size: int, *, epoch: int = 0, seed: int = 0, augment: bool = True, p_swap: float = 0.5,
                   shuffle: bool = True, drop_last: bool = True) -> Iterator[dict]:
        """One epoch as dicts of device tensors in ``GPUDataset``'s shapes: observation ``(N, h*w*7+6)`` and policies
        ``(N, 5)`` float32, ``value_*`` ``(N, 1)`` float32, ``action_*`` ``(N, 1)`` int8, ``cheese_outcomes`` ``(N, h, w)``
        int8. The plan is ``epoch_plan(len(self), seed, epoch, shuffle, augment, p_swap)``; the order is set once, every
        batch is one ``build_into`` into fresh tensors on the current stream, and nothing is synchronised."""
        import torch

        windows = batch_windows(len(self), batch_size, drop_last)
        order, mask = epoch_plan(len(self), seed, epoch, shuffle, augment, p_swap)
        rs = self.rowset
        rs.set_order(self._positions[order], mask[order])
        token = rs._order_token = object()
        device = torch.device("cuda", rs.device_index)
        shapes = row_shapes(rs.width, rs.height)
        for first, n in windows:
            if rs._order_token is not token:
                raise RuntimeError("another epoch over this row set began before this one ended")
            out = {k: torch.empty((n,) + (shapes[k] or (1,)), device=device,
                                  dtype=torch.int8 if k in ("action_p1", "action_p2", "cheese_outcomes") else torch.float32)
                   for k in KEYS}
            rs.build_into(first, n, out)
            yield out

    def grad_iter(self, step: "MLPGradStep | SymmetricGradStep | LocalValueGradStep | CNNGradStep", batch_size: int, *, epoch: int = 0,
                  seed: int = 0, augment: bool = True, p_swap: float = 0.5, shuffle: bool = True,
                  drop_last: bool = True) -> Iterator[tuple]:
        """One epoch as training steps: the plan, the order and the order-token rule of ``epoch_iter``, but instead of
        materialising a batch, ``step.step(rowset, first, n)`` leaves the batch's gradients in the model's ``.grad`` and
        ``(n, losses)`` is yielded -- ``losses`` the ``(6,)`` device tensor of ``MLPGradStep.step`` (``(7,)`` from a
        ``LocalValueGradStep``, ``loss_ownership`` last). The trainer's loop body is ``optimizer.step()``. Nothing is synchronised. A trailing batch of one row is skipped even without
        ``drop_last``: a training BatchNorm over one row has no variance, and torch refuses it too.

        ``step`` is an ``MLPGradStep``, a ``SymmetricGradStep``, a ``LocalValueGradStep``, a ``CNNGradStep`` or a ``GPoolCNNGradStep``. The reference trains LocalValueMLP
        with the player swap at ``p_augment`` 0.5, as PyRatMLP: the defaults here. It trains SymmetricMLP with
        ``NoAugmentation`` (alpharat/nn/architectures/symmetric/config.py): ``augment=False`` is its setting. It trains PyRatCNN with
        ``NoAugmentation`` too (alpharat/nn/architectures/cnn/config.py): ``augment=False`` again. Swapped rows stay legal."""
        windows = batch_windows(len(self), batch_size, drop_last)
        order, mask = epoch_plan(len(self), seed, epoch, shuffle, augment, p_swap)
        rs = self.rowset
        rs.set_order(self._positions[order], mask[order])
        token = rs._order_token = object()
        for first, n in windows:
            if n < 2:
                continue
            if rs._order_token is not token:
                raise RuntimeError("another epoch over this row set began before this one ended")
            yield n, step.step(rs, first, n)
