"""The training step of PyRatMLP, SymmetricMLP, LocalValueMLP or PyRatCNN over a device-resident ``RowSet``: forward, losses and
gradients in one call.

The reference's loop (alpharat/nn/training/loop.py) gathers a batch, runs ``model(obs)`` in training mode,
``compute_mlp_losses`` and ``loss.backward()``. ``MLPGradStep.step`` does the three for rows ``first .. first + n`` of the
set's order with ``ar_rows_grad_mlp`` (alpharat_amd/csrc/train_mlp.h): the rows are built from the stored records, and the
gradients land in tensors this object owns, which it hands to the parameters as their ``.grad``. The optimiser, its
schedule and the checkpoints stay the trainer's::

    step = MLPGradStep(model, policy_weight=1.0, value_weight=1.0)
    for n, losses in train_dataset.grad_iter(step, 4096, epoch=epoch, seed=seed):
        optimizer.step()

Supported: PyRatMLP (``architecture: mlp``, ``MLPGradStep``), SymmetricMLP (``architecture: symmetric``,
``SymmetricGradStep`` over ``ar_rows_grad_symmetric``, alpharat_amd/csrc/train_sym.h) and LocalValueMLP (``architecture:
local_value``, ``LocalValueGradStep`` over ``ar_rows_grad_local_value``, alpharat_amd/csrc/train_lv.h: the MLP's step plus
the ownership head and ``ownership_weight`` times its masked cross-entropy, seven losses) -- same loop, same contract -- in
float32 and a hidden width that is a multiple of 32, at most 256. PyRatCNN (``architecture: cnn``, ``CNNGradStep`` over
``ar_rows_grad_cnn``, alpharat_amd/csrc/train_cnn.h) as ``CNNModelConfig`` builds it by default: a stem, up to 8
``ResBlock``s, ``MLPPolicyHead`` and ``PointValueHead``, ``channels`` and ``hidden_dim`` multiples of 32 up to 256,
``player_dim`` up to 256, boards of 2 to 256 cells, ``n * width * height <= 2**22``; the reference trains it with
``augment=False``. ``GPoolCNNGradStep`` (``ar_rows_grad_cnn_gpool``, alpharat_amd/csrc/train_gpool.h) is that step for a trunk of
any mix of ``ResBlock`` and ``GPoolResBlock`` (``gpool_channels`` up to 256) with dropout behind the ReLU of
``player_encoder`` and of ``combiner``: the network configs/train_cnn_7x7.yaml describes. ``CNNGradStep`` keeps refusing
both. AMP, KataGoCNN and PyRatCNN's pooled value head are not built.

Dropout is opt-in: without ``dropout_seed`` a model whose ``nn.Dropout`` has ``p != 0`` is refused, as it always was (the
architectures' default is 0.0; the reference's configs/model/symmetric.yaml sets ``dropout: 0.1``). With
``dropout_seed=<int>`` the rate is read from the model's ``Dropout`` modules -- all of one ``p`` in ``[0, 1)``, else
``ValueError`` -- and every training-mode step applies inverted dropout behind each BatchNorm -> ReLU of the encoders and
the trunk, as the modules would. The mask is the library's own counter-based generator (alpharat_amd/csrc/dev_dropout.h), a
pure function of ``(dropout_seed, dropout_step)``, the BatchNorm call and the element: not torch's Philox stream, so a run
is reproducible from the seed and the step count, never mask-for-mask equal to a torch run. ``dropout_step`` starts at 0 and
grows by one with every training-mode step; it is an attribute, so a resumed run sets it. In eval mode no dropout is applied
and the counter stays. ``dropout_mask`` returns the mask of one BatchNorm call as the device forms it.

``trunk.0.bias`` and ``trunk.4.bias`` -- and SymmetricMLP's ``shared_encoder.0.bias`` and ``player_encoder.0.bias`` -- sit
in front of a BatchNorm, so their true gradient is zero and what any implementation writes there is rounding noise
(INTEGRATION.md).

torch ships its own copy of the HIP runtime and a process brings up only one: import torch before anything loads
``libalpharat_hip.so``.
"""
from __future__ import annotations

from .shards import LV_PARAM_KEYS, MLP_PARAM_KEYS, MLP_RUNNING_KEYS, SYM_BN_MODULES, SYM_PARAM_KEYS, SYM_RUNNING_KEYS, RowSet

_PREFIX = "_orig_mod."  # torch.compile's wrapper, stripped as weights.py does


class _GradStep:
    """What the steps do. A subclass names its architecture (``_NAME``, for the messages), its parameter and
    running-statistic keys, the ``(num_batches_tracked key, BatchNorm calls per step)`` pairs and the ``RowSet`` method
    that launches it; ``_read_dims`` takes the widths from the checked parameters and ``_check_board`` holds them
    against a row set's board. ``_N_LOSSES``, ``_weights`` and ``_more_outputs`` are the MLP's unless a loss has more terms."""

    _NAME = _PARAM_KEYS = _RUNNING_KEYS = _TRACKED = _ROWSET_METHOD = None
    _N_LOSSES = 6

    def __init__(self, model, policy_weight: float = 1.0, value_weight: float = 1.0, dropout_seed: int | None = None) -> None:
        import torch

        self.model = model
        self.policy_weight, self.value_weight = float(policy_weight), float(value_weight)
        rates = sorted({float(m.p) for m in model.modules() if isinstance(m, torch.nn.Dropout)})
        if dropout_seed is None:
            for p in rates:
                if p != 0:
                    raise ValueError(f"dropout {p} is not supported: the step is built for {self._NAME}'s default dropout 0.0 "
                                     "unless it is given a dropout_seed, which the device's own mask generator starts from")
        elif len(rates) > 1:
            raise ValueError(f"the model's Dropout modules have different p ({', '.join(map(str, rates))}): the step applies one")
        elif rates and not 0.0 <= rates[0] < 1.0:
            raise ValueError(f"dropout {rates[0]} is not supported: p must be in [0, 1)")
        self.dropout_seed = None if dropout_seed is None else int(dropout_seed)
        self.dropout_p = rates[0] if dropout_seed is not None and rates else 0.0
        self.dropout_step = 0  # sent with every training-mode step, then one more; a resumed run sets it
        named = {k.removeprefix(_PREFIX): v for k, v in model.named_parameters()}
        buffers = {k.removeprefix(_PREFIX): v for k, v in model.named_buffers()}
        self._refuse(named, buffers)
        tracked = tuple(k for k, _ in self._TRACKED)
        missing = [k for k in self._PARAM_KEYS if k not in named] + [k for k in self._RUNNING_KEYS + tracked if k not in buffers]
        if missing:
            raise ValueError(f"the model is not a {self._NAME}: its state_dict lacks {', '.join(missing)}")
        self.params = {k: named[k] for k in self._PARAM_KEYS}
        self.running = {k: buffers[k] for k in self._RUNNING_KEYS}
        self._tracked = tuple((buffers[k], calls) for k, calls in self._TRACKED)
        for k, t in {**self.params, **self.running}.items():
            if t.dtype != torch.float32:
                raise ValueError(f"{k} has dtype {t.dtype}: the step is float32 throughout")
            if not t.is_contiguous():
                raise ValueError(f"{k} is not contiguous")
        self._read_dims()
        self.grads = {k: torch.zeros_like(p) for k, p in self.params.items()}

    def _refuse(self, named: dict, buffers: dict) -> None:
        pass

    def _weight(self, key: str):
        w = self.params[key]
        if w.dim() != 2:
            raise ValueError(f"{key} has shape {tuple(w.shape)}")
        return w

    def _weights(self) -> tuple:
        return self.policy_weight, self.value_weight

    def _more_outputs(self, rowset: RowSet, n: int, device) -> dict:
        return {}

    def _dims(self):
        """what the ``RowSet`` method takes for the network's widths: ``hidden_dim``, unless there are more"""
        return self.hidden_dim

    def _dims_args(self) -> tuple:
        """the ``RowSet`` method's arguments between ``n`` and ``params``"""
        return (self._dims(),)

    def step(self, rowset: RowSet, first: int, n: int, outputs: bool = False):
        import torch

        self._check_board(rowset)
        device = torch.device("cuda", rowset.device_index)
        n = int(n)
        out = dict(losses=torch.empty(self._N_LOSSES, device=device, dtype=torch.float32))
        if outputs:
            out.update(logits_p1=torch.empty((n, 5), device=device), logits_p2=torch.empty((n, 5), device=device),
                       value_p1=torch.empty(n, device=device), value_p2=torch.empty(n, device=device))
            out.update(self._more_outputs(rowset, n, device))
        training = bool(self.model.training)
        params = {k: p.data for k, p in self.params.items()}
        # nn.Dropout is the identity in eval mode: no mask then, and the counter stays
        dropping = training and self.dropout_seed is not None and self.dropout_p != 0
        more = dict(dropout=(self.dropout_p, self.dropout_seed, self.dropout_step)) if dropping else {}
        getattr(rowset, self._ROWSET_METHOD)(first, n, *self._dims_args(), params, self.grads, self.running if training else None,
                                             *self._weights(), out, **more)
        for k, p in self.params.items():
            p.grad = self.grads[k]
        if training:
            for t, calls in self._tracked:
                t.add_(calls)
            if self.dropout_seed is not None:
                self.dropout_step += 1
        if outputs:
            return tuple(out.values())
        return out["losses"]


class MLPGradStep(_GradStep):
    """``model``: an ``nn.Module`` whose ``state_dict()`` has PyRatMLP's keys (an ``_orig_mod.`` prefix is stripped).
    ``ValueError`` for a ``Dropout`` with ``p != 0`` and no ``dropout_seed`` (with one: for ``Dropout`` modules of different
    ``p``, or ``p >= 1``), an ``ownership_head``, a missing key, or a parameter or BatchNorm
    buffer that is not float32 or not contiguous. One persistent gradient tensor per parameter is allocated here."""

    _NAME, _PARAM_KEYS, _RUNNING_KEYS, _ROWSET_METHOD = "PyRatMLP", MLP_PARAM_KEYS, MLP_RUNNING_KEYS, "grad_mlp_into"
    _TRACKED = (("trunk.1.num_batches_tracked", 1), ("trunk.5.num_batches_tracked", 1))

    def _refuse(self, named: dict, buffers: dict) -> None:
        if any(k.startswith("ownership_head.") for k in list(named) + list(buffers)):
            raise ValueError("the model has an ownership_head (LocalValueMLP): its loss has a third term that this step "
                             "does not compute")

    def _read_dims(self) -> None:
        w0 = self._weight("trunk.0.weight")
        self.hidden_dim, self.obs_dim = int(w0.shape[0]), int(w0.shape[1])

    def _check_board(self, rowset: RowSet) -> None:
        if rowset.width * rowset.height * 7 + 6 != self.obs_dim:
            raise ValueError(f"the model reads {self.obs_dim} inputs, a {rowset.width}x{rowset.height} row has "
                             f"{rowset.width * rowset.height * 7 + 6}")

    def step(self, rowset: RowSet, first: int, n: int, outputs: bool = False):
        """Loss and gradients of rows ``first .. first + n`` of ``rowset``'s order, launched on torch's current stream;
        nothing is synchronised. Every parameter's ``.grad`` is (again) this object's buffer, overwritten -- so
        ``zero_grad(set_to_none=True)`` between steps is harmless and gradient accumulation is not what this does. With
        ``model.training`` the running statistics are updated in place and both ``num_batches_tracked`` grow by one.
        Returns the ``(6,)`` tensor loss_p1, loss_p2, loss_value_p1, loss_value_p2, loss_value, loss; with ``outputs``
        ``(losses, logits_p1 (n, 5), logits_p2 (n, 5), value_p1 (n,), value_p2 (n,))``, the training-mode outputs."""
        return super().step(rowset, first, n, outputs)


class SymmetricGradStep(_GradStep):
    """``MLPGradStep`` for SymmetricMLP: ``model`` is an ``nn.Module`` whose ``state_dict()`` has SymmetricMLP's keys (an
    ``_orig_mod.`` prefix is stripped). ``ValueError`` for a ``Dropout`` with ``p != 0``, a missing key (a PyRatMLP lacks
    the encoders and ``policy_head``), or a parameter or BatchNorm buffer that is not float32 or not contiguous. One
    persistent gradient tensor per parameter is allocated here."""

    _NAME, _PARAM_KEYS, _RUNNING_KEYS, _ROWSET_METHOD = "SymmetricMLP", SYM_PARAM_KEYS, SYM_RUNNING_KEYS, "grad_symmetric_into"
    # shared_encoder.1 sees a batch once, the other three modules once per player
    _TRACKED = tuple((f"{bn}.num_batches_tracked", 1 if bn.startswith("shared_encoder.") else 2) for bn in SYM_BN_MODULES)

    def _read_dims(self) -> None:
        w4, ws, wp = (self._weight(k) for k in ("trunk.4.weight", "shared_encoder.0.weight", "player_encoder.0.weight"))
        self.hidden_dim, self.shared_dim, self.player_dim = int(w4.shape[0]), int(ws.shape[1]), int(wp.shape[1])

    def _check_board(self, rowset: RowSet) -> None:
        hw = rowset.width * rowset.height
        if (5 * hw + 1, hw + 2) != (self.shared_dim, self.player_dim):
            raise ValueError(f"the model's encoders read {self.shared_dim} and {self.player_dim} inputs, a "
                             f"{rowset.width}x{rowset.height} board gives {5 * hw + 1} and {hw + 2}")

    def step(self, rowset: RowSet, first: int, n: int, outputs: bool = False):
        """``MLPGradStep.step`` under the same contract: launched on torch's current stream, nothing synchronised, every
        parameter's ``.grad`` is (again) this object's buffer, overwritten. The batch's statistics are always used; with
        ``model.training`` the running statistics are updated in place (P1's call, then P2's) and
        ``num_batches_tracked`` grows by one for ``shared_encoder.1`` and by two for the other three modules. Returns the
        ``(6,)`` losses, with ``outputs`` also the four training-mode outputs."""
        return super().step(rowset, first, n, outputs)


class LocalValueGradStep(MLPGradStep):
    """``MLPGradStep`` for LocalValueMLP: ``model`` is an ``nn.Module`` whose ``state_dict()`` has LocalValueMLP's keys --
    PyRatMLP's and the four of ``ownership_head.0`` / ``ownership_head.2`` (an ``_orig_mod.`` prefix is stripped; the
    ``outcome_values`` buffer is not read: it only serves the model's ``ownership_value`` output). ``ValueError`` for a
    ``Dropout`` with ``p != 0``, a missing key (a PyRatMLP lacks the head), or a parameter or BatchNorm buffer that is not
    float32 or not contiguous. One persistent gradient tensor per parameter is allocated here."""

    _NAME, _PARAM_KEYS, _ROWSET_METHOD, _N_LOSSES = "LocalValueMLP", LV_PARAM_KEYS, "grad_local_value_into", 7

    def __init__(self, model, policy_weight: float = 1.0, value_weight: float = 1.0, ownership_weight: float = 1.0,
                 dropout_seed: int | None = None) -> None:
        self.ownership_weight = float(ownership_weight)
        super().__init__(model, policy_weight, value_weight, dropout_seed)

    def _refuse(self, named: dict, buffers: dict) -> None:
        pass

    def _read_dims(self) -> None:
        super()._read_dims()
        self.cells = int(self._weight("ownership_head.2.weight").shape[0])

    def _check_board(self, rowset: RowSet) -> None:
        super()._check_board(rowset)
        if 4 * rowset.width * rowset.height != self.cells:
            raise ValueError(f"ownership_head.2.weight has {self.cells} rows, a {rowset.width}x{rowset.height} board has "
                             f"4 * {rowset.width * rowset.height} cell logits")

    def _weights(self) -> tuple:
        return self.policy_weight, self.value_weight, self.ownership_weight

    def _more_outputs(self, rowset: RowSet, n: int, device) -> dict:
        import torch

        return dict(ownership_logits=torch.empty((n, rowset.height, rowset.width, 4), device=device))

    def step(self, rowset: RowSet, first: int, n: int, outputs: bool = False):
        """``MLPGradStep.step`` under the same contract, with the third term in the loss. Returns the ``(7,)`` tensor
        loss_p1, loss_p2, loss_value_p1, loss_value_p2, loss_value, loss, loss_ownership -- ``loss`` includes
        ``ownership_weight * loss_ownership``; with ``outputs`` ``(losses, logits_p1, logits_p2, value_p1, value_p2,
        ownership_logits (n, h, w, 4))``, the training-mode outputs."""
        return _GradStep.step(self, rowset, first, n, outputs)


def _cnn_block_count(model) -> int:
    """the number of ``blocks.<b>`` of a PyRatCNN, at most 8 (``ValueError`` above): CNNGradStep's and GPoolCNNGradStep's"""
    import re

    names = [k.removeprefix(_PREFIX) for k, _ in list(model.named_parameters()) + list(model.named_buffers())]
    n_blocks = 1 + max((int(m.group(1)) for m in (re.match(r"blocks\.(\d+)\.", k) for k in names) if m), default=-1)
    if n_blocks > 8:
        raise ValueError(f"the model has {n_blocks} residual blocks: the step takes at most 8")
    return n_blocks


def _refuse_other_cnns(keys: list) -> None:
    """what neither CNN step computes, under one message each: KataGoCNN and the pooled value head"""
    if any(k.startswith("scalar_encoder.") for k in keys):
        raise ValueError("the model has a scalar_encoder (KataGoCNN): this step is PyRatCNN's")
    if any(k.startswith("value_head.mlp.") for k in keys):
        raise ValueError("the model has a value_head.mlp (PooledValueHead): the step is built for PointValueHead")


class CNNGradStep(_GradStep):
    """``MLPGradStep`` for PyRatCNN as the reference's ``CNNModelConfig`` builds it by default: ``stem`` and ``stem_bn``,
    ``ResBlock``s, ``player_encoder``, ``combiner``, ``MLPPolicyHead`` and ``PointValueHead`` (an ``_orig_mod.`` prefix is
    stripped). ``channels``, ``player_dim``, ``hidden_dim`` and ``n_blocks`` are read from the parameters. ``ValueError``,
    naming the reason, for a ``GPoolResBlock`` among the blocks (its ``pool_bn`` / ``pool_conv`` / ``pool_linear``), a
    ``PooledValueHead`` (``value_head.mlp``), a KataGoCNN (``scalar_encoder``), any ``Dropout`` with ``p != 0`` -- with a
    ``dropout_seed`` too: dropout is not built for this architecture yet --, a missing key, or a parameter or BatchNorm
    buffer that is not float32 or not contiguous. One persistent gradient tensor per parameter is allocated here."""

    _NAME, _ROWSET_METHOD = "PyRatCNN", "grad_cnn_into"

    def __init__(self, model, policy_weight: float = 1.0, value_weight: float = 1.0, dropout_seed: int | None = None) -> None:
        import torch

        from .shards import cnn_bn_modules, cnn_param_keys, cnn_running_keys

        for m in model.modules():
            if isinstance(m, torch.nn.Dropout) and float(m.p) != 0:
                raise ValueError(f"dropout {float(m.p)} is not supported: dropout is not built for PyRatCNN's step yet, "
                                 "with a dropout_seed or without")
        self.n_blocks = n_blocks = _cnn_block_count(model)
        self._PARAM_KEYS, self._RUNNING_KEYS = cnn_param_keys(n_blocks), cnn_running_keys(n_blocks)
        self._TRACKED = tuple((f"{bn}.num_batches_tracked", 1) for bn in cnn_bn_modules(n_blocks))
        super().__init__(model, policy_weight, value_weight, None)

    def _refuse(self, named: dict, buffers: dict) -> None:
        keys = list(named) + list(buffers)
        if any(k.startswith("scalar_encoder.") for k in keys):  # (named first, as it always was)
            _refuse_other_cnns(keys)
        for part in ("pool_bn", "pool_conv", "pool_linear"):
            if any(k.startswith("blocks.") and f".{part}." in k for k in keys):
                raise ValueError(f"a block has a {part} (GPoolResBlock): the step is built for ResBlocks only")
        _refuse_other_cnns(keys)

    def _read_dims(self) -> None:
        stem, enc, comb = self.params["stem.weight"], self._weight("player_encoder.0.weight"), self._weight("combiner.0.weight")
        if stem.dim() != 4 or tuple(stem.shape[1:]) != (5, 3, 3):
            raise ValueError(f"stem.weight has shape {tuple(stem.shape)}, not (channels, 5, 3, 3)")
        self.channels, self.player_dim, self.hidden_dim = int(stem.shape[0]), int(enc.shape[0]), int(comb.shape[0])

    def _dims(self):
        return self.channels, self.player_dim, self.hidden_dim, self.n_blocks

    def _check_board(self, rowset: RowSet) -> None:
        w, h = getattr(self.model, "width", None), getattr(self.model, "height", None)
        inner = getattr(self.model, "_orig_mod", None)
        if w is None and inner is not None:
            w, h = getattr(inner, "width", None), getattr(inner, "height", None)
        if w is not None and (int(w), int(h)) != (rowset.width, rowset.height):
            raise ValueError(f"the model was built for a {w}x{h} board, the row set holds {rowset.width}x{rowset.height}")
        if rowset.width * rowset.height > 256:
            raise ValueError(f"a {rowset.width}x{rowset.height} board has more than 256 cells")

    def step(self, rowset: RowSet, first: int, n: int, outputs: bool = False):
        """``MLPGradStep.step`` under the same contract: launched on torch's current stream, nothing synchronised, every
        parameter's ``.grad`` is (again) this object's buffer, overwritten. The batch's statistics are always used; with
        ``model.training`` the running statistics are updated in place and ``num_batches_tracked`` of every BatchNorm2d
        grows by one. Returns the ``(6,)`` losses, with ``outputs`` also the four training-mode outputs."""
        return super().step(rowset, first, n, outputs)


class GPoolCNNGradStep(CNNGradStep):
    """``CNNGradStep`` for the PyRatCNN the reference's configs train (configs/train_cnn_7x7.yaml: ``res, res, gpool(32)``,
    ``dropout: 0.1``): a trunk of any mix of ``ResBlock`` and ``GPoolResBlock``, and dropout from the library's seeded mask
    (``ar_rows_grad_cnn_gpool``, alpharat_amd/csrc/train_gpool.h). ``blocks`` is read from the model: a block is a gpool
    block iff it has ``pool_conv.weight``, whose first dimension is its ``gpool_channels`` (at most 256). Dropout as the MLP
    steps handle it: without ``dropout_seed`` a ``Dropout`` with ``p != 0`` is refused; with one, all ``Dropout`` modules
    have one ``p`` in ``[0, 1)`` and every training-mode step applies the mask behind the ReLU of ``player_encoder`` and of
    ``combiner`` (``dropout_mask`` calls 0 .. 3) and ``dropout_step`` grows by one. ``ValueError`` for a ``PooledValueHead``
    or a KataGoCNN, with ``CNNGradStep``'s messages, and for what it refuses otherwise. A model of ``ResBlock``s alone gives
    the bytes ``CNNGradStep`` gives."""

    _ROWSET_METHOD = "grad_cnn_gpool_into"

    def __init__(self, model, policy_weight: float = 1.0, value_weight: float = 1.0, dropout_seed: int | None = None) -> None:
        from .shards import cnn_gpool_bn_modules, cnn_gpool_param_keys, cnn_gpool_running_keys

        named = {k.removeprefix(_PREFIX): v for k, v in model.named_parameters()}
        self.n_blocks = n_blocks = _cnn_block_count(model)
        blocks = []
        for b in range(n_blocks):
            w = named.get(f"blocks.{b}.pool_conv.weight")
            if w is None:  # a ResBlock: it may have nothing of a pool path, whose parameters would get no gradient
                for k in named:
                    if k.startswith((f"blocks.{b}.pool_bn.", f"blocks.{b}.pool_linear.")):
                        raise ValueError(f"blocks.{b} has {k.split('.', 2)[2]} and no pool_conv.weight: neither a ResBlock nor a "
                                         "GPoolResBlock")
            blocks.append(0 if w is None else int(w.shape[0]))
            if blocks[-1] > 256:
                raise ValueError(f"blocks.{b} has gpool_channels {blocks[-1]}: the step takes at most 256")
        self.blocks = tuple(blocks)
        self._PARAM_KEYS, self._RUNNING_KEYS = cnn_gpool_param_keys(self.blocks), cnn_gpool_running_keys(self.blocks)
        self._TRACKED = tuple((f"{bn}.num_batches_tracked", 1) for bn in cnn_gpool_bn_modules(self.blocks))
        _GradStep.__init__(self, model, policy_weight, value_weight, dropout_seed)

    def _refuse(self, named: dict, buffers: dict) -> None:
        _refuse_other_cnns(list(named) + list(buffers))

    def _read_dims(self) -> None:
        super()._read_dims()
        for b, g in enumerate(self.blocks):
            if g:
                conv, lin = self.params[f"blocks.{b}.pool_conv.weight"], self._weight(f"blocks.{b}.pool_linear.weight")
                if tuple(conv.shape) != (g, self.channels, 1, 1) or tuple(lin.shape) != (self.channels, 2 * g):
                    raise ValueError(f"blocks.{b}: pool_conv.weight has shape {tuple(conv.shape)} and pool_linear.weight "
                                     f"{tuple(lin.shape)}, not ({g}, {self.channels}, 1, 1) and ({self.channels}, {2 * g})")

    def _dims_args(self) -> tuple:
        return self._dims(), self.blocks

    def step(self, rowset: RowSet, first: int, n: int, outputs: bool = False):
        """``CNNGradStep.step`` under the same contract; ``num_batches_tracked`` of every BatchNorm2d, each ``pool_bn``
        included, grows by one in training mode, and with a ``dropout_seed`` so does ``dropout_step``."""
        return _GradStep.step(self, rowset, first, n, outputs)


def dropout_mask(seed: int, step: int, call: int, n: int, hidden_dim: int, p: float, device_index: int = 0):
    """The mask of BatchNorm call ``call`` of training step ``step`` under ``dropout_seed`` ``seed``, as the device's own
    generator gives it (``ar_train_dropout_mask``): a bool tensor ``(n, hidden_dim)`` on the device, True where the element
    is kept. ``call``: PyRatMLP and LocalValueMLP 0 ``trunk.3``, 1 ``trunk.7``; SymmetricMLP 0 ``shared_encoder``, 1 / 2
    ``player_encoder`` on P1's / P2's rows, 3 / 4 ``trunk.3``, 5 / 6 ``trunk.7``; PyRatCNN (``GPoolCNNGradStep``) 0 / 1
    ``player_encoder`` on P1's / P2's rows with ``hidden_dim`` = ``player_dim``, 2 / 3 ``combiner`` on P1's / P2's rows.
    ``ValueError`` for ``p`` outside ``[0, 1)``, ``n`` outside 1 .. 65536 or a ``hidden_dim`` that is no multiple of 32 up
    to 256."""
    import ctypes as C

    import torch

    from . import _lib

    n, hidden_dim = int(n), int(hidden_dim)
    if n < 0 or hidden_dim < 0 or int(call) < 0:
        raise ValueError("call, n and hidden_dim must not be negative")
    keep = torch.empty((n, hidden_dim), dtype=torch.uint8, device=torch.device("cuda", int(device_index)))
    stream = torch.cuda.current_stream(int(device_index))
    _lib.check(_lib.load().ar_train_dropout_mask(int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF, int(call), n,
                                                 hidden_dim, float(p), C.c_void_p(keep.data_ptr()),
                                                 C.c_void_p(stream.cuda_stream)))
    return keep.bool()
