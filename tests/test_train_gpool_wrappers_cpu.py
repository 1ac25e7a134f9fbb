"""CPU: alpharat_amd/train.py GPoolCNNGradStep's refusals and dropout bookkeeping, the key functions of
alpharat_amd/shards.py against torch's own order and the reference's (the goldens' state dicts), and the tensor checks of
RowSet.grad_cnn_gpool_into, without a device; the new entry point is declared and exported (tests/test_abi_surface.py then
covers its presence in the library)."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _train_gpool as TG
import _train_gpool_np as NG

ROOT = Path(__file__).resolve().parent.parent


def _model(blocks=(0, 16), **kw):
    import _gpool_train_torch as GT

    return GT.GPoolCNN(5, 5, blocks=blocks, **kw)


@pytest.mark.parametrize("blocks", [(), (0,), (32,), (0, 0, 32), (8, 0, 36, 256), (1,) * 8], ids=str)
def test_key_functions_are_torchs_order(blocks):
    from alpharat_amd.shards import cnn_gpool_bn_modules, cnn_gpool_param_keys, cnn_gpool_param_shapes, cnn_gpool_running_keys, cnn_param_keys

    model = _model(blocks, channels=64, player_dim=24, hidden_dim=32)
    P = sum(1 for g in blocks if g)
    keys = cnn_gpool_param_keys(blocks)
    assert tuple(k for k, _ in model.named_parameters()) == keys == NG.param_keys(blocks)
    assert len(keys) == 11 + 6 * len(blocks) + 5 * P
    running = tuple(k for k, _ in model.named_buffers() if k.endswith(("running_mean", "running_var")))
    assert running == cnn_gpool_running_keys(blocks) == NG.running_keys(blocks) and len(running) == 2 + 4 * len(blocks) + 2 * P
    assert cnn_gpool_bn_modules(blocks) == tuple(k for k, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm2d))
    if not P:
        assert keys == cnn_param_keys(len(blocks))
    shapes = cnn_gpool_param_shapes(5, 5, (64, 24, 32, blocks))
    tensors = dict(model.named_parameters(), **dict(model.named_buffers()))
    for k in keys + running:
        assert tuple(tensors[k].shape) == tuple(shapes[k]), k


@pytest.mark.parametrize("name", TG.GOLDEN)
def test_key_functions_are_the_reference_models_order(name):
    """a golden's state dict is the reference's own model's, in its order: parameters and buffers module by module"""
    from alpharat_amd.shards import cnn_gpool_param_keys, cnn_gpool_running_keys

    with np.load(TG.GOLD / f"{name}.npz") as z:
        stored = [k[3:] for k in z.files if k.startswith("sd/")]
        blocks = tuple(int(g) for g in z["blocks"])
    assert [k for k in stored if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))] == list(cnn_gpool_param_keys(blocks))
    assert [k for k in stored if k.endswith(("running_mean", "running_var"))] == list(cnn_gpool_running_keys(blocks))


def test_a_gpool_block_has_eleven_parameters_in_this_order():
    from alpharat_amd.shards import cnn_gpool_param_keys, cnn_gpool_running_keys

    assert cnn_gpool_param_keys((32,))[3:14] == tuple(f"blocks.0.{k}" for k in (
        "bn1.weight", "bn1.bias", "conv1.weight", "bn2.weight", "bn2.bias", "conv2.weight", "pool_bn.weight", "pool_bn.bias",
        "pool_conv.weight", "pool_linear.weight", "pool_linear.bias"))
    assert cnn_gpool_running_keys((32,))[2:] == tuple(f"blocks.0.{k}" for k in (
        "bn1.running_mean", "bn1.running_var", "bn2.running_mean", "bn2.running_var", "pool_bn.running_mean", "pool_bn.running_var"))
    with pytest.raises(ValueError):
        cnn_gpool_param_keys((0,) * 9)


def test_step_reads_the_blocks_from_the_model():
    from alpharat_amd.dataset import GPoolCNNGradStep as exported
    from alpharat_amd.shards import cnn_gpool_param_keys
    from alpharat_amd.train import CNNGradStep, GPoolCNNGradStep

    assert exported is GPoolCNNGradStep
    model = _model((0, 0, 32), channels=64)
    step = GPoolCNNGradStep(model, policy_weight=1.0, value_weight=0.5)
    assert step.blocks == (0, 0, 32) and step._dims() == (64, 32, 64, 3) and step._dims_args() == ((64, 32, 64, 3), (0, 0, 32))
    assert tuple(step.grads) == cnn_gpool_param_keys((0, 0, 32))
    assert len(step._tracked) == 1 + 2 * 3 + 1 and all(calls == 1 for _, calls in step._tracked)
    assert step._ROWSET_METHOD == "grad_cnn_gpool_into" and step.dropout_seed is None and step.dropout_p == 0.0
    with pytest.raises(ValueError, match="GPoolResBlock"):  # the ResBlock step still refuses it
        CNNGradStep(model)
    plain = GPoolCNNGradStep(_model((0, 0)))
    assert plain.blocks == (0, 0) and tuple(plain.grads) == tuple(CNNGradStep(_model((0, 0))).grads)


def test_step_refuses_what_it_does_not_compute():
    import _cnn_train_torch as CT
    from alpharat_amd.train import GPoolCNNGradStep

    with pytest.raises(ValueError, match=r"value_head\.mlp.*PooledValueHead"):
        GPoolCNNGradStep(CT.CNN(5, 5, pooled_value=True))
    with pytest.raises(ValueError, match="scalar_encoder.*KataGoCNN"):
        GPoolCNNGradStep(CT.CNN(5, 5, katago=True))
    with pytest.raises(ValueError, match="at most 8"):
        GPoolCNNGradStep(_model((0,) * 9))
    wide = _model((16,))
    wide.blocks[0].pool_conv = torch.nn.Conv2d(32, 257, 1, bias=False)
    wide.blocks[0].pool_linear = torch.nn.Linear(514, 32)
    with pytest.raises(ValueError, match="at most 256"):
        GPoolCNNGradStep(wide)
    odd = _model((16,))
    odd.blocks[0].pool_linear = torch.nn.Linear(16, 32)  # not 2 G inputs
    with pytest.raises(ValueError, match="pool_linear"):
        GPoolCNNGradStep(odd)
    half = _model((16,))
    del half.blocks[0].pool_conv  # a pool path without its convolution: its parameters would get no gradient
    with pytest.raises(ValueError, match=r"blocks\.0 has pool_bn\.weight and no pool_conv\.weight"):
        GPoolCNNGradStep(half)
    missing = _model((16,))
    del missing.blocks[0].pool_bn
    with pytest.raises(ValueError, match=r"blocks\.0\.pool_bn\.weight"):
        GPoolCNNGradStep(missing)
    with pytest.raises(ValueError, match="float32|dtype"):
        GPoolCNNGradStep(_model((16,)).double())


def test_dropout_bookkeeping():
    from alpharat_amd.train import GPoolCNNGradStep

    with pytest.raises(ValueError, match="dropout 0.1.*dropout_seed"):  # refused without a seed
        GPoolCNNGradStep(_model(dropout=0.1))
    step = GPoolCNNGradStep(_model(dropout=0.1), dropout_seed=7)
    assert (step.dropout_seed, step.dropout_step) == (7, 0) and step.dropout_p == pytest.approx(0.1)
    assert GPoolCNNGradStep(_model(), dropout_seed=7).dropout_p == 0.0  # a seed and no dropout: nothing to apply
    uneven = _model(dropout=0.1)
    uneven.combiner[2].p = 0.2
    with pytest.raises(ValueError, match="different p"):
        GPoolCNNGradStep(uneven, dropout_seed=1)
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        GPoolCNNGradStep(_model(dropout=1.0), dropout_seed=1)

    # what a step hands to the row set: the triple in training mode only, and the counter grows with it
    calls = []

    class FakeRowSet:
        width = height = 5
        device_index = 0

        def grad_cnn_gpool_into(self, first, n, dims, blocks, params, grads, running, pw, vw, out, dropout=None):
            calls.append((dims, blocks, running is not None, dropout))

    model = _model(dropout=0.1)
    step = GPoolCNNGradStep(model, dropout_seed=7)
    real = torch.empty

    def cpu_empty(*a, device=None, **kw):
        return real(*a, **kw)

    torch.empty = cpu_empty  # the step allocates its losses on the row set's device; there is none here
    try:
        model.train()
        step.step(FakeRowSet(), 0, 4)
        step.step(FakeRowSet(), 0, 4)
        model.eval()
        step.step(FakeRowSet(), 0, 4)
    finally:
        torch.empty = real
    p = float(step.dropout_p)
    assert calls == [((32, 32, 64, 2), (0, 16), True, (p, 7, 0)), ((32, 32, 64, 2), (0, 16), True, (p, 7, 1)),
                     ((32, 32, 64, 2), (0, 16), False, None)]
    assert step.dropout_step == 2
    tracked = {k: int(v) for k, v in model.named_buffers() if k.endswith("num_batches_tracked")}
    assert set(tracked) == {f"{bn}.num_batches_tracked" for bn in NG.bn_modules((0, 16))} and set(tracked.values()) == {2}


def test_export_is_declared_and_listed():
    from alpharat_amd import _lib

    header = (ROOT / "include" / "alpharat_hip.h").read_text()
    assert re.search(r"\bint\s+ar_rows_grad_cnn_gpool\s*\(", header)
    for name in ("ArCnnPoolDims", "ArCnnPoolBlock", "ArCnnPoolTensors", "ArCnnPoolStats"):
        assert re.search(rf"typedef struct {name}\b", header), name
    assert "ar_rows_grad_cnn_gpool" in _lib.EXPORTS and "ar_rows_grad_cnn" in _lib.EXPORTS
    args = _lib.EXPORTS["ar_rows_grad_cnn_gpool"][1]
    assert len(args) == 16
    import ctypes as C

    assert C.sizeof(_lib.ArCnnPoolDims) == 32 and C.sizeof(_lib.ArCnnPoolTensors) == 40 * C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.ArCnnPoolStats) == 16 * C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.ArCnnTensors) == 59 * C.sizeof(C.c_void_p) and C.sizeof(_lib.ArCnnBnStats) == 34 * C.sizeof(C.c_void_p)
    assert _lib.CNN_POOL_TENSORS[:5] == ("b0_pool_bn_w", "b0_pool_bn_b", "b0_pool_conv_w", "b0_pool_linear_w", "b0_pool_linear_b")


def test_grad_cnn_gpool_into_checks_its_tensors_before_the_library():
    from alpharat_amd.shards import check_grad_tensors, cnn_gpool_param_keys, cnn_gpool_param_shapes, cnn_gpool_running_keys

    blocks, dims = (0, 16), (32, 32, 64, (0, 16))
    shapes = cnn_gpool_param_shapes(5, 5, dims)
    dev = torch.device("cpu")
    params = {k: torch.zeros(shapes[k]) for k in cnn_gpool_param_keys(blocks)}
    grads = {k: torch.zeros(shapes[k]) for k in cnn_gpool_param_keys(blocks)}
    running = {k: torch.zeros(shapes[k]) for k in cnn_gpool_running_keys(blocks)}
    check_grad_tensors(params, grads, running, None, 4, 5, 5, dims, dev, architecture="pyrat_cnn_gpool")
    assert shapes["blocks.1.pool_conv.weight"] == (16, 32, 1, 1) and shapes["blocks.1.pool_linear.weight"] == (32, 32)
    with pytest.raises(ValueError, match="pool_conv.weight"):
        check_grad_tensors({k: v for k, v in params.items() if k != "blocks.1.pool_conv.weight"}, grads, running, None, 4, 5, 5, dims,
                           dev, architecture="pyrat_cnn_gpool")
    with pytest.raises(ValueError, match="pool_linear.weight.*shape"):
        check_grad_tensors(dict(params, **{"blocks.1.pool_linear.weight": torch.zeros(32, 16)}), grads, running, None, 4, 5, 5, dims,
                           dev, architecture="pyrat_cnn_gpool")
    with pytest.raises(ValueError, match="pool_bn.running_var"):
        check_grad_tensors(params, grads, {k: v for k, v in running.items() if k != "blocks.1.pool_bn.running_var"}, None, 4, 5, 5,
                           dims, dev, architecture="pyrat_cnn_gpool")
