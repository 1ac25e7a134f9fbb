"""CPU: alpharat_amd/train.py CNNGradStep's refusals, the key lists and shapes of alpharat_amd/shards.py and the tensor
checks of RowSet.grad_cnn_into, without a device; the new entry point is declared and exported (tests/test_abi_surface.py
then covers its presence in the library)."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch
from torch import nn

ROOT = Path(__file__).resolve().parent.parent


def _CNN(width=5, height=5, **kw):
    import _cnn_train_torch as CT

    return CT.CNN(width, height, **kw)


def test_step_accepts_the_architecture():
    from alpharat_amd.dataset import CNNGradStep as exported
    from alpharat_amd.shards import cnn_param_keys, cnn_running_keys
    from alpharat_amd.train import CNNGradStep

    assert exported is CNNGradStep
    for B in (0, 1, 3, 8):
        model = _CNN(channels=64, player_dim=24, hidden_dim=32, n_blocks=B)
        step = CNNGradStep(model, policy_weight=1.0, value_weight=0.5)
        assert (step.channels, step.player_dim, step.hidden_dim, step.n_blocks) == (64, 24, 32, B) == step._dims()
        assert tuple(k for k, _ in model.named_parameters()) == cnn_param_keys(B) == tuple(step.grads)  # torch's own order
        assert len(cnn_param_keys(B)) == 11 + 6 * B and len(cnn_running_keys(B)) == 2 + 4 * B
        assert set(step.running) == set(cnn_running_keys(B))
        assert len(step._tracked) == 1 + 2 * B and all(calls == 1 for _, calls in step._tracked)
        for k, p in model.named_parameters():
            assert step.grads[k].shape == p.shape and step.grads[k].dtype == torch.float32


def test_key_lists_are_the_reference_models_names():
    from alpharat_amd.shards import cnn_param_keys, cnn_running_keys

    assert cnn_param_keys(1) == ("stem.weight", "stem_bn.weight", "stem_bn.bias", "blocks.0.bn1.weight", "blocks.0.bn1.bias",
                                 "blocks.0.conv1.weight", "blocks.0.bn2.weight", "blocks.0.bn2.bias", "blocks.0.conv2.weight",
                                 "player_encoder.0.weight", "player_encoder.0.bias", "combiner.0.weight", "combiner.0.bias",
                                 "policy_head.linear.weight", "policy_head.linear.bias", "value_head.linear.weight",
                                 "value_head.linear.bias")
    assert cnn_running_keys(1) == ("stem_bn.running_mean", "stem_bn.running_var", "blocks.0.bn1.running_mean",
                                   "blocks.0.bn1.running_var", "blocks.0.bn2.running_mean", "blocks.0.bn2.running_var")
    assert cnn_param_keys(0)[3] == "player_encoder.0.weight" and cnn_running_keys(0) == ("stem_bn.running_mean", "stem_bn.running_var")


def test_step_refuses_what_it_does_not_compute():
    import _mlp_torch as MT
    from alpharat_amd.train import CNNGradStep, MLPGradStep

    with pytest.raises(ValueError, match="pool_bn.*GPoolResBlock"):
        CNNGradStep(_CNN(n_blocks=2, gpool=True))
    with pytest.raises(ValueError, match=r"value_head\.mlp.*PooledValueHead"):
        CNNGradStep(_CNN(pooled_value=True))
    with pytest.raises(ValueError, match="scalar_encoder.*KataGoCNN"):
        CNNGradStep(_CNN(katago=True))
    with pytest.raises(ValueError, match="dropout 0.1.*not built"):
        CNNGradStep(_CNN(dropout=0.1))
    with pytest.raises(ValueError, match="dropout 0.1.*not built"):  # a seed does not help: no mask is built for this step
        CNNGradStep(_CNN(dropout=0.1), dropout_seed=3)
    with pytest.raises(ValueError, match=r"stem\.weight.*policy_head\.linear\.weight"):  # a PyRatMLP: the missing keys
        CNNGradStep(MT.MLP(181, 32))
    with pytest.raises(ValueError, match="trunk.0.weight"):  # and the other way round, as before
        MLPGradStep(_CNN())
    missing = _CNN()
    del missing.blocks[0].bn2
    with pytest.raises(ValueError, match=r"blocks\.0\.bn2\.weight"):
        CNNGradStep(missing)
    with pytest.raises(ValueError, match="9 residual blocks"):
        CNNGradStep(_CNN(n_blocks=9))
    with pytest.raises(ValueError, match="float32|dtype"):
        CNNGradStep(_CNN().double())
    strided = _CNN()
    strided.combiner[0].weight = nn.Parameter(torch.zeros(64, 64).T)
    assert not strided.combiner[0].weight.is_contiguous()
    with pytest.raises(ValueError, match="contiguous"):
        CNNGradStep(strided)


def test_step_refuses_a_board_of_another_size():
    from alpharat_amd.train import CNNGradStep

    class Board:  # what step() reads of a RowSet before it touches the library
        width, height, device_index = 7, 5, 0

    with pytest.raises(ValueError, match="5x5.*7x5"):
        CNNGradStep(_CNN(5, 5)).step(Board(), 0, 8)

    class Wrapper(nn.Module):  # what torch.compile makes of a model's names
        def __init__(self):
            super().__init__()
            self._orig_mod = _CNN(5, 5)

    step = CNNGradStep(Wrapper())
    assert step._dims() == (32, 32, 64, 1)
    with pytest.raises(ValueError, match="5x5.*7x5"):
        step.step(Board(), 0, 8)


def test_tensor_checks_need_no_device():
    from alpharat_amd.shards import check_grad_tensors, cnn_param_keys, cnn_param_shapes, cnn_running_keys

    dims = (64, 24, 32, 2)
    shapes = cnn_param_shapes(7, 5, dims)
    assert shapes["stem.weight"] == (64, 5, 3, 3) and shapes["blocks.1.conv2.weight"] == (64, 64, 3, 3)
    assert shapes["player_encoder.0.weight"] == (24, 3) and shapes["combiner.0.weight"] == (32, 88)
    assert shapes["policy_head.linear.weight"] == (5, 64) and shapes["value_head.linear.weight"] == (1, 64)
    assert shapes["value_head.linear.bias"] == (1,) and shapes["blocks.0.bn2.running_var"] == (64,)
    model = _CNN(7, 5, channels=64, player_dim=24, hidden_dim=32, n_blocks=2)
    assert {k: tuple(v.shape) for k, v in model.state_dict().items() if k in shapes} == shapes
    dev = torch.device("cpu")
    pk, rk = cnn_param_keys(2), cnn_running_keys(2)
    make = lambda keys: {k: torch.zeros(shapes[k]) for k in keys}  # noqa: E731
    params, grads, running = make(pk), make(pk), make(rk)
    out = dict(losses=torch.zeros(6), logits_p1=torch.zeros(7, 5), value_p2=torch.zeros(7))
    check = lambda p, g, r, o, d=dev: check_grad_tensors(p, g, r, o, 7, 7, 5, dims, d, architecture="pyrat_cnn")  # noqa: E731
    check(params, grads, running, out)
    check(params, grads, None, None)
    for bad, match in ((torch.zeros(64, 64, 3, 3, dtype=torch.float64), "dtype"), (torch.zeros(3, 3, 64, 64).permute(3, 2, 1, 0), "contiguous"),
                       (torch.zeros(64, 64, 3), "shape"), (np.zeros((64, 64, 3, 3), np.float32), "torch tensor")):
        with pytest.raises(ValueError, match=match):
            check(params, dict(grads, **{"blocks.1.conv1.weight": bad}), running, out)
    with pytest.raises(ValueError, match="has no"):
        check({k: v for k, v in params.items() if k != "value_head.linear.bias"}, grads, running, out)
    with pytest.raises(ValueError, match="has no"):
        check(params, grads, {k: v for k, v in running.items() if k != "blocks.1.bn2.running_var"}, out)
    with pytest.raises(ValueError, match="shape"):
        check(params, grads, running, dict(out, logits_p1=torch.zeros(6, 5)))
    with pytest.raises(ValueError, match="is on"):
        check(params, grads, running, out, torch.device("cuda", 0))


def test_block_slots_of_the_structs():
    from alpharat_amd import _lib
    from alpharat_amd.shards import _cnn_slots, cnn_param_keys, cnn_running_keys

    assert len(_lib.CNN_TENSORS) == 59 and len(_lib.CNN_STATS) == 34
    slots = _cnn_slots(cnn_param_keys(2), 2, 3, 6)
    assert [_lib.CNN_TENSORS[s] for s in slots] == ["stem_w", "stem_bn_w", "stem_bn_b", "b0_bn1_w", "b0_bn1_b", "b0_conv1_w", "b0_bn2_w",
                                                    "b0_bn2_b", "b0_conv2_w", "b1_bn1_w", "b1_bn1_b", "b1_conv1_w", "b1_bn2_w", "b1_bn2_b",
                                                    "b1_conv2_w", "enc_w", "enc_b", "comb_w", "comb_b", "policy_w", "policy_b", "value_w",
                                                    "value_b"]
    assert [_lib.CNN_STATS[s] for s in _cnn_slots(cnn_running_keys(1), 1, 2, 4)] == ["stem_mean", "stem_var", "b0_bn1_mean", "b0_bn1_var",
                                                                                     "b0_bn2_mean", "b0_bn2_var"]
    assert [_lib.CNN_TENSORS[s] for s in _cnn_slots(cnn_param_keys(0), 0, 3, 6)][3] == "enc_w"
    assert _cnn_slots(cnn_param_keys(8), 8, 3, 6) == list(range(59))


def test_symbol_is_declared_and_exported():
    from alpharat_amd import _lib

    header = (ROOT / "include" / "alpharat_hip.h").read_text()
    assert re.search(r"\bint ar_rows_grad_cnn\s*\(", header)
    assert "ar_rows_grad_cnn" in _lib.EXPORTS
    assert len(_lib.ArCnnTensors._fields_) == 59 and len(_lib.ArCnnBnStats._fields_) == 34 and len(_lib.ArCnnDims._fields_) == 4
    for struct in ("ArCnnDims", "ArCnnBlock", "ArCnnTensors", "ArCnnBnStats"):
        assert f"}} {struct};" in header
