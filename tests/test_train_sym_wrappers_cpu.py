"""CPU: alpharat_amd/train.py SymmetricGradStep's refusals and the tensor checks of RowSet.grad_symmetric_into, without a
device; the new entry point is declared and exported (tests/test_abi_surface.py then covers its presence in the library)."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch
from torch import nn

ROOT = Path(__file__).resolve().parent.parent


def _SYM(width=5, height=5, hidden=32, dropout=0.0):
    import _sym_torch as ST

    return ST.Symmetric(width, height, hidden, dropout)


def test_step_accepts_the_architecture():
    from alpharat_amd.dataset import SymmetricGradStep as exported
    from alpharat_amd.shards import SYM_PARAM_KEYS, SYM_RUNNING_KEYS
    from alpharat_amd.train import SymmetricGradStep

    assert exported is SymmetricGradStep
    model = _SYM()
    step = SymmetricGradStep(model, policy_weight=1.0, value_weight=0.5)
    assert (step.hidden_dim, step.shared_dim, step.player_dim) == (32, 126, 27)
    assert tuple(k for k, _ in model.named_parameters()) == SYM_PARAM_KEYS == tuple(step.grads)  # torch's own order
    assert len(SYM_PARAM_KEYS) == 20 and len(SYM_RUNNING_KEYS) == 8 and set(step.running) == set(SYM_RUNNING_KEYS)
    for k, p in model.named_parameters():
        assert step.grads[k].shape == p.shape and step.grads[k].dtype == torch.float32


def test_step_refuses_what_it_does_not_compute():
    import _mlp_torch as MT
    from alpharat_amd.train import MLPGradStep, SymmetricGradStep

    with pytest.raises(ValueError, match="dropout"):
        SymmetricGradStep(_SYM(dropout=0.1))
    with pytest.raises(ValueError, match=r"shared_encoder\.0\.weight.*policy_head\.weight"):  # a PyRatMLP: the missing keys
        SymmetricGradStep(MT.MLP(181, 32))
    with pytest.raises(ValueError, match="policy_p1_head"):  # and the other way round, as before
        MLPGradStep(_SYM())
    missing = _SYM()
    del missing.value_head
    with pytest.raises(ValueError, match="value_head"):
        SymmetricGradStep(missing)
    with pytest.raises(ValueError, match="float32|dtype"):
        SymmetricGradStep(_SYM().double())
    strided = _SYM()
    strided.trunk[4].weight = nn.Parameter(torch.zeros(32, 32).T)
    assert not strided.trunk[4].weight.is_contiguous()
    with pytest.raises(ValueError, match="contiguous"):
        SymmetricGradStep(strided)


def test_step_refuses_a_board_of_another_size():
    from alpharat_amd.train import SymmetricGradStep

    class Board:  # what step() reads of a RowSet before it touches the library
        width, height, device_index = 7, 5, 0

    with pytest.raises(ValueError, match="7x5"):
        SymmetricGradStep(_SYM(5, 5)).step(Board(), 0, 8)


def test_compiled_prefix_is_stripped():
    from alpharat_amd.train import SymmetricGradStep

    class Wrapper(nn.Module):  # what torch.compile makes of a model's names
        def __init__(self):
            super().__init__()
            self._orig_mod = _SYM()

    assert SymmetricGradStep(Wrapper()).hidden_dim == 32


def test_tensor_checks_need_no_device():
    from alpharat_amd.shards import SYM_PARAM_KEYS, SYM_RUNNING_KEYS, check_grad_tensors, sym_param_shapes

    shapes = sym_param_shapes(5, 5, 32)
    assert shapes["shared_encoder.0.weight"] == (32, 126) and shapes["player_encoder.0.weight"] == (32, 27)
    assert shapes["trunk.0.weight"] == (32, 64) and shapes["policy_head.weight"] == (5, 64) and shapes["value_head.weight"] == (1, 64)
    assert shapes["value_head.bias"] == (1,) and shapes["player_encoder.1.running_var"] == (32,)
    assert {k: tuple(v.shape) for k, v in _SYM().state_dict().items() if k in shapes} == shapes
    dev = torch.device("cpu")
    make = lambda keys: {k: torch.zeros(shapes[k]) for k in keys}  # noqa: E731
    params, grads, running = make(SYM_PARAM_KEYS), make(SYM_PARAM_KEYS), make(SYM_RUNNING_KEYS)
    out = dict(losses=torch.zeros(6), logits_p1=torch.zeros(7, 5), value_p2=torch.zeros(7))
    check = lambda p, g, r, o, d=dev: check_grad_tensors(p, g, r, o, 7, 5, 5, 32, d, architecture="symmetric")  # noqa: E731
    check(params, grads, running, out)
    check(params, grads, None, None)
    for bad, match in ((torch.zeros(32, 64, dtype=torch.float64), "dtype"), (torch.zeros(64, 32).T, "contiguous"),
                       (torch.zeros(32, 63), "shape"), (np.zeros((32, 64), np.float32), "torch tensor")):
        with pytest.raises(ValueError, match=match):
            check(params, dict(grads, **{"trunk.0.weight": bad}), running, out)
    with pytest.raises(ValueError, match="has no"):
        check({k: v for k, v in params.items() if k != "value_head.bias"}, grads, running, out)
    with pytest.raises(ValueError, match="has no"):
        check(params, grads, {k: v for k, v in running.items() if k != "trunk.5.running_var"}, out)
    with pytest.raises(ValueError, match="shape"):
        check(params, grads, running, dict(out, logits_p1=torch.zeros(6, 5)))
    with pytest.raises(ValueError, match="is on"):
        check(params, grads, running, out, torch.device("cuda", 0))
    with pytest.raises(ValueError, match="architecture"):
        check_grad_tensors(params, grads, running, out, 7, 5, 5, 32, dev, architecture="cnn")


def test_symbol_is_declared_and_exported():
    from alpharat_amd import _lib

    header = (ROOT / "include" / "alpharat_hip.h").read_text()
    assert re.search(r"\bint ar_rows_grad_symmetric\s*\(", header)
    assert "ar_rows_grad_symmetric" in _lib.EXPORTS
    assert len(_lib.ArSymTensors._fields_) == 20 == len(_lib.SYM_TENSORS) and len(_lib.ArSymBnStats._fields_) == 8
    for struct in ("ArSymTensors", "ArSymBnStats"):
        assert f"}} {struct};" in header
