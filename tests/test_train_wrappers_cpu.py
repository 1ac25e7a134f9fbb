"""CPU: alpharat_amd/train.py MLPGradStep's refusals and the tensor checks of RowSet.grad_mlp_into, without a device; the
new entry point is declared and exported (tests/test_abi_surface.py then covers its presence in the library)."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch
from torch import nn

ROOT = Path(__file__).resolve().parent.parent


def _MLP(obs_dim=181, hidden=32, dropout=0.0):
    import _mlp_torch as MT

    return MT.MLP(obs_dim, hidden, dropout)


def test_step_accepts_the_architecture():
    from alpharat_amd.dataset import MLPGradStep as exported
    from alpharat_amd.shards import MLP_PARAM_KEYS
    from alpharat_amd.train import MLPGradStep

    assert exported is MLPGradStep
    model = _MLP()
    step = MLPGradStep(model, policy_weight=1.0, value_weight=0.5)
    assert (step.hidden_dim, step.obs_dim) == (32, 181)
    assert set(step.grads) == set(MLP_PARAM_KEYS) == {k for k, _ in model.named_parameters()}
    for k, p in model.named_parameters():
        assert step.grads[k].shape == p.shape and step.grads[k].dtype == torch.float32


def test_step_refuses_what_it_does_not_compute():
    from alpharat_amd.train import MLPGradStep

    with pytest.raises(ValueError, match="dropout"):
        MLPGradStep(_MLP(dropout=0.1))
    missing = _MLP()
    del missing.policy_p2_head
    with pytest.raises(ValueError, match="policy_p2_head"):
        MLPGradStep(missing)
    with pytest.raises(ValueError, match="float32|dtype"):
        MLPGradStep(_MLP().double())
    lv = _MLP()
    lv.ownership_head = nn.Sequential(nn.Linear(32, 32), nn.ReLU(), nn.Linear(32, 100))
    with pytest.raises(ValueError, match="ownership_head"):
        MLPGradStep(lv)


def test_compiled_prefix_is_stripped():
    from alpharat_amd.train import MLPGradStep

    class Wrapper(nn.Module):  # what torch.compile makes of a model's names
        def __init__(self):
            super().__init__()
            self._orig_mod = _MLP()

    assert MLPGradStep(Wrapper()).hidden_dim == 32


def test_tensor_checks_need_no_device():
    from alpharat_amd.shards import MLP_PARAM_KEYS, MLP_RUNNING_KEYS, check_grad_tensors, mlp_param_shapes

    shapes = mlp_param_shapes(5, 5, 32)
    assert shapes["trunk.0.weight"] == (32, 181) and shapes["value_head.weight"] == (2, 32) and shapes["trunk.5.running_var"] == (32,)
    dev = torch.device("cpu")
    make = lambda keys: {k: torch.zeros(shapes[k]) for k in keys}  # noqa: E731
    params, grads, running = make(MLP_PARAM_KEYS), make(MLP_PARAM_KEYS), make(MLP_RUNNING_KEYS)
    out = dict(losses=torch.zeros(6), logits_p1=torch.zeros(7, 5), value_p2=torch.zeros(7))
    check_grad_tensors(params, grads, running, out, 7, 5, 5, 32, dev)
    check_grad_tensors(params, grads, None, None, 7, 5, 5, 32, dev)
    for bad, match in ((torch.zeros(32, 181, dtype=torch.float64), "dtype"), (torch.zeros(181, 32).T, "contiguous"),
                       (torch.zeros(32, 180), "shape"), (np.zeros((32, 181), np.float32), "torch tensor")):
        with pytest.raises(ValueError, match=match):
            check_grad_tensors(params, dict(grads, **{"trunk.0.weight": bad}), running, out, 7, 5, 5, 32, dev)
    with pytest.raises(ValueError, match="has no"):
        check_grad_tensors({k: v for k, v in params.items() if k != "value_head.bias"}, grads, running, out, 7, 5, 5, 32, dev)
    with pytest.raises(ValueError, match="shape"):
        check_grad_tensors(params, grads, running, dict(out, logits_p1=torch.zeros(6, 5)), 7, 5, 5, 32, dev)
    with pytest.raises(ValueError, match="is on"):
        check_grad_tensors(params, grads, running, out, 7, 5, 5, 32, torch.device("cuda", 0))


def test_symbol_is_declared_and_exported():
    from alpharat_amd import _lib

    header = (ROOT / "include" / "alpharat_hip.h").read_text()
    assert re.search(r"\bint ar_rows_grad_mlp\s*\(", header)
    assert "ar_rows_grad_mlp" in _lib.EXPORTS
    assert len(_lib.ArMlpTensors._fields_) == 14 == len(_lib.MLP_TENSORS)
    for struct in ("ArMlpTensors", "ArMlpBnStats", "ArTrainOut"):
        assert f"}} {struct};" in header
