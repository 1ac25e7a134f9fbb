"""CPU: alpharat_amd/train.py LocalValueGradStep's refusals and the tensor checks of RowSet.grad_local_value_into, without a
device; the new entry point is declared and exported (tests/test_abi_surface.py then covers its presence in the library) and
its structs keep the order of the keys."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch
from torch import nn

ROOT = Path(__file__).resolve().parent.parent


def _LV(width=5, height=5, hidden=32, dropout=0.0):
    import _lv_torch as LT

    return LT.LocalValue(width, height, hidden, dropout)


def test_step_accepts_the_architecture():
    from alpharat_amd.dataset import LocalValueGradStep as exported
    from alpharat_amd.shards import LV_PARAM_KEYS, MLP_PARAM_KEYS, MLP_RUNNING_KEYS
    from alpharat_amd.train import LocalValueGradStep

    assert exported is LocalValueGradStep
    model = _LV()
    step = LocalValueGradStep(model, policy_weight=1.0, value_weight=0.5, ownership_weight=0.25)
    assert (step.policy_weight, step.value_weight, step.ownership_weight) == (1.0, 0.5, 0.25)
    assert (step.hidden_dim, step.obs_dim, step.cells) == (32, 181, 100)
    assert tuple(k for k, _ in model.named_parameters()) == LV_PARAM_KEYS == tuple(step.grads)  # torch's own order
    assert len(LV_PARAM_KEYS) == 18 and LV_PARAM_KEYS[:14] == MLP_PARAM_KEYS and set(step.running) == set(MLP_RUNNING_KEYS)
    assert "outcome_values" in dict(model.named_buffers())  # there, and not read
    for k, p in model.named_parameters():
        assert step.grads[k].shape == p.shape and step.grads[k].dtype == torch.float32
    assert LocalValueGradStep(model).ownership_weight == 1.0


def test_step_refuses_what_it_does_not_compute():
    import _mlp_torch as MT
    from alpharat_amd.train import LocalValueGradStep, MLPGradStep

    with pytest.raises(ValueError, match=r"LocalValueMLP.*ownership_head\.0\.weight.*ownership_head\.2\.bias"):  # a PyRatMLP
        LocalValueGradStep(MT.MLP(181, 32))
    with pytest.raises(ValueError, match="ownership_head"):  # and the other way round, as before
        MLPGradStep(_LV())
    with pytest.raises(ValueError, match="dropout"):
        LocalValueGradStep(_LV(dropout=0.1))
    with pytest.raises(ValueError, match="float32|dtype"):
        LocalValueGradStep(_LV().double())
    strided = _LV()
    strided.ownership_head[0].weight = nn.Parameter(torch.zeros(32, 32).T)
    assert not strided.ownership_head[0].weight.is_contiguous()
    with pytest.raises(ValueError, match="contiguous"):
        LocalValueGradStep(strided)


def test_step_refuses_a_board_of_another_size():
    from alpharat_amd.train import LocalValueGradStep

    class Board:  # what step() reads of a RowSet before it touches the library
        width, height, device_index = 7, 5, 0

    with pytest.raises(ValueError, match="7x5"):
        LocalValueGradStep(_LV(5, 5)).step(Board(), 0, 8)
    # the trunk fits the board, the ownership head another one
    mixed = _LV(7, 5)
    mixed.ownership_head[2] = nn.Linear(32, 100)
    with pytest.raises(ValueError, match=r"ownership_head\.2\.weight has 100 rows.*7x5"):
        LocalValueGradStep(mixed).step(Board(), 0, 8)


def test_compiled_prefix_is_stripped():
    from alpharat_amd.train import LocalValueGradStep

    class Wrapper(nn.Module):  # what torch.compile makes of a model's names
        def __init__(self):
            super().__init__()
            self._orig_mod = _LV()

    assert LocalValueGradStep(Wrapper()).cells == 100


def test_tensor_checks_need_no_device():
    from alpharat_amd.shards import LV_PARAM_KEYS, MLP_RUNNING_KEYS, check_grad_tensors, lv_param_shapes, mlp_param_shapes

    shapes = lv_param_shapes(7, 5, 32)
    assert shapes["ownership_head.0.weight"] == (32, 32) and shapes["ownership_head.0.bias"] == (32,)
    assert shapes["ownership_head.2.weight"] == (140, 32) and shapes["ownership_head.2.bias"] == (140,)
    assert {k: v for k, v in shapes.items() if k in mlp_param_shapes(7, 5, 32)} == mlp_param_shapes(7, 5, 32)
    assert {k: tuple(v.shape) for k, v in _LV(7, 5).state_dict().items() if k in shapes} == shapes
    dev = torch.device("cpu")
    make = lambda keys: {k: torch.zeros(shapes[k]) for k in keys}  # noqa: E731
    params, grads, running = make(LV_PARAM_KEYS), make(LV_PARAM_KEYS), make(MLP_RUNNING_KEYS)
    out = dict(losses=torch.zeros(7), logits_p1=torch.zeros(9, 5), value_p2=torch.zeros(9), ownership_logits=torch.zeros(9, 5, 7, 4))
    check = lambda p, g, r, o, d=dev: check_grad_tensors(p, g, r, o, 9, 7, 5, 32, d, architecture="local_value")  # noqa: E731
    check(params, grads, running, out)
    check(params, grads, None, None)
    with pytest.raises(ValueError, match="shape"):
        check(params, grads, running, dict(out, losses=torch.zeros(6)))  # seven losses here
    with pytest.raises(ValueError, match="shape"):
        check_grad_tensors({k: params[k] for k in LV_PARAM_KEYS[:14]}, {k: grads[k] for k in LV_PARAM_KEYS[:14]}, running,
                           dict(losses=torch.zeros(7)), 9, 7, 5, 32, dev, architecture="mlp")  # and six there, as before
    with pytest.raises(ValueError, match="shape"):
        check(params, grads, running, dict(out, ownership_logits=torch.zeros(9, 7, 5, 4)))  # (n, h, w, 4)
    for bad, match in ((torch.zeros(140, 32, dtype=torch.float64), "dtype"), (torch.zeros(32, 140).T, "contiguous"),
                       (torch.zeros(100, 32), "shape"), (np.zeros((140, 32), np.float32), "torch tensor")):
        with pytest.raises(ValueError, match=match):
            check(params, dict(grads, **{"ownership_head.2.weight": bad}), running, out)
    with pytest.raises(ValueError, match="has no"):
        check({k: v for k, v in params.items() if k != "ownership_head.0.bias"}, grads, running, out)
    with pytest.raises(ValueError, match="is on"):
        check(params, grads, running, out, torch.device("cuda", 0))


def test_symbol_is_declared_and_exported_and_the_keys_keep_the_structs_order():
    from alpharat_amd import _lib
    from alpharat_amd.shards import _GRAD_STEPS, LV_PARAM_KEYS, LV_TRAIN_OUT_KEYS

    header = (ROOT / "include" / "alpharat_hip.h").read_text()
    assert re.search(r"\bint ar_rows_grad_local_value\s*\(", header)
    assert "ar_rows_grad_local_value" in _lib.EXPORTS
    for struct in ("ArLvTensors", "ArLvTrainOut"):
        assert f"}} {struct};" in header
    # the header's field order is the mirror's, and the keys name the same tensors in the same places
    body = header[header.index("typedef struct ArLvTensors"):header.index("} ArLvTensors;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\*(\w+)", body)
    assert tuple(fields) == _lib.LV_TENSORS == tuple(k for k, _ in _lib.ArLvTensors._fields_) and len(fields) == 18
    assert _lib.LV_TENSORS[:14] == _lib.MLP_TENSORS and C.sizeof(_lib.ArLvTensors) == 18 * C.sizeof(C.c_void_p)
    short = {"trunk.0": "trunk0", "trunk.1": "bn1", "trunk.4": "trunk4", "trunk.5": "bn2", "policy_p1_head": "p1", "policy_p2_head": "p2",
             "value_head": "value", "ownership_head.0": "own0", "ownership_head.2": "own2"}
    assert tuple(f"{short[k.rsplit('.', 1)[0]]}_{k.rsplit('.', 1)[1][0]}" for k in LV_PARAM_KEYS) == _lib.LV_TENSORS
    body = header[header.index("typedef struct ArLvTrainOut"):header.index("} ArLvTrainOut;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert tuple(re.findall(r"\*\s*(\w+)", body)) == LV_TRAIN_OUT_KEYS == tuple(k for k, _ in _lib.ArLvTrainOut._fields_)
    assert tuple(k for k, _ in _lib.ArLvTrainOut._fields_)[:5] == tuple(k for k, _ in _lib.ArTrainOut._fields_)  # the old layout stays
    args = _lib.EXPORTS["ar_rows_grad_local_value"][1]
    assert args.count(C.c_float) == 3 and len(args) == len(_lib.EXPORTS["ar_rows_grad_mlp"][1]) + 1
    assert _GRAD_STEPS["local_value"][5] == "ar_rows_grad_local_value"
