"""CPU: dropout in alpharat_amd/train.py's three step classes without a device -- what a ``dropout_seed`` lets through and
what it refuses, the step counter (with a stub where the launch is), and the four new entry points as the header declares
them and alpharat_amd/_lib.py mirrors them (tests/test_abi_surface.py then covers their presence in the library)."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch
from torch import nn

ROOT = Path(__file__).resolve().parent.parent


def _models(dropout):
    import _lv_torch as LT
    import _mlp_torch as MT
    import _sym_torch as ST
    from alpharat_amd.train import LocalValueGradStep, MLPGradStep, SymmetricGradStep

    return [(MLPGradStep, MT.MLP(181, 32, dropout), "grad_mlp_into", 2), (SymmetricGradStep, ST.Symmetric(5, 5, 32, dropout),
                                                                         "grad_symmetric_into", 0),
            (LocalValueGradStep, LT.LocalValue(5, 5, 32, dropout), "grad_local_value_into", 2)]


def test_a_seed_lets_a_model_with_dropout_through():
    for cls, model, _, _ in _models(0.1):
        with pytest.raises(ValueError, match="dropout_seed"):  # as before, and the message names the way out
            cls(model)
        step = cls(model, dropout_seed=7)
        assert (step.dropout_seed, step.dropout_p, step.dropout_step) == (7, 0.1, 0)
    for cls, model, _, _ in _models(0.0):
        assert cls(model).dropout_seed is None and cls(model).dropout_p == 0.0
        step = cls(model, dropout_seed=2 ** 63 + 5)
        assert (step.dropout_seed, step.dropout_p, step.dropout_step) == (2 ** 63 + 5, 0.0, 0)


def test_mixed_rates_and_p_one_are_refused():
    for cls, model, _, _ in _models(0.1):
        next(m for m in model.modules() if isinstance(m, nn.Dropout)).p = 0.2
        with pytest.raises(ValueError, match="different p"):
            cls(model, dropout_seed=1)
    for cls, model, _, _ in _models(1.0):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            cls(model, dropout_seed=1)
        with pytest.raises(ValueError, match="dropout"):
            cls(model)


class _StubRowSet:
    """a row set whose launch only records what it was asked"""

    width = height = 5
    device_index = 0

    def __init__(self):
        self.calls = []

    def _record(self, *args, **kw):
        self.calls.append(kw.get("dropout"))

    grad_mlp_into = grad_symmetric_into = grad_local_value_into = _record


def test_the_counter_starts_grows_and_stays_in_eval_mode(monkeypatch):
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **kw: real_empty(*a, **kw))  # the outputs: no device here
    for cls, model, _, _ in _models(0.1):
        rs = _StubRowSet()
        step = cls(model, dropout_seed=11)
        model.train()
        step.step(rs, 0, 8)
        step.step(rs, 8, 8)
        assert rs.calls == [(0.1, 11, 0), (0.1, 11, 1)] and step.dropout_step == 2
        model.eval()
        step.step(rs, 0, 8)
        assert rs.calls[2] is None and step.dropout_step == 2  # nn.Dropout is the identity in eval mode
        model.train()
        step.dropout_step = 40  # a resumed run
        step.step(rs, 0, 8)
        assert rs.calls[3] == (0.1, 11, 40) and step.dropout_step == 41
    for cls, model, _, _ in _models(0.0):
        rs = _StubRowSet()
        model.train()
        cls(model).step(rs, 0, 8)
        seeded = cls(model, dropout_seed=3)
        seeded.step(rs, 0, 8)
        assert rs.calls == [None, None]  # without a seed, and at p = 0, the call is the old one
        assert seeded.dropout_step == 1


def test_the_header_declares_the_struct_and_the_four_symbols():
    from alpharat_amd import _lib

    header = (ROOT / "include" / "alpharat_hip.h").read_text()
    assert re.search(r"typedef struct ArTrainDropout \{\s*float p;\s*uint64_t seed;\s*uint64_t step;\s*\} ArTrainDropout;", header)
    assert [f[0] for f in _lib.ArTrainDropout._fields_] == ["p", "seed", "step"]
    assert [f[1] for f in _lib.ArTrainDropout._fields_] == [C.c_float, C.c_uint64, C.c_uint64]
    assert C.sizeof(_lib.ArTrainDropout) == 24 and _lib.ArTrainDropout.seed.offset == 8 and _lib.ArTrainDropout.step.offset == 16
    for old in ("ar_rows_grad_mlp", "ar_rows_grad_symmetric", "ar_rows_grad_local_value"):
        new = old + "_dropout"
        assert re.search(rf"\bint {new}\s*\(", header) and new in _lib.EXPORTS
        # the old signature with the dropout in front of the stream
        res, args = _lib.EXPORTS[old]
        assert _lib.EXPORTS[new] == (res, args[:-1] + [C.POINTER(_lib.ArTrainDropout), args[-1]])
        decl = re.search(rf"\bint {new}\s*\(([^;]*)\);", header).group(1)
        assert re.search(r"const ArTrainDropout\* dropout,\s*void\* stream$", decl)
    assert re.search(r"\bint ar_train_dropout_mask\s*\(uint64_t seed, uint64_t step, uint32_t call, uint64_t n, uint32_t hidden_dim, "
                     r"float p,\s*uint8_t\* keep_device, void\* stream\);", header)
    assert _lib.EXPORTS["ar_train_dropout_mask"] == (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_float,
                                                               C.c_void_p, C.c_void_p])


def test_exports_match_the_header():
    from alpharat_amd import _lib
    from alpharat_amd.shards import _GRAD_STEPS

    header = (ROOT / "include" / "alpharat_hip.h").read_text()
    assert set(re.findall(r"\b(ar_[a-z_]+)\s*\(", header)) == set(_lib.EXPORTS)
    # index 5 stays the symbol without dropout; the one with it is that name and a suffix
    assert [_GRAD_STEPS[a][5] for a in ("mlp", "symmetric", "local_value")] == ["ar_rows_grad_mlp", "ar_rows_grad_symmetric",
                                                                                "ar_rows_grad_local_value"]
