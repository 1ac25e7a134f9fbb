"""CPU: the ownership terms of a cell and of a row (alpharat_amd/csrc/dev_ownership.h, compiled for the CPU by
tests/hostsim_ownership) against the float64 restatement (tests/_ownership_np.py), on random logits and on the reference's
own logits (tests/golden/ownership). Bound: 1e-6 relative to 1 + |term|, f32 expf / logf and f32 terms against float64. An f32
logsumexp carries 6e-8 |lse| whatever the term's size, so the logits here stay below 16 in magnitude, as a head's do."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import _ownership_np as ON

HERE = Path(__file__).resolve().parent / "hostsim_ownership"
GOLD = Path(__file__).resolve().parent / "golden" / "ownership"
_sim = None


def sim() -> C.CDLL:
    global _sim
    if _sim is None:
        subprocess.run(["make", "-s", "-C", str(HERE)], check=True)
        L = C.CDLL(str(HERE / "libownershipsim.so"))
        L.os_rows.restype = None
        L.os_rows.argtypes = [C.c_int, C.c_uint64, C.c_int] + [C.c_void_p] * 6
        L.os_cells.restype = None
        L.os_cells.argtypes = [C.c_uint64] + [C.c_void_p] * 4
        _sim = L
    return _sim


def sim_rows(nw, mask, outcomes, logits):
    n, hw = mask.shape
    mask, outcomes = np.ascontiguousarray(mask, np.uint8), np.ascontiguousarray(outcomes, np.uint8)
    logits = np.ascontiguousarray(logits, np.float32).reshape(n, hw, 4)
    ce, cells, value = np.zeros(n, np.float64), np.zeros(n, np.uint32), np.zeros(n, np.float32)
    sim().os_rows(nw, n, hw, mask.ctypes.data, outcomes.ctypes.data, logits.ctypes.data, ce.ctypes.data, cells.ctypes.data,
                  value.ctypes.data)
    return ce, cells, value


def close(got, want, rel=1e-6):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.all(np.abs(got - want) <= rel * (1 + np.abs(want))), np.abs(got - want).max()


def test_cell_terms_every_class_and_equal_logits():
    rng = np.random.default_rng(0)
    logits = np.clip(rng.standard_normal((400, 4)) * 3, -12, 12).astype(np.float32)
    logits[:8] = np.float32(1.25)  # equal logits: ce = log 4, ev = 0
    logits[8:12] = [[8, -8, 0, 0], [-8, 0, 0, 8], [0, 12, 0, 0], [-12, -12, -12, -12]]  # saturated softmaxes
    targets = (np.arange(400) % 4).astype(np.int32)
    ce, ev = np.zeros(400, np.float32), np.zeros(400, np.float32)
    sim().os_cells(400, logits.ctypes.data, targets.ctypes.data, ce.ctypes.data, ev.ctypes.data)
    want_ce, want_ev = ON.cell_terms(logits, targets)
    close(ce, want_ce)
    close(ev, want_ev)
    close(ce[:8], np.log(4.0))
    assert np.all(ev[:8] == 0.0)


@pytest.mark.parametrize("w,h,nw", [(5, 5, 1), (8, 8, 1), (15, 11, 4), (16, 16, 4)])
def test_row_terms_random(w, h, nw):
    rng = np.random.default_rng(w * 100 + h)
    hw, n = w * h, 40
    logits = (rng.standard_normal((n, hw, 4)) * 3).astype(np.float32)
    outcomes = rng.integers(0, 4, size=(n, hw)).astype(np.uint8)
    mask = (rng.random((n, hw)) < 0.2).astype(np.uint8)
    mask[0] = 0
    mask[0, hw - 1] = 1  # one active cell, the last one
    mask[1] = 0
    mask[1, [0, hw // 2]] = 1  # two
    mask[2] = 1  # all
    mask[3] = 0  # none
    if nw == 4:
        mask[4] = 0
        mask[4, [63, 64, 127, 128]] = 1  # both sides of the cheese words' borders
    ce, cells, value = sim_rows(nw, mask, outcomes, logits)
    targets = np.where(mask > 0, outcomes.astype(np.int64), -1)
    want_ce, want_cells, want_value = ON.row_terms(logits, targets)
    assert np.array_equal(cells, want_cells)
    assert cells[0] == 1 and cells[1] == 2 and cells[2] == hw and cells[3] == 0 and ce[3] == 0.0 and value[3] == 0.0
    close(ce, want_ce)
    close(value, want_value)


@pytest.mark.parametrize("name", ["lv_5x5_h32", "lv_7x5_h64"])
def test_row_terms_on_the_reference_logits(name):
    z = np.load(GOLD / f"{name}.npz")
    n = len(z["observation"])
    co = z["cheese_outcomes"].reshape(n, -1)
    ce, cells, value = sim_rows(1, co >= 0, np.where(co >= 0, co, 0), z["ownership_logits"])
    want_ce, want_cells, want_value = ON.row_terms(z["ownership_logits"], co)
    assert np.array_equal(cells, want_cells)
    close(ce, want_ce)
    close(value, want_value)
    np.testing.assert_allclose(value, z["ownership_value"], atol=1e-5, rtol=1e-5)  # the reference's own ownership_value
    B = int(z["batch_rows"])
    assert abs(ON.loss_ownership(ce, cells, B) - float(z["loss_ownership"])) <= 1e-6 * (1 + float(z["loss_ownership"]))
