"""CPU: the float64 restatement of LocalValueMLP's ownership head and loss (tests/_ownership_np.py) equals the reference's
own numbers (tests/golden/ownership, written by tools/gen_ownership_golden.py from the reference's model and loss)."""
from pathlib import Path

import numpy as np
import pytest

import _mlp_np
import _ownership_np as ON

GOLD = Path(__file__).resolve().parent / "golden" / "ownership"
CASES = ("lv_5x5_h32", "lv_7x5_h64")


def load(name):
    z = np.load(GOLD / f"{name}.npz")
    return z, {k[3:]: z[k] for k in z.files if k.startswith("sd/")}


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference(name):
    z, sd = load(name)
    n, B = len(z["observation"]), int(z["batch_rows"])
    logits = ON.forward(sd, z["observation"])
    np.testing.assert_allclose(logits.reshape(z["ownership_logits"].shape), z["ownership_logits"], atol=1e-5, rtol=1e-5)
    ce, cells, value = ON.row_terms(logits, z["cheese_outcomes"])
    assert np.array_equal(cells, (z["cheese_outcomes"].reshape(n, -1) >= 0).sum(axis=1))
    np.testing.assert_allclose(value, z["ownership_value"], atol=1e-5, rtol=1e-5)
    # the loss is compared at 1e-6: both sides from the f32 model's logits, so only the f32 loss arithmetic separates them
    ce32, cells32, _ = ON.row_terms(z["ownership_logits"], z["cheese_outcomes"])
    assert abs(ON.loss_ownership(ce32, cells32, B) - float(z["loss_ownership"])) <= 1e-6
    assert abs(ON.loss_ownership(ce32, cells32, 0) - float(z["loss_ownership_one_batch"])) <= 1e-6
    assert abs(ON.loss_ownership(ce, cells, B) - float(z["loss_ownership"])) <= 1e-5


def test_a_batch_without_an_active_cell_counts_zero():
    z, _ = load("lv_5x5_h32")
    B = int(z["batch_rows"])
    cells = (z["cheese_outcomes"].reshape(len(z["observation"]), -1) >= 0).sum(axis=1)
    per_batch = [int(cells[lo:lo + B].sum()) for lo in range(0, len(cells), B)]
    assert 0 in per_batch and len(cells) % B != 0  # the 0.0 branch and a short last batch are in the fixture
    ce, cells, _ = ON.row_terms(z["ownership_logits"], z["cheese_outcomes"])
    assert ON.loss_ownership(ce, cells, B) != pytest.approx(ON.loss_ownership(ce, cells, 0), abs=1e-4)


@pytest.mark.parametrize("name", CASES)
def test_total_loss_of_the_reference(name):
    """loss = policy_weight (p1 + p2) + value_weight loss_value + ownership_weight loss_ownership, per batch, batches
    weighted by size: from the reference's own outputs and the restated terms"""
    z, sd = load(name)
    n, B = len(z["observation"]), int(z["batch_rows"])
    pw, vw, ow = z["weights"]
    fwd = _mlp_np.mlp_forward(sd, z["observation"])
    for k in ("logits_p1", "logits_p2"):
        np.testing.assert_allclose(fwd[k], z[k], atol=1e-5, rtol=1e-5)
    ce, cells, _ = ON.row_terms(z["ownership_logits"], z["cheese_outcomes"])

    def logsoftmax(l):
        l = np.asarray(l, np.float64)
        m = l.max(axis=1, keepdims=True)
        return l - m - np.log(np.exp(l - m).sum(axis=1, keepdims=True))

    ce_p = [-(z[f"policy_p{p}"].astype(np.float64) * logsoftmax(z[f"logits_p{p}"])).sum(axis=1) for p in (1, 2)]
    sq = [(z[f"pred_value_p{p}"].astype(np.float64) - z[f"value_p{p}"]) ** 2 for p in (1, 2)]
    total = 0.0
    for lo in range(0, n, B):
        s = slice(lo, lo + B)
        k = int(cells[s].sum())
        own = ce[s].sum() / k if k else 0.0
        total += len(ce[s]) * (pw * (ce_p[0][s].mean() + ce_p[1][s].mean()) + vw * 0.5 * (sq[0][s].mean() + sq[1][s].mean())
                               + ow * own)
    assert abs(total / n - float(z["loss"])) <= 1e-5
