"""Player-swap augmentation in NumPy -- test infrastructure only.

A restatement, written from its text, of alpharat/nn/augmentation.py:86-184 swap_player_perspective_batch on the eight arrays
of tests/_rows_np.py (value_* and action_* of shape (n,) or (n, 1), cheese_outcomes (n, h, w)). It is tied to the reference
by tests/golden/augment (tools/gen_augment_golden.py runs the reference's own function); what the tests compare with it is
equality of bytes, floats through a uint32 view: the score difference of a swapped row is `-obs`, so 0.0 becomes -0.0.
"""
from __future__ import annotations

import numpy as np

from _rows_np import KEYS


def swap_rows(rows: dict, mask, w: int, h: int) -> dict:
    """The rows with the perspective of the masked ones exchanged; `rows` is left as it is."""
    mask = np.asarray(mask, bool)
    hw = w * h
    p1, p2, s = slice(hw * 4, hw * 5), slice(hw * 5, hw * 6), hw * 7  # flat.py FlatObsLayout
    obs = rows["observation"]
    sw = obs.copy()                                                    # :129
    sw[:, p1], sw[:, p2] = obs[:, p2], obs[:, p1]                      # :132-133
    sw[:, s + 0] = -obs[:, s + 0]                                      # :136  (-(0.0) is -0.0)
    sw[:, s + 2], sw[:, s + 3] = obs[:, s + 3], obs[:, s + 2]          # :139-140 mud
    sw[:, s + 4], sw[:, s + 5] = obs[:, s + 5], obs[:, s + 4]          # :143-144 scores

    def where(a, b):  # torch.where(mask broadcast over the row, a, b)
        return np.where(mask.reshape((-1,) + (1,) * (b.ndim - 1)), a, b)

    out = {"observation": where(sw, obs)}                              # :146
    for k in ("policy", "action", "value"):                            # :150-167
        a, b = rows[f"{k}_p1"], rows[f"{k}_p2"]
        out[f"{k}_p1"], out[f"{k}_p2"] = where(b, a), where(a, b)
    co = rows["cheese_outcomes"]
    sc = co.copy()                                                     # :175-181: 0 <-> 3, the rest as it is
    sc[co == 0] = 3
    sc[co == 3] = 0
    out["cheese_outcomes"] = where(sc, co)                             # :182
    return {k: np.ascontiguousarray(out[k], dtype=rows[k].dtype) for k in KEYS}


def bits_equal(a: np.ndarray, b: np.ndarray) -> bool:
    """Equality of bytes (for floats: -0.0 != 0.0)."""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
