"""The NumPy restatement of the player-swap augmentation (tests/_augment_np.py) against what the reference's own
swap_player_perspective_batch wrote (tests/golden/augment, tools/gen_augment_golden.py). Equality of bytes: floats are
compared through their bits, so that -0.0 is not 0.0."""
from pathlib import Path

import numpy as np
import pytest

import _augment_np as A
import _rows_np as R

GOLDEN = sorted((Path(__file__).parent / "golden" / "augment").glob("*.npz"))


def _load(path):
    with np.load(path) as z:
        return (int(z["width"]), int(z["height"]), z["mask"], {k: z[f"in_{k}"] for k in R.KEYS},
                {k: z[f"out_{k}"] for k in R.KEYS})


def _assert_bits(got, want, what):
    for k in R.KEYS:
        assert A.bits_equal(got[k], want[k]), (what, k)


def test_the_fixtures_are_there():
    assert [p.stem for p in GOLDEN] == ["capture_5x5", "mud_7x5", "open_5x5"]


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: p.stem)
def test_swap_rows_reproduces_the_reference(path):
    w, h, mask, rows, want = _load(path)
    assert mask.any() and not mask.all()
    before = {k: rows[k].copy() for k in R.KEYS}
    _assert_bits(A.swap_rows(rows, mask, w, h), want, path.stem)
    _assert_bits(rows, before, "the input is left as it is")


@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: p.stem)
def test_swap_rows_is_an_involution_and_leaves_unmasked_rows(path):
    w, h, mask, rows, _ = _load(path)
    n = len(mask)
    once = A.swap_rows(rows, mask, w, h)
    for k in R.KEYS:
        assert once[k][~mask].tobytes() == rows[k][~mask].tobytes(), k
    assert once["observation"][mask].tobytes() != rows["observation"][mask].tobytes()
    twice = A.swap_rows(once, mask, w, h)
    # -(-x) is x for every float, -0.0 included: the second swap gives the first bytes back
    _assert_bits(twice, rows, path.stem)
    _assert_bits(A.swap_rows(rows, np.zeros(n, bool), w, h), rows, "no row masked")
    full = A.swap_rows(A.swap_rows(rows, np.ones(n, bool), w, h), np.ones(n, bool), w, h)
    _assert_bits(full, rows, "every row masked, twice")


def test_the_fixtures_cover_what_they_are_there_for():
    by = {p.stem: _load(p) for p in GOLDEN}
    # a score difference of 0 becomes -0.0: sign bit 1, magnitude 0
    w, h, mask, rows, want = by["open_5x5"]
    s0 = want["observation"][:, w * h * 7].view(np.uint32)
    assert mask[0] and s0[0] == 0x80000000 and rows["observation"][0, w * h * 7].view(np.uint32) == 0
    # mud timers that differ, exchanged
    w, h, mask, rows, want = by["mud_7x5"]
    s = w * h * 7
    differ = mask & (rows["observation"][:, s + 2] != rows["observation"][:, s + 3])
    assert differ.any()
    assert (want["observation"][differ, s + 2] == rows["observation"][differ, s + 3]).all()
    assert (rows["observation"][:, : w * h * 4] >= 0.2).any()
    # every cheese outcome, and 0 <-> 3 only
    w, h, mask, rows, want = by["capture_5x5"]
    co, sw = rows["cheese_outcomes"][mask], want["cheese_outcomes"][mask]
    assert set(np.unique(co)) == {-1, 0, 1, 2, 3}
    assert (sw[co == 0] == 3).all() and (sw[co == 3] == 0).all()
    for v in (-1, 1, 2):
        assert (sw[co == v] == v).all()
    assert rows["value_p1"].shape == (len(mask), 1)  # as the reference's trainer holds them
