"""CPU: the references of tests/test_gpu_boards.py, pinned on boards above 64 cells before any GPU run.

The oracle's forward (double accumulation) is the GPU tests' reference for PyRatMLP and SymmetricMLP; here it must agree
with a float64 numpy statement of each network (tests/_mlp_np.py) on seeded random blobs. The oracle's encoder must
agree with a numpy statement of the flat layout that tests/golden/encoder pins on 5x5 and 7x5 boards. And the position
generator must produce what those tests rely on: mixed mazes, cheese in every 64-bit word, players on high cells,
mud, unequal scores, turn > 0."""
import numpy as np
import pytest

import _mlp_np
import _oracle as O
from _random_nets import positions, random_mlp, random_symmetric

BOARDS = [(8, 8), (12, 7), (15, 11), (16, 16)]
KEYS = ("logits_p1", "logits_p2", "policy_p1", "policy_p2", "value_p1", "value_p2")


def _encode(og, max_turns=100):
    """flat_encoder.rs's layout: maze (cost / 10, -1 for a wall or the edge), p1 / p2 one-hots, cheese, six scalars"""
    hw = og.w * og.h
    st = og.state()
    cost = og.cost().reshape(-1).astype(np.float32)
    one = lambda p: np.eye(hw, dtype=np.float32)[p[1] * og.w + p[0]]  # noqa: E731
    s1, s2 = np.float32(st["p1_score"]), np.float32(st["p2_score"])
    scalars = np.array([s1 - s2, np.float32(st["turn"]) / np.float32(max_turns), np.float32(st["p1_mud"]) / np.float32(10),
                        np.float32(st["p2_mud"]) / np.float32(10), s1 / np.float32(10), s2 / np.float32(10)], np.float32)
    return np.concatenate([np.where(cost == 0, np.float32(-1), cost / np.float32(10)), one(st["p1"]), one(st["p2"]),
                           og.cheese_mask().astype(np.float32), scalars])


@pytest.mark.parametrize("w,h", BOARDS, ids=lambda v: str(v))
def test_oracle_encoder_matches_the_flat_layout(w, h):
    ogs = positions(w, h, 24, seed=w * 31 + h)
    got = np.stack([og.encode() for og in ogs])
    want = np.stack([_encode(og) for og in ogs])
    np.testing.assert_allclose(got, want, atol=1e-6, rtol=0)
    hw = w * h
    assert got.shape[1] == hw * 7 + 6 and got[:, hw * 7 - 1].any()  # the last cheese cell is read


@pytest.mark.parametrize("arch", ["mlp", "symmetric"])
@pytest.mark.parametrize("w,h", BOARDS, ids=lambda v: str(v))
def test_numpy_forward_matches_the_oracle_forward(arch, w, h, tmp_path):
    from alpharat_amd.weights import write_blob

    H = 64 if w * h <= 64 else 192
    t = (random_mlp if arch == "mlp" else random_symmetric)(w, h, H, seed=w * 100 + h)
    blob = write_blob(tmp_path / f"{arch}.arnet", arch, w, h, t)
    obs = np.stack([og.encode() for og in positions(w, h, 24, seed=w + h)])
    got = O.Net(blob).forward(obs)
    want = _mlp_np.mlp_forward(t, obs) if arch == "mlp" else _mlp_np.symmetric_forward(t, w, h, obs)
    for k in KEYS:
        np.testing.assert_allclose(got[k], want[k], atol=1e-6, rtol=1e-6, err_msg=k)
    # the logits stay in a range where 1e-5 is a meaningful bar
    assert 0.05 < np.abs(want["logits_p1"]).max() < 20


@pytest.mark.parametrize("w,h", [(8, 8), (13, 5), (16, 16), (2, 40)], ids=lambda v: str(v))
def test_positions_reach_every_cheese_word_and_state_field(w, h):
    hw = w * h
    ogs = positions(w, h, 40, seed=3)
    st = [og.state() for og in ogs]
    masks = np.stack([og.cheese_mask() for og in ogs])
    assert len({og.cost().tobytes() for og in ogs}) > 30  # one maze per game
    assert len({og.cost().tobytes() for og in positions(w, h, 12, seed=3, mazes=1)}) == 1
    assert masks[:, hw - 1].mean() > 0.5  # (unless a player stands there)
    for b in range((hw + 63) // 64):
        assert masks[:, 64 * b: 64 * b + 64].any(axis=1).mean() > 0.9, b
    assert all(s["turn"] > 0 for s in st)
    assert sum(s["p1"][1] * w + s["p1"][0] >= hw - max(2, hw // 8) for s in st) >= 10  # player 1 on high cells
    assert any(s["p1_mud"] > 0 for s in st) and any(s["p2_mud"] > 0 for s in st)
    assert any(s["p1_score"] != s["p2_score"] and s["p1_score"] > 0 and s["p2_score"] > 0 for s in st)
    assert (O.Game(w, h).cost() > 0).any() and any((og.cost() >= 2).any() for og in ogs)  # mud on the boards
