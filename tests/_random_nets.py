"""Seeded networks and positions for boards of any size (1 to 256 cells) -- test infrastructure only.

- ``random_mlp`` / ``random_symmetric``: PyRatMLP / SymmetricMLP tensors under the PyTorch ``state_dict`` names, so
  ``write_blob`` and the oracle read them as they read checkpoints. Their first layers have an ``hw`` dimension, so
  they cannot be taken from a golden of another board.
- ``transplant``: a PyRatCNN / KataGoCNN golden's trained tensors, which have no ``hw`` dimension, for another board.
- ``positions``: oracle games on generated mazes with mud, scores, mud timers and cheese in every 64-bit word of the
  cheese mask; ``pyrat`` turns one into the ``PyRat`` the device reads.
"""
from __future__ import annotations

import numpy as np

import _oracle as O


def _linear(rng, t, name, o, i):
    t[f"{name}.weight"] = (rng.standard_normal((o, i)) * np.sqrt(2.0 / i)).astype(np.float32)
    t[f"{name}.bias"] = (rng.standard_normal(o) * 0.1).astype(np.float32)


def _bn(rng, t, name, n):
    t[f"{name}.weight"] = (1 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    t[f"{name}.bias"] = (0.1 * rng.standard_normal(n)).astype(np.float32)
    t[f"{name}.running_mean"] = (0.1 * rng.standard_normal(n)).astype(np.float32)
    t[f"{name}.running_var"] = (1 + 0.1 * rng.random(n)).astype(np.float32)


def _head(rng, t, name, o, i):
    t[f"{name}.weight"] = (rng.standard_normal((o, i)) * 0.2).astype(np.float32)
    t[f"{name}.bias"] = (0.1 * rng.standard_normal(o)).astype(np.float32)


def random_mlp(w: int, h: int, H: int, seed: int) -> dict:
    """PyRatMLP (architecture ``mlp``): trunk.0 / trunk.1 (BN) / trunk.4 / trunk.5 (BN), three heads. `seed`: an int or
    a numpy Generator, which is then advanced past the weights"""
    rng = np.random.default_rng(seed)
    t = {}
    _linear(rng, t, "trunk.0", H, w * h * 7 + 6)
    _linear(rng, t, "trunk.4", H, H)
    for bn in ("trunk.1", "trunk.5"):
        _bn(rng, t, bn, H)
    for name, o in (("policy_p1_head", 5), ("policy_p2_head", 5), ("value_head", 2)):
        _head(rng, t, name, o, H)
    return t


def random_symmetric(w: int, h: int, H: int, seed: int) -> dict:
    """SymmetricMLP (architecture ``symmetric``): shared encoder over [maze, cheese, progress], player encoder over
    [position, mud, score], trunk over [shared, player], policy / value heads over [player trunk, sum of both]"""
    rng = np.random.default_rng(seed)
    hw = w * h
    t = {}
    for lin, bn, i in (("shared_encoder.0", "shared_encoder.1", hw * 5 + 1),
                       ("player_encoder.0", "player_encoder.1", hw + 2), ("trunk.0", "trunk.1", 2 * H),
                       ("trunk.4", "trunk.5", H)):
        _linear(rng, t, lin, H, i)
        _bn(rng, t, bn, H)
    _head(rng, t, "policy_head", 5, 2 * H)
    _head(rng, t, "value_head", 1, 2 * H)
    return t


def transplant(golden_blob, w: int, h: int) -> tuple[str, dict]:
    """(arch, tensors) of a PyRatCNN / KataGoCNN golden: none of their tensors depends on the board size, so written with
    ``write_blob(path, arch, w, h, tensors)`` they are the same trained network on a w x h board"""
    from alpharat_amd.weights import read_blob

    arch, _, _, t = read_blob(golden_blob)
    assert arch in ("cnn", "cnn_katago"), arch
    return arch, t


def _mud_step(og: O.Game) -> int | None:
    """a direction out of player 1's cell over a mud edge, if there is one"""
    x, y = og.state()["p1"]
    ds = [d for d in range(4) if og.cost()[y, x, d] >= 2]
    return ds[0] if ds else None


_DXY = ((0, 1), (1, 0), (0, -1), (-1, 0))  # UP, RIGHT, DOWN, LEFT (y up)


def _eat(og: O.Game, p: int) -> None:
    """player p (0 / 1) steps over an open edge onto a cheese put there for it"""
    st = og.state()
    if st[("p1_mud", "p2_mud")[p]]:
        return
    x, y = st[("p1", "p2")[p]]
    for d in range(4):
        nx, ny = x + _DXY[d][0], y + _DXY[d][1]
        if og.cost()[y, x, d] == 1 and (nx, ny) != st[("p2", "p1")[p]]:
            og.add_cheese(nx, ny)
            og.make_move(d, 4) if p == 0 else og.make_move(4, d)
            return


def positions(w: int, h: int, n: int, seed: int, mazes: int | None = None, max_turns: int = 100) -> list:
    """n oracle games on w x h boards. Game i is on maze ``i % mazes`` (default: a maze of its own, so that a batch binds
    one maze per leaf). Every game: walls and mud from ``random_maze``, player 1 on one of the highest cells, cheese on
    a quarter of the free cells plus cell hw-1 and one cell of every 64-bit word of the mask, 1 to 8 random moves
    (turn > 0, scores, mud timers); every fourth game then has a cheese eaten by one player and two by the other, and
    every third game ends with player 1 stepping into mud where it can."""
    rng = np.random.default_rng(seed)
    hw = w * h
    out = []
    for i in range(n):
        k = i if mazes is None else i % mazes
        mrng = np.random.default_rng([seed, k])
        wall, mud = float(mrng.uniform(0.3, 0.7)), float(mrng.uniform(0.15, 0.35))
        hi = int(rng.integers(max(0, hw - max(2, hw // 8)), hw))
        lo = int(rng.integers(0, hw))
        og = O.Game(w, h, max_turns, p1=(hi % w, hi // w), p2=(lo % w, lo // w))
        og.random_maze(wall, mud, bool(mrng.integers(0, 2)), seed * 7919 + k)
        for c in np.flatnonzero(rng.random(hw) < 0.25):
            if int(c) not in (hi, lo):
                og.add_cheese(int(c) % w, int(c) // w)
        for _ in range(int(rng.integers(1, 9))):
            og.make_move(int(rng.integers(0, 5)), int(rng.integers(0, 5)))
        if i % 4 == 1:  # unequal non-zero scores
            for p in (0, 1, 1):
                _eat(og, p)
        if i % 3 == 0 and og.state()["p1_mud"] == 0:
            d = _mud_step(og)
            if d is not None:
                og.make_move(d, 4)
        st = og.state()
        occupied = {st["p1"][0] + st["p1"][1] * w, st["p2"][0] + st["p2"][1] * w}
        have = og.cheese_mask()
        free = [sorted(set(range(64 * b, min(64 * b + 64, hw))) - occupied) for b in range((hw + 63) // 64)]
        for c in {hw - 1, *(int(rng.choice(f)) for f in free if f)} - occupied:
            if not have[c]:
                og.add_cheese(c % w, c // w)
        out.append(og)
    return out


def pyrat(og: O.Game, max_turns: int = 100):
    """the device's PyRat for an oracle game: its cost, cheese and state"""
    from alpharat_amd.game import PyRat

    st = og.state()
    return PyRat(og.w, og.h, og.cost(), og.cheese_mask(), st["p1"], st["p2"], max_turns, st["turn"], st["p1_score"],
                 st["p2_score"], st["p1_mud"], st["p2_mud"])
