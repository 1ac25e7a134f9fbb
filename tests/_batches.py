"""Games and the driver of tests/hostsim_batches for the batch tests -- test infrastructure only.

A game is the record dict of tests/_rows.py. The driver hands the harness output arrays with guard rows of 0x5A on both
sides of the rows it may write, and checks them.
"""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import _oracle as O
import _rows as T
import _rows_np as R

HERE = Path(__file__).resolve().parent / "hostsim_batches"
GUARD = 3  # rows in front of and behind the rows that are written

# the boards of tests/test_rows_logic_cpu.py and one of 72 cells, whose cheese bits cross a 64-bit word
BOARDS = T.BOARDS + [("9x8", 9, 8, 30, 12, None, 2, 24)]


def capture_game() -> dict:
    """5x5: both players step onto the cheese at (2, 2) in the first move (outcome 1); P1 then walks two cells up or down
    its column and takes the cheese at one end alone (outcome 0) while the one at the other end stays (outcome 2), and P2
    takes (4, 2) alone (outcome 3). Positions after the first show -1 at (2, 2)."""
    og = O.Game(5, 5, 4, p1=(1, 2), p2=(3, 2), cheese=[(2, 2), (2, 4), (2, 0), (4, 2)])
    return T.scripted(og, [(1, 3), (0, 1), (0, 1), (4, 4)], index=3)


def mud_game() -> dict:
    """7x5 with mud, played by the oracle: the two players' mud timers differ in some position."""
    og = O.Game(7, 5, 30)
    og.random_maze(0.3, 0.6, False, 5)
    og.random_cheese(7, True, 105)
    return T.played(og, 1, 24)


def open_game() -> dict:
    """5x5 open, played by the oracle: the first position has score difference 0."""
    return T.board_games(*T.BOARDS[0][:6], 1, 24)[0]


def with_guards(n: int, w: int, h: int) -> tuple[dict, dict]:
    """(whole arrays of n + 2 * GUARD rows preset to 0x5A, views of their n middle rows)"""
    whole = T.empty_rows(n + 2 * GUARD, w, h)
    return whole, {k: whole[k][GUARD:GUARD + n] for k in R.KEYS}


def assert_guards_intact(whole: dict, n: int, what="") -> None:
    for k in R.KEYS:
        for part in (whole[k][:GUARD], whole[k][GUARD + n:]):
            assert (part.view(np.uint8) == 0x5A).all(), f"{what}: {k} written outside its {n} rows"


_sim = None


def sim() -> C.CDLL:
    global _sim
    if _sim is None:
        subprocess.run(["make", "-s", "-C", str(HERE)], check=True)
        L = C.CDLL(str(HERE / "libbatchessim.so"))
        L.bs_build.restype = C.c_int
        L.bs_build.argtypes = [C.POINTER(T.RsGame), C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int] + [C.c_void_p] * 8
        L.bs_record_bytes.restype = C.c_uint32
        L.bs_record_bytes.argtypes = [C.c_uint32]
        _sim = L
    return _sim


def sim_batch(games, rows, swap=None, reverse=False) -> dict:
    """rows_build_row_as over `rows` (swap: one flag per row, or None), written between guard rows that are checked here."""
    keep: list = []
    gs = (T.RsGame * len(games))(*[T._rs_game(g, keep) for g in games])
    rows = np.ascontiguousarray(rows, np.uint64)
    swap_p = None
    if swap is not None:
        swap = np.ascontiguousarray(swap, np.uint8)
        assert len(swap) == len(rows)
        swap_p = swap.ctypes.data
    n = len(rows)
    whole, out = with_guards(n, games[0]["width"], games[0]["height"])
    rc = sim().bs_build(gs, len(games), rows.ctypes.data, swap_p, n, int(reverse), *[out[k].ctypes.data for k in R.KEYS])
    assert rc == 0, rc
    assert_guards_intact(whole, n, "hostsim_batches")
    return {k: out[k].copy() for k in R.KEYS}
