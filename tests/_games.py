"""ctypes driver of tests/hostsim_games: the product's supply of games (alpharat_amd/csrc/host_games.h GameSupply)
compiled for the CPU, one game per call."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent / "hostsim_games"


class GsParams(C.Structure):
    _fields_ = [
        ("width", C.c_uint8), ("height", C.c_uint8), ("cheese_count", C.c_uint16), ("max_turns", C.c_uint16),
        ("cheese_symmetric", C.c_int), ("maze_type", C.c_char_p), ("positions", C.c_char_p),
        ("wall_density", C.c_float), ("mud_density", C.c_float), ("maze_symmetric", C.c_int), ("has_seed", C.c_int),
        ("game_seed_base", C.c_uint64), ("first_game_index", C.c_uint32),
    ]


_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-s", "-C", str(HERE), "libgamessim.so"], check=True)
        L = C.CDLL(str(HERE / "libgamessim.so"))
        L.gs_make_game.restype = C.c_int
        L.gs_make_game.argtypes = [C.POINTER(GsParams), C.c_uint32, C.POINTER(C.c_uint32)] + [C.c_void_p] * 3 + [
            C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
        _lib = L
    return _lib


def make_game(nth, *, width, height, cheese_count, cheese_symmetric=True, maze_type="open", positions="corners",
              wall_density=0.7, mud_density=0.1, maze_symmetric=True, seed=0, first_game_index=0, max_turns=30) -> dict:
    """Game `nth` of the run these arguments describe (those of rust_self_play and play_match): dict(index, p1, p2 (cell
    indices y * width + x), cheese[hw], cost[h, w, 4], generated). Raises ValueError with the library's message."""
    enc = lambda s: None if s is None else str(s).encode()  # noqa: E731
    p = GsParams(width, height, cheese_count, max_turns, int(cheese_symmetric), enc(maze_type), enc(positions), wall_density,
                 mud_density, int(maze_symmetric), 1, seed & 0xFFFFFFFFFFFFFFFF, first_game_index)
    hw = max(width * height, 1)
    index, generated = C.c_uint32(0), C.c_int(0)
    start, cheese, cost = np.zeros(2, np.uint8), np.zeros(hw, np.uint8), np.zeros(hw * 4, np.uint8)
    err = C.create_string_buffer(256)
    rc = lib().gs_make_game(C.byref(p), nth, C.byref(index), start.ctypes.data, cheese.ctypes.data, cost.ctypes.data,
                            C.byref(generated), err, 256)
    if rc != 0:
        raise ValueError(err.value.decode())
    return dict(index=index.value, p1=int(start[0]), p2=int(start[1]), cheese=cheese,
                cost=cost.reshape(height, width, 4), generated=bool(generated.value))
