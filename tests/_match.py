"""Test helpers for head-to-head matches: the match restated on the CPU oracle (tests/_oracle.py), the ctypes driver of
tests/hostsim_match (the product's search headers + dev_match.h compiled for the CPU), and one comparison for both.

A game record here is a dict: n, a_is_p1, final (s1, s2), ints[n, 9] (p1x p1y p2x p2y mud1 mud2 turn a1 a2),
masks[n, hw], and per agent ("a", "b") floats[n, 34] (p1_score p2_score value_p1 value_p2 visit_counts_p1/2 prior_p1/2
policy_p1/2 -- the row layout of the oracle's self-play driver) and counts[n, 4] (total_visits nn_evals terminals
collisions)."""
from __future__ import annotations

import ctypes as C
import subprocess
from dataclasses import dataclass
from pathlib import Path

import numpy as np

import _oracle as O

HERE = Path(__file__).resolve().parent / "hostsim_match"


@dataclass
class Agent:
    """One side as the oracle sees it. backend 0: SmartUniform; 4 with `net` an O.CallbackBackend."""
    cfg: O.OrSearchConfig
    sims: int
    batch: int
    seed: int
    backend: int = 0
    net: object = None


def _row(st, r):
    f = np.zeros(34, np.float32)
    f[0], f[1] = st["p1_score"], st["p2_score"]
    f[2], f[3] = r["value_p1"], r["value_p2"]
    for k, a in (("visit_counts_p1", 4), ("visit_counts_p2", 9), ("prior_p1", 14), ("prior_p2", 19), ("policy_p1", 24),
                 ("policy_p2", 29)):
        f[a:a + 5] = r[k]
    return f, [r[k] for k in ("total_visits", "nn_evals", "terminals", "collisions")]


def oracle_game(og: O.Game, index: int, a: Agent, b: Agent, a_is_p1: bool, only: str | None = None) -> dict:
    """The issue's composition for one game: per turn each agent searches a fresh tree with its own persistent stream,
    then samples the policy of its side from that stream. `only`: search with that agent alone ("a"), the other side
    of the record stays empty and the other agent's action is STAY (used to state that A does not depend on B)."""
    g = og.clone()
    rng = {"a": O.Rng(a.seed + index), "b": O.Rng(b.seed + index)}
    ag = {"a": a, "b": b}
    p1, p2 = ("a", "b") if a_is_p1 else ("b", "a")
    ints, masks = [], []
    fl = {"a": [], "b": []}
    cn = {"a": [], "b": []}
    while not g.over():
        st = g.state()
        res = {}
        for x in ("a", "b"):
            if only is not None and x != only:
                continue
            X = ag[x]
            res[x] = O.Tree(g).search(g, X.cfg, X.sims, X.batch, rng[x], backend=X.backend, net=X.net)
            f, c = _row(st, res[x])
            fl[x].append(f)
            cn[x].append(c)
        act = {}
        for x, key in ((p1, "policy_p1"), (p2, "policy_p2")):
            if x in res:
                d = rng[x].weighted5(res[x][key])
                act[x] = 4 if d < 0 else d
            else:
                act[x] = 4
        ints.append([*st["p1"], *st["p2"], st["p1_mud"], st["p2_mud"], st["turn"], act[p1], act[p2]])
        masks.append(g.cheese_mask())
        g.make_move(act[p1], act[p2])
        if only is not None:
            break  # (a record of the first position is all such a run states)
    st = g.state()
    n = len(ints)
    hw = og.w * og.h
    out = dict(n=n, a_is_p1=bool(a_is_p1), final=(np.float32(st["p1_score"]), np.float32(st["p2_score"])),
               ints=np.array(ints, np.int32).reshape(n, 9), masks=np.array(masks, np.uint8).reshape(n, hw))
    for x in ("a", "b"):
        k = len(fl[x])
        out[x] = dict(floats=np.array(fl[x], np.float32).reshape(k, 34), counts=np.array(cn[x], np.uint32).reshape(k, 4))
    return out


def assert_same_game(got: dict, want: dict, label="") -> None:
    """Bit for bit: positions, both actions, both agents' policies, values, visit counts, priors and counters."""
    assert got["n"] == want["n"], (label, got["n"], want["n"])
    assert got["a_is_p1"] == want["a_is_p1"], label
    np.testing.assert_array_equal(got["ints"], want["ints"], err_msg=f"{label} positions / actions")
    np.testing.assert_array_equal(got["masks"], want["masks"], err_msg=f"{label} cheese")
    for x in ("a", "b"):
        assert got[x]["floats"].tobytes() == want[x]["floats"].tobytes(), (label, x, "search outputs")
        np.testing.assert_array_equal(got[x]["counts"], want[x]["counts"], err_msg=f"{label} agent {x} counters")
    assert np.float32(got["final"][0]).tobytes() == np.float32(want["final"][0]).tobytes(), label
    assert np.float32(got["final"][1]).tobytes() == np.float32(want["final"][1]).tobytes(), label


def from_play_match(rec: dict) -> dict:
    """A record of alpharat_amd.match.play_match(keep_games=True) in the layout above."""
    n = rec["n"]
    ints = np.concatenate([rec["p1_pos"].astype(np.int32), rec["p2_pos"].astype(np.int32),
                           rec["p1_mud"].astype(np.int32)[:, None], rec["p2_mud"].astype(np.int32)[:, None],
                           rec["turn"].astype(np.int32)[:, None], rec["action_p1"].astype(np.int32)[:, None],
                           rec["action_p2"].astype(np.int32)[:, None]], axis=1).reshape(n, 9)
    out = dict(n=n, a_is_p1=rec["a_is_p1"], final=(np.float32(rec["final_p1_score"]), np.float32(rec["final_p2_score"])),
               ints=ints, masks=rec["cheese_mask"])
    for x in ("a", "b"):
        s = rec[x]
        f = np.concatenate([rec["p1_score"][:, None], rec["p2_score"][:, None], s["value_p1"][:, None], s["value_p2"][:, None],
                            s["visit_counts_p1"], s["visit_counts_p2"], s["prior_p1"], s["prior_p2"], s["policy_p1"],
                            s["policy_p2"]], axis=1).astype(np.float32).reshape(n, 34)
        c = np.stack([s["total_visits"], s["nn_evals"], s["terminals"], s["collisions"]], axis=1).astype(np.uint32).reshape(n, 4)
        out[x] = dict(floats=f, counts=c)
    return out


# ---- tests/hostsim_match -------------------------------------------------------------------------------------------
class MsAgent(C.Structure):
    _fields_ = [
        ("c_puct", C.c_float), ("fpu_reduction", C.c_float), ("force_k", C.c_float), ("noise_epsilon", C.c_float),
        ("noise_concentration", C.c_float), ("coll_min", C.c_uint32), ("coll_max", C.c_uint32), ("coll_start", C.c_uint32),
        ("coll_end", C.c_uint32), ("coll_power", C.c_float), ("n_sims", C.c_uint32), ("batch", C.c_uint32),
        ("evaluator", C.c_uint32), ("gather_rounds", C.c_uint32), ("arena_nodes", C.c_uint32), ("seed_base", C.c_uint64),
    ]


class MsGame(C.Structure):
    _fields_ = [
        ("width", C.c_uint8), ("height", C.c_uint8), ("max_turns", C.c_uint16), ("p1_x", C.c_uint8), ("p1_y", C.c_uint8),
        ("p2_x", C.c_uint8), ("p2_y", C.c_uint8), ("game_index", C.c_uint32), ("cost", C.c_void_p), ("cheese", C.c_void_p),
    ]


_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-s", "-C", str(HERE)], check=True)
        L = C.CDLL(str(HERE / "libmatchsim.so"))
        L.ms_run.restype = C.c_void_p
        L.ms_run.argtypes = [C.POINTER(MsGame), C.c_uint32, C.POINTER(MsAgent), C.POINTER(MsAgent), C.c_int, C.c_uint32,
                             C.c_uint32]
        L.ms_free.argtypes = [C.c_void_p]
        L.ms_header.restype = None
        L.ms_header.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 3
        L.ms_positions.restype = None
        L.ms_positions.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 6
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def ms_agent(a: Agent, evaluator=0, gather_rounds=0, arena_nodes=0) -> MsAgent:
    c = a.cfg
    return MsAgent(c.c_puct, c.fpu_reduction, c.force_k, c.noise_epsilon, c.noise_concentration, c.collision_limit_min,
                   c.collision_limit_max, c.collision_scaling_start, c.collision_scaling_end, c.collision_scaling_power,
                   a.sims, a.batch, evaluator, gather_rounds, arena_nodes, a.seed)


def hostsim_match(ogs, indices, max_turns, a: MsAgent, b: MsAgent, swap_sides=True, resident=4, visit_every=3):
    """Play the games `ogs` (oracle Games at their start positions, with global indices `indices`) as one match on the
    CPU harness. Returns (records in game order, dict(ticks, grows_a, grows_b))."""
    L = lib()
    keep = []
    arr = (MsGame * len(ogs))()
    for k, (og, idx) in enumerate(zip(ogs, indices)):
        maze = og.maze().reshape(-1).astype(np.int16)
        cost = np.ascontiguousarray(np.where(maze < 0, 0, maze).astype(np.uint8))
        cheese = np.ascontiguousarray(og.cheese_mask().astype(np.uint8))
        keep += [cost, cheese]
        st = og.state()
        arr[k] = MsGame(og.w, og.h, max_turns, st["p1"][0], st["p1"][1], st["p2"][0], st["p2"][1], idx, _p(cost), _p(cheese))
    h = L.ms_run(arr, len(ogs), C.byref(a), C.byref(b), int(swap_sides), resident, visit_every)
    try:
        recs = []
        totals = np.zeros(3, np.uint64)
        for k, og in enumerate(ogs):
            hdr = np.zeros(4, np.uint32)
            fs = np.zeros(2, np.float32)
            L.ms_header(h, k, _p(hdr), _p(fs), _p(totals))
            assert hdr[2] == 0, "bug guard set"
            n, hw = int(hdr[0]), og.w * og.h
            ints = np.zeros((n, 9), np.int32)
            fa, fb = np.zeros((n, 34), np.float32), np.zeros((n, 34), np.float32)
            ca, cb = np.zeros((n, 4), np.uint32), np.zeros((n, 4), np.uint32)
            masks = np.zeros((n, hw), np.uint8)
            L.ms_positions(h, k, og.w, hw, _p(ints), _p(fa), _p(fb), _p(ca), _p(cb), _p(masks))
            recs.append(dict(n=n, a_is_p1=bool(hdr[1]), final=(fs[0], fs[1]), ints=ints, masks=masks,
                             a=dict(floats=fa, counts=ca), b=dict(floats=fb, counts=cb), game_index=int(hdr[3])))
        return recs, dict(ticks=int(totals[0]), grows_a=int(totals[1]), grows_b=int(totals[2]))
    finally:
        L.ms_free(h)
