"""Test helpers for match agents that do not search and for the sampling temperature: the semantics restated in Python
(greedy: heapq on O.Game.cost(); random: O.Rng.gen_range(5); temperature: numpy f64 and O.Rng.weighted5), the match
composition of tests/_match.py oracle_game extended to every agent kind, and the ctypes driver of tests/hostsim_agents
(alpharat_amd/csrc/dev_agents.h compiled for the CPU on top of the slot sets of tests/hostsim_match).

Game records have the layout of tests/_match.py; the rows of an agent that does not search are all zero."""
from __future__ import annotations

import ctypes as C
import heapq
import subprocess
from dataclasses import dataclass
from pathlib import Path

import numpy as np

import _match as M
import _oracle as O

HERE = Path(__file__).resolve().parent / "hostsim_agents"
SEARCH, RANDOM, GREEDY = 0, 1, 2
STAY = 4


@dataclass
class Agent:
    """One side: kind SEARCH with `search` an M.Agent (and a temperature), or RANDOM (its stream base `seed`), or GREEDY."""
    kind: int = SEARCH
    search: M.Agent | None = None
    temperature: float = 1.0
    seed: int = 0

    @property
    def stream_base(self) -> int:
        return self.search.seed if self.kind == SEARCH else self.seed


# ---- the semantics, restated -------------------------------------------------------------------------------------------
def neighbour(cell: int, d: int, w: int) -> int:
    """st_step's geometry: UP is y + 1 (cell index + width), RIGHT x + 1, DOWN y - 1, LEFT x - 1."""
    return cell + (w, 1, -w, -1)[d]


def greedy_search(cost: np.ndarray, cheese: np.ndarray, start: int, w: int):
    """Dijkstra from `start` with a heap ordered by (cost, push counter); directions tried 0, 1, 2, 3; a cost of 0 is a
    wall or the board edge. Returns (move, cheese cell or -1, its distance, whether the chosen path has an edge of cost
    >= 2)."""
    cost = np.asarray(cost, np.uint8).reshape(-1)
    INF = 1 << 30
    dist = {start: 0}
    first = {start: None}
    muddy = {start: False}  # (not part of the semantics: the test's own input analysis)
    counter = 0
    heap = [(0, 0, start)]
    while heap:
        c, _, cell = heapq.heappop(heap)
        if c > dist.get(cell, INF):
            continue
        if cheese[cell]:
            return (STAY if cell == start else first[cell]), cell, c, muddy[cell]
        for d in range(4):
            wt = int(cost[cell * 4 + d])
            if wt == 0:
                continue
            nb = neighbour(cell, d, w)
            nc = c + wt
            if nc < dist.get(nb, INF):
                dist[nb] = nc
                first[nb] = d if cell == start else first[cell]
                muddy[nb] = muddy[cell] or wt >= 2
                counter += 1
                heapq.heappush(heap, (nc, counter, nb))
    return STAY, -1, -1, False


def greedy_move(cost, cheese, start: int, w: int) -> int:
    return greedy_search(cost, cheese, start, w)[0]


def all_distances(cost: np.ndarray, start: int, w: int, hw: int) -> np.ndarray:
    """Plain Dijkstra distances from `start` to every cell (test-input analysis only)."""
    cost = np.asarray(cost, np.uint8).reshape(-1)
    INF = 1 << 30
    dist = np.full(hw, INF, np.int64)
    dist[start] = 0
    heap = [(0, start)]
    while heap:
        c, cell = heapq.heappop(heap)
        if c > dist[cell]:
            continue
        for d in range(4):
            wt = int(cost[cell * 4 + d])
            if wt:
                nb = neighbour(cell, d, w)
                if c + wt < dist[nb]:
                    dist[nb] = c + wt
                    heapq.heappush(heap, (c + wt, nb))
    return dist


def optimal_first_moves(cost: np.ndarray, cheese: np.ndarray, start: int, w: int, distances=None) -> set:
    """Every first move of a minimum-cost path from `start` to a minimum-cost cheese (test-input analysis only).
    `distances(cell)`: all_distances from that cell, for callers that share them between the positions of a maze."""
    cost = np.asarray(cost, np.uint8).reshape(-1)
    hw = len(cheese)
    if distances is None:
        def distances(c):
            return all_distances(cost, c, w, hw)
    from_start = distances(start)
    targets = [c for c in np.flatnonzero(cheese) if from_start[c] < (1 << 30)]
    if not targets:
        return set()
    best = min(from_start[c] for c in targets)
    if best == 0:
        return {STAY}
    moves = set()
    for d in range(4):
        wt = int(cost[start * 4 + d])
        if wt == 0:
            continue
        rest = distances(neighbour(start, d, w))
        if any(from_start[c] == best and wt + rest[c] == best for c in targets):
            moves.add(d)
    return moves


def random_move(rng: O.Rng) -> int:
    return int(rng.gen_range(5))


def tempered_weights(policy, temperature: float) -> np.ndarray:
    p = np.asarray(policy, np.float32).astype(np.float64)
    q = np.exp(np.log(p + 1e-10) / np.float64(temperature))
    total = np.float64(0.0)
    for v in q:  # (sums in index order)
        total = total + v
    return (q / total).astype(np.float32)


def sample(rng: O.Rng, policy, temperature: float) -> int:
    """ai/utils.py:26-40 on an f32 policy; an all-zero policy is STAY at every temperature and draws nothing."""
    policy = np.asarray(policy, np.float32)
    if temperature == 1.0:
        d = rng.weighted5(policy)
        return STAY if d < 0 else int(d)
    if not policy.any():
        return STAY
    if temperature == 0.0:
        return int(np.argmax(policy))  # (the first index of the largest entry)
    d = rng.weighted5(tempered_weights(policy, temperature))
    return STAY if d < 0 else int(d)


def game_cost(og: O.Game) -> np.ndarray:
    return np.ascontiguousarray(og.cost().reshape(-1).astype(np.uint8))


def oracle_game(og: O.Game, index: int, a: Agent, b: Agent, a_is_p1: bool, only: str | None = None) -> dict:
    """tests/_match.py oracle_game for any pair of agent kinds: per turn each agent moves from the same position -- a
    search on a fresh tree with its own persistent stream and then one sample at its temperature, or one draw from its
    stream, or the greedy move -- at every turn, in mud or not. `only`: as in tests/_match.py."""
    g = og.clone()
    cost = game_cost(og)
    ag = {"a": a, "b": b}
    rng = {x: O.Rng(ag[x].stream_base + index) for x in ("a", "b")}
    p1, p2 = ("a", "b") if a_is_p1 else ("b", "a")
    ints, masks = [], []
    fl = {"a": [], "b": []}
    cn = {"a": [], "b": []}
    while not g.over():
        st = g.state()
        cheese = g.cheese_mask()
        act = {}
        for x, key, who in ((p1, "policy_p1", "p1"), (p2, "policy_p2", "p2")):
            X = ag[x]
            if only is not None and x != only:
                act[x] = STAY
                continue
            if X.kind == SEARCH:
                S = X.search
                res = O.Tree(g).search(g, S.cfg, S.sims, S.batch, rng[x], backend=S.backend, net=S.net)
                f, c = M._row(st, res)
                act[x] = sample(rng[x], res[key], X.temperature)
            else:
                f = np.zeros(34, np.float32)
                f[0], f[1] = st["p1_score"], st["p2_score"]
                c = [0, 0, 0, 0]
                if X.kind == RANDOM:
                    act[x] = random_move(rng[x])
                else:
                    act[x] = greedy_move(cost, cheese, st[who][1] * og.w + st[who][0], og.w)
            fl[x].append(f)
            cn[x].append(c)
        ints.append([*st["p1"], *st["p2"], st["p1_mud"], st["p2_mud"], st["turn"], act[p1], act[p2]])
        masks.append(cheese)
        g.make_move(act[p1], act[p2])
        if only is not None:
            break
    st = g.state()
    n = len(ints)
    out = dict(n=n, a_is_p1=bool(a_is_p1), final=(np.float32(st["p1_score"]), np.float32(st["p2_score"])),
               ints=np.array(ints, np.int32).reshape(n, 9), masks=np.array(masks, np.uint8).reshape(n, og.w * og.h))
    for x in ("a", "b"):
        k = len(fl[x])
        out[x] = dict(floats=np.array(fl[x], np.float32).reshape(k, 34), counts=np.array(cn[x], np.uint32).reshape(k, 4))
    return out


# ---- tests/hostsim_agents ----------------------------------------------------------------------------------------------
class AsAgent(C.Structure):
    _fields_ = [("search", M.MsAgent), ("kind", C.c_uint32), ("temperature", C.c_float)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.run(["make", "-s", "-C", str(HERE)], check=True)
        L = C.CDLL(str(HERE / "libagentssim.so"))
        L.as_greedy.restype = C.c_uint32
        L.as_greedy.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]
        L.as_sample.restype = C.c_uint32
        L.as_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_float]
        L.as_match_sample.restype = C.c_uint32
        L.as_match_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.as_random_move.restype = C.c_uint32
        L.as_random_move.argtypes = [C.c_void_p]
        L.as_run.restype = C.c_void_p
        L.as_run.argtypes = [C.POINTER(M.MsGame), C.c_uint32, C.POINTER(AsAgent), C.POINTER(AsAgent), C.c_int, C.c_uint32,
                             C.c_uint32]
        L.ms_free.argtypes = [C.c_void_p]
        L.ms_header.restype = None
        L.ms_header.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 3
        L.ms_positions.restype = None
        L.ms_positions.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 6
        _lib = L
    return _lib


_p = M._p


def hostsim_greedy(w: int, h: int, cost: np.ndarray, cheese: np.ndarray, start: int, reverse: bool = False):
    """The lane phases of k_match_greedy on the CPU. Returns (move, bound hit, levels run)."""
    out = np.zeros(2, np.uint32)
    cost = np.ascontiguousarray(cost, np.uint8)
    cheese = np.ascontiguousarray(cheese, np.uint8)
    mv = lib().as_greedy(w, h, _p(cost), _p(cheese), start, int(reverse), _p(out))
    return int(mv), bool(out[0]), int(out[1])


def hostsim_sample(state: np.ndarray, policy, temperature: float) -> int:
    policy = np.ascontiguousarray(policy, np.float32)
    return int(lib().as_sample(_p(state), _p(policy), temperature))


def hostsim_match_sample(state: np.ndarray, policy, player: int) -> int:
    policy = np.ascontiguousarray(policy, np.float32)
    return int(lib().as_match_sample(_p(state), _p(policy), player))


def as_agent(a: Agent, **search_kw) -> AsAgent:
    if a.kind == SEARCH:
        return AsAgent(M.ms_agent(a.search, **search_kw), SEARCH, a.temperature)
    ms = M.MsAgent()
    ms.seed_base = a.seed
    ms.batch = 1
    return AsAgent(ms, a.kind, 1.0)


def hostsim_match(ogs, indices, max_turns, a: AsAgent, b: AsAgent, swap_sides=True, resident=4, visit_every=3):
    """tests/_match.py hostsim_match through as_run: any pair of agent kinds. Returns (records in game order, ticks)."""
    L = lib()
    keep = []
    arr = (M.MsGame * len(ogs))()
    for k, (og, idx) in enumerate(zip(ogs, indices)):
        cost = game_cost(og)
        cheese = np.ascontiguousarray(og.cheese_mask().astype(np.uint8))
        keep += [cost, cheese]
        st = og.state()
        arr[k] = M.MsGame(og.w, og.h, max_turns, st["p1"][0], st["p1"][1], st["p2"][0], st["p2"][1], idx, _p(cost), _p(cheese))
    h = L.as_run(arr, len(ogs), C.byref(a), C.byref(b), int(swap_sides), resident, visit_every)
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
        return recs, int(totals[0])
    finally:
        L.ms_free(h)
