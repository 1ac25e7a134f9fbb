"""Match agents on the CPU: the lane phases of k_match_greedy, the temperature sample and the move of any pair of agent
kinds (alpharat_amd/csrc/dev_agents.h, compiled for the CPU by tests/hostsim_agents) against their semantics restated in
Python (tests/_agents.py); then the C-ABI fields, the refusals and the Python constructors. Bar: equal, move for move and
bit for bit."""
import dataclasses
import re
from pathlib import Path

import numpy as np
import pytest

import _agents as A
import _match as M
import _oracle as O

ROOT = Path(__file__).resolve().parent.parent
SEED_A, SEED_B = 0xA0000, 0xB0000


# ---- 1. greedy ---------------------------------------------------------------------------------------------------------
# (name, width, height, walls and mud: None = open, else (wall_density, mud_density), positions per maze and cheese count).
# The generator's defaults (0.7, 0.1) give mazes that are close to trees, and mud of many costs breaks ties: the ties are
# on the open boards (the large ones have the widest levels) and behind sparse walls, the mud on the paths of the muddy mazes.
BOARDS = [
    ("5x5 open", 5, 5, None, 60), ("7x7 open", 7, 7, None, 60), ("11x9 open", 11, 9, None, 60), ("15x11 open", 15, 11, None, 60),
    ("5x5 default", 5, 5, (0.7, 0.1), 15), ("7x7 default", 7, 7, (0.7, 0.1), 15),
    ("5x5 muddy", 5, 5, (0.25, 0.5), 15), ("7x7 muddy", 7, 7, (0.25, 0.5), 15),
    ("7x7 sparse walls", 7, 7, (0.3, 0.0), 30), ("15x11 sparse walls", 15, 11, (0.3, 0.0), 30),
    ("11x9 muddy", 11, 9, (0.3, 0.4), 15), ("15x11 muddy", 15, 11, (0.3, 0.4), 15),
]
CHEESE_COUNTS = (1, 2, 5, 20)
MAZES_PER_BOARD = 3


def _maze(w, h, spec, seed):
    g = O.Game(w, h, 100)
    if spec is not None:
        g.random_maze(spec[0], spec[1], True, seed)
    return A.game_cost(g)


def _greedy_positions():
    """(label, w, h, cost, cheese, start, player is in mud)"""
    rng = np.random.default_rng(20240607)
    for name, w, h, spec, per_case in BOARDS:
        for m in range(MAZES_PER_BOARD):
            cost = _maze(w, h, spec, 100 + m)
            for n_cheese in CHEESE_COUNTS:
                for k in range(per_case):
                    cheese = np.zeros(w * h, np.uint8)
                    cheese[rng.choice(w * h, size=n_cheese, replace=False)] = 1
                    yield f"{name} maze {m} cheese {n_cheese} #{k}", w, h, cost, cheese, int(rng.integers(w * h)), False
    # positions of games in progress on a muddy maze: players stuck in mud still get a move
    for seed in (1,):
        g = O.Game(7, 7, 60).random_maze(0.7, 0.6, True, seed).random_cheese(9, True, seed)
        cost = A.game_cost(g)
        while not g.over():
            st = g.state()
            cheese = g.cheese_mask().copy()
            for who, mud in (("p1", "p1_mud"), ("p2", "p2_mud")):
                yield f"7x7 game {seed} turn {st['turn']} {who}", 7, 7, cost, cheese, st[who][1] * 7 + st[who][0], st[mud] > 0
            g.make_move(int(rng.integers(4)), int(rng.integers(4)))
    # walls around the corner cell (0, 0): its cheese cannot be reached; a player inside reaches nothing
    g = O.Game(5, 5, 100, walls=[((0, 0), (1, 0)), ((0, 0), (0, 1))])
    cost = A.game_cost(g)
    corner = np.zeros(25, np.uint8)
    corner[0] = 1
    far = np.zeros(25, np.uint8)
    far[24] = 1
    yield "walled corner, cheese inside", 5, 5, cost, corner, 12, False
    yield "walled corner, player inside", 5, 5, cost, far, 0, False
    yield "no cheese at all", 5, 5, cost, np.zeros(25, np.uint8), 7, False


def test_greedy_lane_phases_equal_the_heap_move_for_move():
    total = ties = muddy = unreachable = on_cheese = in_mud = 0
    dist_cache = {}
    for label, w, h, cost, cheese, start, stuck in _greedy_positions():
        want, cell, _dist, crosses_mud = A.greedy_search(cost, cheese, start, w)
        for reverse in (False, True):  # (no phase may depend on the order the lanes run in)
            got, bound_hit, levels = A.hostsim_greedy(w, h, cost, cheese, start, reverse)
            assert not bound_hit and levels <= w * h, label
            assert got == want, (label, start, got, want)
        # what the restatement alone says about this input
        total += 1
        key = (cost.tobytes(), w)
        cache = dist_cache.setdefault(key, {})

        def distances(c, cache=cache, cost=cost, w=w, h=h):
            if c not in cache:
                cache[c] = A.all_distances(cost, c, w, w * h)
            return cache[c]

        ties += len(A.optimal_first_moves(cost, cheese, start, w, distances)) >= 2
        muddy += bool(crosses_mud)
        unreachable += cell < 0 and want == A.STAY
        on_cheese += bool(cheese[start]) and want == A.STAY
        in_mud += bool(stuck)
    assert total >= 2500
    assert ties * 3 >= total, (ties, total)
    assert muddy * 10 >= total, (muddy, total)
    assert unreachable >= 1 and on_cheese >= 1 and in_mud >= 1, (unreachable, on_cheese, in_mud)


def test_the_greedy_move_is_one_of_the_optimal_first_moves():
    cost = _maze(7, 7, (0.25, 0.5), 100)
    cheese = np.zeros(49, np.uint8)
    cheese[[3, 30, 44]] = 1
    for start in range(49):
        assert A.greedy_move(cost, cheese, start, 7) in A.optimal_first_moves(cost, cheese, start, 7)


# ---- 2. temperature ----------------------------------------------------------------------------------------------------
POLICIES = [
    [0.1, 0.2, 0.3, 0.25, 0.15], [0.0, 0.5, 0.0, 0.5, 0.0], [0.0, 0.0, 1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0, 0.0],
    [0.0, 0.0, 0.0, 0.0, 1.0], [0.3, 0.3, 0.3, 0.05, 0.05], [0.0, 0.4, 0.2, 0.4, 0.0], [0.2, 0.2, 0.2, 0.2, 0.2],
    [0.0, 0.0, 0.0, 0.0, 0.0], [0.7, 0.0, 0.1, 0.0, 0.2], [1e-6, 0.999999, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.5, 0.5],
]


@pytest.mark.parametrize("temperature", [0.0, 1.0, 0.5, 2.0])
def test_temperature_sample_equals_the_restatement(temperature):
    gen = np.random.default_rng(7)
    policies = [np.array(p, np.float32) for p in POLICIES]
    for _ in range(40):  # policies as a search returns them: visit shares with zeros
        v = gen.integers(0, 30, 5) * (gen.random(5) < 0.7)
        if v.sum() > 0:
            policies.append((v / v.sum()).astype(np.float32))
    for k, pol in enumerate(policies):
        want_rng, got = O.Rng(1000 + k), O.Rng(1000 + k)
        for draw in range(25):
            before = got.s.copy()
            want = A.sample(want_rng, pol, temperature)
            action = A.hostsim_sample(got.s, pol, temperature)
            assert action == want, (k, draw, pol, temperature)
            assert np.array_equal(got.s, want_rng.s), (k, draw)
            if temperature == 0.0 or not pol.any():
                assert np.array_equal(got.s, before)  # no draw
                assert action == (A.STAY if not pol.any() else int(np.argmax(pol)))
            else:
                assert not np.array_equal(got.s, before)
            if temperature == 1.0:  # today's match_sample: the same action from the same stream, left in the same state
                for player in (0, 1):
                    s = before.copy()
                    assert A.hostsim_match_sample(s, pol, player) == action
                    assert np.array_equal(s, got.s)


def test_tempered_weights_sharpen_and_flatten():
    p = np.array([0.1, 0.2, 0.3, 0.25, 0.15], np.float32)
    sharp, flat = A.tempered_weights(p, 0.5), A.tempered_weights(p, 2.0)
    assert sharp.dtype == np.float32 and sharp.max() > p.max() > flat.max()
    np.testing.assert_allclose(sharp, (p.astype(np.float64) ** 2 / (p.astype(np.float64) ** 2).sum()), rtol=1e-6)


def test_random_agent_draw_is_gen_range_5():
    want, got = O.Rng(5), O.Rng(5)
    for _ in range(200):
        assert A.lib().as_random_move(M._p(got.s)) == A.random_move(want)
        assert np.array_equal(got.s, want.s)


# ---- 3. whole matches --------------------------------------------------------------------------------------------------
GREEDY = A.Agent(A.GREEDY)
RANDOM = A.Agent(A.RANDOM, seed=SEED_B)
IDX = list(range(12))


def _search_agent(seed=SEED_A, temperature=1.0):
    return A.Agent(A.SEARCH, M.Agent(O.make_config(), 32, 8, seed), temperature)


def _games():
    return [O.Game(5, 5, 30).random_cheese(5, True, i) for i in IDX]


def _play_and_compare(a, b, ogs=None, idx=IDX, max_turns=30, swap=True, resident=4):
    ogs = ogs if ogs is not None else _games()
    got, ticks = A.hostsim_match(ogs, idx, max_turns, A.as_agent(a), A.as_agent(b), swap_sides=swap, resident=resident)
    for k, (i, og) in enumerate(zip(idx, ogs)):
        want = A.oracle_game(og, i, a, b, a_is_p1=(i % 2 == 0) or not swap)
        M.assert_same_game(got[k], want, f"game {i}")
    return got, ticks


def _rows_are_zero(side):
    return not side["floats"][:, 2:].any() and not side["counts"].any()


def test_greedy_against_random():
    got, ticks = _play_and_compare(GREEDY, RANDOM)
    assert {g["a_is_p1"] for g in got} == {True, False}
    assert all(_rows_are_zero(g["a"]) and _rows_are_zero(g["b"]) for g in got)
    # no agent searches: one move per tick for every resident game (12 games on 4 slots: refills happened)
    assert ticks >= max(g["n"] for g in got) and sum(g["n"] for g in got) <= 4 * ticks
    # greedy plays better than random
    assert sum(g["final"][0] if g["a_is_p1"] else g["final"][1] for g in got) > sum(
        g["final"][1] if g["a_is_p1"] else g["final"][0] for g in got)


def test_random_against_search():
    got, _ = _play_and_compare(A.Agent(A.RANDOM, seed=SEED_B), _search_agent())
    assert all(_rows_are_zero(g["a"]) and g["b"]["counts"][:, 0].all() for g in got)


def test_greedy_against_search_with_swapped_sides():
    got, _ = _play_and_compare(GREEDY, _search_agent(), swap=True)
    assert {g["a_is_p1"] for g in got} == {True, False}
    got, _ = _play_and_compare(_search_agent(), GREEDY, swap=True)
    assert all(_rows_are_zero(g["b"]) for g in got)


@pytest.mark.parametrize("temperature", [0.0, 0.5])
def test_search_with_a_temperature_against_greedy(temperature):
    _play_and_compare(_search_agent(temperature=temperature), GREEDY)


def test_two_search_agents_at_temperature_one_equal_todays_match():
    a, b = _search_agent(SEED_A), _search_agent(SEED_B)
    ogs = _games()[:4]
    got, _ = A.hostsim_match(ogs, IDX[:4], 30, A.as_agent(a), A.as_agent(b), resident=2)
    today, _ = M.hostsim_match(ogs, IDX[:4], 30, M.ms_agent(a.search), M.ms_agent(b.search), resident=2)
    for k in range(4):
        M.assert_same_game(got[k], today[k], f"game {k}")


def test_muddy_maze_above_64_cells_greedy_against_greedy_and_random():
    idx = [0, 1, 2]
    ogs = [O.Game(11, 9, 40).random_maze(0.7, 0.4, True, i).random_cheese(11, True, i) for i in idx]
    got, _ = _play_and_compare(GREEDY, RANDOM, ogs=ogs, idx=idx, max_turns=40, resident=2)
    assert any(g["ints"][:, 4:6].any() for g in got)  # somebody was stuck in mud, and a move was recorded there
    _play_and_compare(GREEDY, A.Agent(A.GREEDY), ogs=ogs, idx=idx, max_turns=40, resident=3)


def test_agent_a_does_not_depend_on_bs_kind_or_seed():
    a = _search_agent()
    ogs = _games()[:3]
    runs = []
    for b in (RANDOM, A.Agent(A.RANDOM, seed=SEED_B + 977), GREEDY, _search_agent(SEED_B)):
        got, _ = _play_and_compare(a, b, ogs=ogs, idx=IDX[:3], swap=False, resident=3)
        runs.append(got)
    for k, og in enumerate(ogs):
        alone = A.oracle_game(og, k, a, a, a_is_p1=True, only="a")
        for got in runs:
            assert got[k]["a"]["floats"][0].tobytes() == alone["a"]["floats"][0].tobytes(), k
            np.testing.assert_array_equal(got[k]["a"]["counts"][0], alone["a"]["counts"][0])
            assert got[k]["ints"][0, 7] == alone["ints"][0, 7]  # A's first action (A is P1)
    assert any(not np.array_equal(runs[0][k]["ints"], runs[1][k]["ints"]) for k in range(3))  # B's seed did change B
    # and the greedy agent needs no stream: its games do not depend on a seed
    g1, _ = A.hostsim_match(ogs, IDX[:3], 30, A.as_agent(GREEDY), A.as_agent(A.Agent(A.GREEDY, seed=99)), resident=3)
    g2, _ = A.hostsim_match(ogs, IDX[:3], 30, A.as_agent(A.Agent(A.GREEDY, seed=5)), A.as_agent(GREEDY), resident=1)
    for k in range(3):
        M.assert_same_game(g1[k], g2[k], f"game {k}")


# ---- 4. ABI and Python -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from alpharat_amd import _lib

    return _lib.load()


def test_header_and_ctypes_mirror_agree_on_the_new_fields(lib):
    from alpharat_amd import _lib

    header = (ROOT / "include" / "alpharat_hip.h").read_text()
    body = re.search(r"typedef struct ArMatchAgent \{(.*?)\} ArMatchAgent;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [s.strip() for s in body.split(";") if s.strip()]
    assert decl[-2:] == ["uint32_t kind", "float temperature"] and decl[-3] == "uint64_t rng_seed_base"
    import ctypes as C

    assert _lib.ArMatchAgent._fields_[-2:] == [("kind", C.c_uint32), ("temperature", C.c_float)]
    for name, value in (("AR_AGENT_SEARCH", 0), ("AR_AGENT_RANDOM", 1), ("AR_AGENT_GREEDY", 2)):
        assert re.search(r"\b%s = %d\b" % (name, value), header) and getattr(_lib, name) == value


GAME = dict(width=5, height=5, cheese_count=5, max_turns=30, num_games=2)


def test_refusals_name_the_field(lib):
    from alpharat_amd.match import MatchAgent, play_match

    with pytest.raises(ValueError, match="kind"):
        play_match(MatchAgent("a", kind="minimax"), MatchAgent("b"), **GAME)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            play_match(MatchAgent("a"), MatchAgent("b", temperature=bad), **GAME)
    gold = ROOT / "tests" / "golden" / "nets" / "mlp_5x5_h32.arnet"
    for kind in ("random", "greedy"):
        with pytest.raises(ValueError, match="weights_path"):
            play_match(MatchAgent("a"), MatchAgent("b", kind=kind, checkpoint=gold), **GAME)
    # the library itself refuses a kind it does not know (the Python layer never passes one on)
    import ctypes as C

    from alpharat_amd import _lib

    def params(a, b):
        return _lib.ArMatchParams(5, 5, 5, 30, 1, b"open", b"corners", 0.7, 0.1, 1, 2, 0, 1, 0, 1, 0, b"auto", 0, a, b)

    ok = MatchAgent("x")._c()
    bad = MatchAgent("y")._c()
    bad.kind = 7
    out = _lib.ArMatchStats()
    with pytest.raises(ValueError, match="kind"):
        _lib.check(lib.ar_match_run(C.byref(params(ok, bad)), _lib.ArMatchSink(), None, C.byref(out)))
    # simulations, batch_size and search of an agent that does not search are not validated
    import torch

    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no HIP device|hipGetDeviceCount"):
            play_match(MatchAgent("r", kind="random", simulations=0, batch_size=0, c_puct=-1.0), MatchAgent.greedy(), **GAME)


def test_match_agent_defaults_and_constructors():
    import alpharat_amd
    from alpharat_amd import _lib
    from alpharat_amd.match import MatchAgent, play_round_robin, standard_agents

    assert alpharat_amd.standard_agents is standard_agents and alpharat_amd.play_round_robin is play_round_robin
    x = MatchAgent("x")
    assert (x.kind, x.temperature) == ("search", 1.0)
    c = x._c()
    assert (c.kind, c.temperature) == (_lib.AR_AGENT_SEARCH, 1.0)
    r, g = MatchAgent.random(seed=9), MatchAgent.greedy()
    assert (r.name, r.kind, r.seed, r.checkpoint) == ("random", "random", 9, None) and r._c().kind == _lib.AR_AGENT_RANDOM
    assert (g.name, g.kind, g.checkpoint) == ("greedy", "greedy", None) and g._c().kind == _lib.AR_AGENT_GREEDY
    n = MatchAgent.nn("net.arnet", seed=3)
    assert (n.kind, n.temperature, n.simulations, n.batch_size, n.noise_epsilon, n.seed) == ("search", 0.0, 1, 1, 0.0, 3)
    assert MatchAgent.nn("net.arnet", temperature=0.5, name="policy").temperature == 0.5

    class Cfg:
        simulations, batch_size, c_puct, force_k, fpu_reduction = 500, 16, 0.512, 0.103, 0.459
        noise_epsilon, noise_concentration = 0.25, 10.83
        collision_limit_min, collision_limit_max, collision_scaling_start, collision_scaling_end = 1, 256, 800, 50000
        collision_scaling_power = 1.0

    assert MatchAgent.from_config(Cfg).temperature == 1.0
    std = standard_agents("new.arnet", Cfg, seed=11)
    assert list(std) == ["random", "greedy", "mcts", "nn", "mcts+nn"]
    both = standard_agents("new.arnet", Cfg, baseline_checkpoint="old.arnet", seed=11)
    assert list(both) == ["random", "greedy", "mcts", "nn", "mcts+nn", "nn-prev", "mcts+nn-prev"]
    assert all(both[k].name == k for k in both)
    assert all(a.noise_epsilon == 0.0 for a in both.values())
    assert len({a.seed for a in both.values()}) == len(both)
    assert standard_agents("new.arnet", Cfg, seed=12)["random"].seed != std["random"].seed
    assert (both["random"].kind, both["greedy"].kind) == ("random", "greedy")
    assert (both["mcts"].checkpoint, both["mcts"].simulations, both["mcts"].c_puct, both["mcts"].temperature) == (None, 500, 0.512, 1.0)
    assert (both["mcts+nn"].checkpoint, both["mcts+nn-prev"].checkpoint) == ("new.arnet", "old.arnet")
    for k, cp in (("nn", "new.arnet"), ("nn-prev", "old.arnet")):
        assert (both[k].checkpoint, both[k].simulations, both[k].batch_size, both[k].temperature) == (cp, 1, 1, 1.0)


def test_round_robin_plays_every_unordered_pair_once(monkeypatch):
    from alpharat_amd import match
    from alpharat_amd.match import MatchAgent, MatchResult

    calls = []

    def fake(a, b, **kw):
        calls.append((a.name, b.name, kw))
        return MatchResult(a.name, b.name, 1, 0, 1, 0.0, 0.0)

    monkeypatch.setattr(match, "play_match", fake)
    agents = {"random": MatchAgent.random(), "greedy": MatchAgent.greedy(), "mcts": MatchAgent("mcts")}
    out = match.play_round_robin(agents, games_per_matchup=6, width=5, height=5, cheese_count=5, max_turns=30, seed=4)
    assert [c[:2] for c in calls] == [("random", "greedy"), ("random", "mcts"), ("greedy", "mcts")] == list(out)
    for _, _, kw in calls:  # every pair plays the same games
        assert kw == dict(num_games=6, swap_sides=True, width=5, height=5, cheese_count=5, max_turns=30, seed=4)
    assert all(isinstance(r, MatchResult) for r in out.values())
    assert dataclasses.asdict(out[("greedy", "mcts")])["agent_a"] == "greedy"
    with pytest.raises(TypeError):
        match.play_round_robin(agents, games_per_matchup=6, num_games=3, width=5, height=5, cheese_count=5, max_turns=30)
