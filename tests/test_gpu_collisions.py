"""-m gpu: collision budgets (collision_limit_* / collision_scaling_*, search.rs:437-450 and :961-999) through the real
kernels, bit-exact against the oracle. The budget sets how many pick_nodes_to_extend calls a batch makes (at most
batch_size + budget); the work-queue gather (k_gatherw) keys its entries with the pick number, so it serves a batch only
while that bound is at most GW_MAX_PICKS (dev_gatherw.h), and k_gather8 takes the rest. Batch sizes 16 and below reach
k_gatherw on the network path, 17 and above k_gather8. Every case here is first checked on the CPU harness
(test_kernel_logic_cpu.py, the collision sweep)."""
import numpy as np
import pytest

import _oracle as O
from _random_nets import random_mlp
from test_gpu_parity import _assert_result, _check_game, _pyrat
from test_gpu_pipeline_parity import GOLD, HipEvaluator

pytestmark = pytest.mark.gpu

TUNED = dict(c_puct=0.512, fpu_reduction=0.459, force_k=0.103)
GW_MAX_PICKS = 4095
MLP = GOLD / "mlp_7x7_h256.arnet"


def _coll(lo, hi=None, start=800, end=50000, power=1.0):
    return dict(collision_limit_min=lo, collision_limit_max=lo if hi is None else hi, collision_scaling_start=start,
                collision_scaling_end=end, collision_scaling_power=power)


def _positions_7x7():
    """7x7 positions (the board of the network): an open maze, a random maze with mud, both players on one cell"""
    yield O.Game(7, 7, 50).random_cheese(10, True, 5)
    yield O.Game(7, 7, 50).random_maze(0.7, 0.2, True, 3).random_cheese(8, True, 3)
    g = O.Game(7, 7, 50, p1=(3, 3), p2=(3, 3), cheese=[(i, 0) for i in range(7)])
    g.make_move(0, 0)
    yield g


def _cost(og):
    maze = og.maze().reshape(-1).astype(np.int16)
    return np.where(maze < 0, 0, maze).astype(np.uint8)


# (collision settings, simulations, batch): fixed budgets around the old 8-bit pick number and the 4095-pick bound,
# budgets that scale while the tree grows, a minimum of 0 (empty batches), and batch sizes on both sides of GW_SLOTS
CASES = [
    (_coll(1), 1001, 16),
    (_coll(256), 1001, 16),
    (_coll(257), 1001, 16),
    (_coll(1000), 1001, 16),
    (_coll(4079), 1001, 16),   # 16 + 4079 = 4095: still the work-queue gather
    (_coll(4080), 1001, 16),   # one past: k_gather8
    (_coll(65536), 1001, 16),
    (_coll(1, 512, 20, 1500, 0.5), 1001, 16),
    (_coll(1, 512, 20, 1500, 2.0), 1001, 16),
    (_coll(0, 256, 20, 1500, 2.0), 1001, 16),
    (_coll(1000), 301, 1),
    (_coll(4080), 1001, 15),   # 15 + 4080 = 4095
    (_coll(1000), 1001, 17),
    (_coll(257), 1001, 64),
]


def _id(case):
    c, sims, batch = case
    return f"min{c['collision_limit_min']}-max{c['collision_limit_max']}-p{c['collision_scaling_power']}-b{batch}-s{sims}"


@pytest.fixture(scope="module")
def mlp():
    from alpharat_amd.nets import Net

    return Net(str(MLP))


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_net_searches_collision_budgets(case, mlp):
    """rust_mcts_search and search_many with the device MLP; the oracle evaluates its leaves with the same device net."""
    from alpharat_amd.mcts import rust_mcts_search, search_many

    coll, sims, batch = case
    ogs = list(_positions_7x7())
    seeds = [11 + i for i in range(len(ogs))]
    res = search_many([_pyrat(og, 50) for og in ogs], simulations=sims, batch_size=batch, seeds=seeds, net=mlp, **TUNED,
                      **coll)
    one = rust_mcts_search(_pyrat(ogs[1], 50), simulations=sims, batch_size=batch, seed=seeds[1], net=mlp, **TUNED, **coll)
    cfg = O.make_config(**TUNED, **coll)
    for i, og in enumerate(ogs):
        ev = HipEvaluator(MLP, 7, 7, 50, cost=_cost(og))
        want = O.search_once(og, cfg, sims, batch, seed=seeds[i], backend=4, net=ev.backend)
        _assert_result(res[i], want, ("search_many", i))
        if i == 1:
            _assert_result(one, want, "rust_mcts_search")


@pytest.mark.parametrize("uniform", ["queue", "fused"])
def test_smart_uniform_searches_collision_budgets(uniform, monkeypatch):
    """SmartUniform: the split pipeline (lane gather) and the fused search kernel at the same budgets."""
    from alpharat_amd.mcts import search_many
    from test_kernel_logic_cpu import games

    monkeypatch.setenv("AR_UNIFORM", uniform)
    items = list(games())
    for coll, sims, batch in CASES:
        seeds = [5 + i for i in range(len(items))]
        res = search_many([_pyrat(og, mt) for _, og, mt in items], simulations=sims, batch_size=batch, seeds=seeds,
                          **TUNED, **coll)
        cfg = O.make_config(**TUNED, **coll)
        for i, (name, og, _) in enumerate(items):
            _assert_result(res[i], O.search_once(og, cfg, sims, batch, seed=seeds[i]), (name, _id((coll, sims, batch))))


def _selfplay(w, h, cheese, turns, n_games, sims, blob, coll, **kw):
    """A whole network self-play run in one session: (records by game index, session info)."""
    from alpharat_amd.sampling import SelfPlaySession

    games = {}
    with SelfPlaySession(width=w, height=h, cheese_count=cheese, max_turns=turns, num_games=n_games, simulations=sims,
                         batch_size=16, seed=0, concurrent_games=n_games, weights_path=str(blob), noise_epsilon=0.25,
                         on_game=lambda g: games.__setitem__(g["game_index"], g), **TUNED, **coll, **kw) as s:
        info = s.info()
        s.run_to_end()
    assert sorted(games) == list(range(n_games))
    return games, info


def _replay(w, h, cheese, turns, sims, blob, coll, idx):
    ev = HipEvaluator(blob, w, h, turns)
    cfg = O.make_config(noise_epsilon=0.25, **TUNED, **coll)
    return {i: O.play_game(O.Game(w, h, turns).random_cheese(cheese, True, i), cfg, sims, 16, 0xA1FA0000 + i, backend=4,
                           net=ev.backend, game_index=i) for i in idx}


def _same_records(a, b):
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == b[k].tobytes(), k
        else:
            assert v == b[k], k


@pytest.mark.parametrize("coll", [_coll(1000), _coll(1, 512, 20, 1500, 2.0)], ids=["limit1000", "scaling_p2"])
def test_network_selfplay_per_gather_kernel(coll, monkeypatch):
    """The three gathers of the network path play the same 40 games (tree reuse carries the node count, and with it
    the budget, from move to move); two of them are replayed on the oracle."""
    runs = {}
    for shape, kind in (("wide", 2), ("octet", 1), ("lane", 0)):
        monkeypatch.setenv("AR_GATHER", shape)
        runs[shape], info = _selfplay(7, 7, 10, 50, 40, 600, MLP, coll)
        assert info["gather_kind"] == kind, (shape, info)
    want = _replay(7, 7, 10, 50, 600, MLP, coll, (0, 39))
    for i, w in want.items():
        _check_game(runs["wide"][i], w)
        assert w["total_collisions"] > 0
    for shape in ("octet", "lane"):
        for i in range(40):
            _same_records(runs["wide"][i], runs[shape][i])


def test_wide_gather_refused_beyond_its_pick_bound(monkeypatch):
    """batch 16 + a budget of 65536: AR_GATHER=wide is not taken (k_gather8 runs), and the records stay exact."""
    coll = _coll(65536)
    monkeypatch.setenv("AR_GATHER", "wide")
    got, info = _selfplay(7, 7, 10, 50, 8, 200, MLP, coll)
    assert info["gather_kind"] == 1, info
    _check_game(got[3], _replay(7, 7, 10, 50, 200, MLP, coll, (3,))[3])


def _random_mlp(tmp_path, w, h, hidden, seed):
    """seeded random PyRatMLP weights (tests/_random_nets.py) for a w x h board"""
    from alpharat_amd.weights import write_blob

    return write_blob(tmp_path / f"mlp_{w}x{h}_h{hidden}.arnet", "mlp", w, h, random_mlp(w, h, hidden, seed))


@pytest.mark.parametrize("w,h,cheese,turns", [(9, 10, 12, 40), (15, 11, 21, 40)])
def test_network_selfplay_above_64_cells_through_the_work_queue_gather(w, h, cheese, turns, tmp_path):
    """Boards above 64 cells take the four-word state build of k_gatherw (16 games per wavefront)."""
    blob = _random_mlp(tmp_path, w, h, 64, w * 100 + h)
    coll = _coll(1, 512, 20, 1500, 2.0)
    got, info = _selfplay(w, h, cheese, turns, 8, 300, blob, coll)
    assert info["gather_kind"] == 2, info
    want = _replay(w, h, cheese, turns, 300, blob, coll, (0, 7))
    for i, wt in want.items():
        _check_game(got[i], wt)
        assert wt["total_nn_evals"] > 0


def test_collision_min_above_max_is_refused(mlp):
    """The reference's u32::clamp panics on min > max; every entry point refuses it before any device work."""
    from alpharat_amd.mcts import rust_mcts_search, search_many
    from alpharat_amd.sampling import rust_self_play

    og = next(_positions_7x7())
    bad = _coll(300, 299)
    with pytest.raises(ValueError, match="collision_limit_min"):
        rust_mcts_search(_pyrat(og, 50), simulations=50, batch_size=8, seed=1, **bad)
    with pytest.raises(ValueError, match="collision_limit_min"):
        search_many([_pyrat(og, 50)], simulations=50, batch_size=8, seeds=[1], net=mlp, **bad)
    with pytest.raises(ValueError, match="collision_limit_min"):
        rust_self_play(width=7, height=7, cheese_count=10, max_turns=50, num_games=2, simulations=50, batch_size=8,
                       output_dir=None, seed=0, **bad)
    # min == max is a fixed budget, and the library still searches after the refusals
    ok = _coll(299, 299)
    got = rust_mcts_search(_pyrat(og, 50), simulations=50, batch_size=8, seed=1, **ok)
    _assert_result(got, O.search_once(og, O.make_config(**ok), 50, 8, seed=1), "after refusal")
