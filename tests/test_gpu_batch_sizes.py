"""-m gpu: batch sizes above 16 (check_cfg accepts 1..4096) through the real kernels, bit-exact against the oracle.
The batch size decides which gather runs (the work-queue gather serves at most GW_SLOTS = 16 entries, k_gather8 the rest),
how many trips k_backup16 makes round its chunks of sixteen entries, how the per-slot scratch is carved (ProcEntry[batch],
CollEntry[coll_max + batch + 1], EvalOut[batch], State[batch]) and how large the leaf queue, the cache's miss map and
predict_fn's buffers are. From 257 on a batch's evaluation indices no longer fit eight bits (dev_search.h proc_pack).
Every search case here is first checked on the CPU harness (test_kernel_logic_cpu.py, the batch-size sweep)."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
from test_gpu_parity import _assert_result, _check_game, _games, _pyrat
from test_gpu_pipeline_parity import GOLD, HipEvaluator

pytestmark = pytest.mark.gpu

TUNED = dict(c_puct=0.512, fpu_reduction=0.459, force_k=0.103)
MLP = GOLD / "mlp_7x7_h256.arnet"


def _coll(limit):
    """a fixed collision budget: with one of at least the batch size, batches fill as far as the tree lets them"""
    return dict(collision_limit_min=limit, collision_limit_max=limit)


# (batch, collision settings, simulations): default budgets up to 64; from 257 on a fixed budget of at least the batch
# size (2000 where the batch is smaller) and ten batches' worth of simulations; batches larger than the whole search
SEARCH_CASES = [
    (17, dict(), 1000),
    (64, dict(), 2000),
    (257, _coll(2000), 3000),
    (512, _coll(2000), 5120),
    (4096, _coll(4096), 40960),
    (64, dict(), 10),
    (4096, _coll(4096), 100),
]
SEARCH_IDS = [f"b{b}-s{s}-{'fixed' if c else 'default'}" for b, c, s in SEARCH_CASES]


@pytest.mark.parametrize("uniform", ["fused", "queue"])
@pytest.mark.parametrize("batch,coll,sims", SEARCH_CASES, ids=SEARCH_IDS)
def test_smart_uniform_searches(batch, coll, sims, uniform, monkeypatch):
    """search_many over every position (15x11: the four-word masks; a terminal root) and rust_mcts_search on one, through
    the fused search kernel and through the split pipeline (k_gather8 -> k_uniform_eval -> k_backup16 in chunks)."""
    from alpharat_amd.mcts import rust_mcts_search, search_many

    monkeypatch.setenv("AR_UNIFORM", uniform)
    items = list(_games())
    seeds = [23 + i for i in range(len(items))]
    res = search_many([_pyrat(og, mt) for _, og, mt in items], simulations=sims, batch_size=batch, seeds=seeds, **TUNED,
                      **coll)
    one = rust_mcts_search(_pyrat(items[3][1], items[3][2]), simulations=sims, batch_size=batch, seed=seeds[3], **TUNED,
                           **coll)
    cfg = O.make_config(**TUNED, **coll)
    for i, (name, og, _) in enumerate(items):
        want = O.search_once(og, cfg, sims, batch, seed=seeds[i])
        _assert_result(res[i], want, (name, batch, "search_many"))
        if i == 3:
            _assert_result(one, want, (name, batch, "rust_mcts_search"))


def _constant_predict(sizes):
    def predict_fn(games):
        sizes.append(len(games))
        n = len(games)
        p1 = np.zeros((n, 5), np.float32)
        p2 = np.zeros((n, 5), np.float32)
        for i, g in enumerate(games):
            for arr, eff in ((p1, g.effective_actions_p1()), (p2, g.effective_actions_p2())):
                u = sorted(set(eff))
                for a in u:
                    arr[i, a] = np.float32(1.0) / np.float32(len(u))
        return p1, p2, np.full(n, 1.5, np.float32), np.full(n, 0.5, np.float32)

    return predict_fn


@pytest.mark.parametrize("batch,coll,sims", [(32, dict(), 600), (300, _coll(2000), 3000)], ids=["b32", "b300"])
def test_predict_fn_batches_above_16(batch, coll, sims):
    """The host callback's buffers at these sizes; at 300 a call carries more leaves than eight bits of index hold."""
    from alpharat_amd.mcts import rust_mcts_search

    for og, mt in ((O.Game(5, 5, 100, p1=(1, 1), p2=(3, 3), cheese=[(2, 2), (0, 4)]), 100),
                   (O.Game(7, 7, 50).random_cheese(10, True, 5), 50)):
        sizes = []
        want = O.search_once(og, O.make_config(**coll), sims, batch, seed=123, backend=1, v1=1.5, v2=0.5)
        got = rust_mcts_search(_pyrat(og, mt), predict_fn=_constant_predict(sizes), simulations=sims, batch_size=batch,
                               seed=123, **coll)
        _assert_result(got, want, ("callback", batch, og.w))
        assert sizes and max(sizes) <= batch
        if batch > 256:
            assert max(sizes) > 256, max(sizes)


@pytest.mark.parametrize("uniform", ["fused", "queue"])
@pytest.mark.parametrize("batch,coll,sims", [(32, dict(), 600), (300, _coll(2000), 3000)], ids=["b32", "b300"])
def test_smart_uniform_selfplay(batch, coll, sims, uniform, monkeypatch):
    """Whole games with tree reuse, more games than slots (refills) and noise (k_backup then takes the root batches behind
    k_backup16), through both SmartUniform pipelines: every record against the oracle's."""
    from alpharat_amd.sampling import rust_self_play

    monkeypatch.setenv("AR_UNIFORM", uniform)
    kw = dict(noise_epsilon=0.25, **TUNED, **coll)
    games = {}
    n_games = 20
    stats = rust_self_play(width=7, height=7, cheese_count=10, max_turns=50, num_games=n_games, simulations=sims,
                           batch_size=batch, output_dir=None, seed=0, concurrent_games=8,
                           on_game=lambda g: games.__setitem__(g["game_index"], g), **kw)
    assert stats.total_games == n_games and sorted(games) == list(range(n_games))
    cfg = O.make_config(**kw)
    for i in range(n_games):
        _check_game(games[i], O.play_game(O.Game(7, 7, 50).random_cheese(10, True, i), cfg, sims, batch, 0xA1FA0000 + i))


def _net_selfplay(batch, coll, sims, n_games, resident, **kw):
    """A network self-play run in one session: (records by game index, session info, stats)."""
    from alpharat_amd.sampling import SelfPlaySession

    games = {}
    with SelfPlaySession(width=7, height=7, cheese_count=10, max_turns=50, num_games=n_games, simulations=sims,
                         batch_size=batch, seed=0, concurrent_games=resident, weights_path=str(MLP), noise_epsilon=0.25,
                         on_game=lambda g: games.__setitem__(g["game_index"], g), **TUNED, **coll, **kw) as s:
        info = s.info()
        stats = s.run_to_end()
    assert sorted(games) == list(range(n_games))
    return games, info, stats


def _same_records(a, b):
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == b[k].tobytes(), k
        else:
            assert v == b[k], k


NET_CASES = [(17, dict(), 600), (32, dict(), 600), (300, _coll(2000), 3000)]


@pytest.mark.parametrize("batch,coll,sims", NET_CASES, ids=["b17", "b32", "b300"])
def test_network_selfplay(batch, coll, sims, monkeypatch):
    """k_gather8 -> leaf queue -> MLP -> k_backup16 (several chunks per batch) with more games than slots; the oracle
    evaluates its leaves with the same device network. The lane-per-game backup must play the same games."""
    n_games, resident = 24, 16
    got, info, stats = _net_selfplay(batch, coll, sims, n_games, resident)
    assert info["gather_kind"] != 2, info  # the work-queue gather serves at most 16 entries per batch
    assert stats.total_nn_evals > 0
    ev = HipEvaluator(MLP, 7, 7, 50)
    cfg = O.make_config(noise_epsilon=0.25, **TUNED, **coll)
    for i in (0, n_games - 1):  # (the last game started in a refilled slot)
        want = O.play_game(O.Game(7, 7, 50).random_cheese(10, True, i), cfg, sims, batch, 0xA1FA0000 + i, backend=4,
                           net=ev.backend, game_index=i)
        _check_game(got[i], want)
    assert max(ev.backend.sizes) <= batch
    if batch > 256:
        assert max(ev.backend.sizes) > 256, max(ev.backend.sizes)
    monkeypatch.setenv("AR_BACKUP", "lane")
    lane, _, _ = _net_selfplay(batch, coll, sims, n_games, resident)
    for i in range(n_games):
        _same_records(got[i], lane[i])


@pytest.mark.parametrize("batch,coll,sims", NET_CASES[1:], ids=["b32", "b300"])
def test_network_selfplay_with_eval_cache(batch, coll, sims):
    """cache_size > 0: the miss queue, the miss map and the scatter-back of the evaluations at these batch sizes."""
    n_games, resident = 24, 16
    got, _, stats = _net_selfplay(batch, coll, sims, n_games, resident, cache_size=4096)
    assert stats.cache_hits > 0 and stats.cache_misses > 0
    ev = HipEvaluator(MLP, 7, 7, 50)
    cfg = O.make_config(noise_epsilon=0.25, **TUNED, **coll)
    for i in (1, n_games - 1):
        want = O.play_game(O.Game(7, 7, 50).random_cheese(10, True, i), cfg, sims, batch, 0xA1FA0000 + i, backend=4,
                           net=ev.backend, game_index=i)
        _check_game(got[i], want)


@pytest.mark.parametrize("uniform", ["fused", "queue"])
def test_selfplay_above_64_cells_at_batch_32(uniform, monkeypatch):
    """An 11x9 generated maze per game (four-word masks, cost tables in global memory) at batch 32."""
    from alpharat_amd.sampling import rust_self_play

    monkeypatch.setenv("AR_UNIFORM", uniform)
    games = []
    stats = rust_self_play(width=11, height=9, cheese_count=12, max_turns=60, num_games=12, simulations=300, batch_size=32,
                           output_dir=None, seed=0, concurrent_games=8, maze_type="random", on_game=games.append,
                           wall_density=0.8, mud_density=0.2, maze_symmetric=True)
    assert stats.total_games == 12
    cfg = O.make_config()
    for g in games:
        i = g["game_index"]
        og = O.Game(11, 9, 60).random_maze(0.8, 0.2, True, i).random_cheese(12, True, i)
        _check_game(g, O.play_game(og, cfg, 300, 32, 0xA1FA0000 + i))


@pytest.mark.parametrize("batch", [0, 4097])
def test_batch_sizes_outside_the_range_are_refused(batch):
    from alpharat_amd import _lib
    from alpharat_amd.mcts import make_search_config, rust_mcts_search, search_many, spec_from_game
    from alpharat_amd.sampling import rust_self_play

    og = O.Game(5, 5, 100, p1=(1, 1), p2=(3, 3), cheese=[(2, 2), (0, 4)])
    with pytest.raises(ValueError, match="batch_size"):
        rust_mcts_search(_pyrat(og, 100), simulations=50, batch_size=batch, seed=1)
    with pytest.raises(ValueError, match="batch_size"):
        search_many([_pyrat(og, 100)], simulations=50, batch_size=batch, seeds=[1])
    with pytest.raises(ValueError, match="batch_size"):
        rust_self_play(width=5, height=5, cheese_count=5, max_turns=30, num_games=2, simulations=50, batch_size=batch,
                       output_dir=None, seed=0)
    keep = []
    spec = spec_from_game(_pyrat(og, 100), keep)
    cfg = make_search_config()
    out = _lib.ArSearchResult()
    rc = _lib.load().ar_search(C.byref(spec), C.byref(cfg), 50, batch, C.pointer(C.c_uint64(1)), _lib.ArPredictFn(), None,
                               None, 0, C.byref(out))
    assert rc == _lib.AR_E_INVALID
    # the limits themselves are served, and the library still searches after the refusals
    for ok in (1, 4096):
        got = rust_mcts_search(_pyrat(og, 100), simulations=50, batch_size=ok, seed=1)
        _assert_result(got, O.search_once(og, O.make_config(), 50, ok, seed=1), ("after refusal", ok))
