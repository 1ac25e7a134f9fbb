"""-m gpu: tree reuse (k_advance, alpharat_amd/csrc/dev_advance.h). (a) the compaction routine itself on made-up trees,
through the test entry ar_debug_advance, against the scalar passes restated in NumPy (tests/_advance.py), byte for byte;
(b) self-play records against the oracle with the compaction on its fast path, on its slow path, with trees that change
runs at every move, and on the step stream."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import _advance as A
import _oracle as O

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).parent / "golden" / "nets"
TUNED = dict(c_puct=0.512, fpu_reduction=0.459, force_k=0.103, noise_epsilon=0.25)
ADV_MAX_NODES = 32768  # dev_advance.h: the fast path's tables


def _keep_roots(rec):
    hi = rec.shape[0]
    if hi == 1:
        return [0]
    return sorted({k for k in (1, 37, 300, hi - 1, A.first_leaf(rec)) if k < hi})


@pytest.fixture(scope="module")
def batch():
    """Every (tree, keep_root, in place | moved) of the launch, with what the scalar compaction leaves: at least 600 trees,
    so the blocks outnumber what is resident at once."""
    cases = []  # (records, keep_root, moves)
    for hi in (1, 2, 63, 64, 65, 255, 256, 257):
        for rep in range(12):
            rec = A.random_tree(hi, 1000 * hi + rep)
            cases += [(rec, k, mv) for k in _keep_roots(rec) for mv in (0, 1)]
    for hi in (1000, 4097):
        rec = A.random_tree(hi, hi)
        cases += [(rec, k, mv) for k in _keep_roots(rec) for mv in (0, 1)]
    # everything from keep_root on is kept (src[n] = n + 1, the tightest in-place case): one chunk's worth, several
    # chunks, and a few thousand nodes
    for hi in (40, 1000, 9100):
        cases += [(A.random_tree(hi, 7 * hi, under_first_child=True), 1, mv) for mv in (0, 1)]
    # above the fast path's limit whatever the knob says
    big = A.random_tree(ADV_MAX_NODES + 300, 99)
    cases += [(big, 1, 0), (big, 1, 1)]
    assert len(cases) >= 600
    first = np.cumsum([0] + [c[0].shape[0] for c in cases]).astype(np.uint64)
    want = {}
    expect = []
    for rec, k, mv in cases:
        key = (id(rec), k)
        if key not in want:
            want[key] = A.compact_np(rec, k)
        expect.append(want[key])
    return dict(cases=cases, first=first, expect=expect, records=np.ascontiguousarray(np.concatenate([c[0] for c in cases])))


def _run(batch, fast_nodes):
    from alpharat_amd import _lib

    L = _lib.load()
    L.ar_debug_advance.restype = C.c_int
    L.ar_debug_advance.argtypes = [C.c_void_p, C.c_uint64] + [C.c_void_p] * 4 + [C.c_uint32, C.c_uint32] + [C.c_void_p] * 3
    cases, first, recs = batch["cases"], batch["first"], batch["records"]
    n = len(cases)
    u32 = lambda xs: np.ascontiguousarray(np.asarray(xs, dtype=np.uint32))  # noqa: E731
    f, hi, kr, mv = u32(first[:-1]), u32([c[0].shape[0] for c in cases]), u32([c[1] for c in cases]), u32([c[2] for c in cases])
    a, b, cnt = np.empty_like(recs), np.empty_like(recs), np.zeros(n, np.uint32)
    p = lambda x: x.ctypes.data  # noqa: E731
    _lib.check(L.ar_debug_advance(p(recs), recs.shape[0], p(f), p(hi), p(kr), p(mv), n, fast_nodes, p(a), p(b), p(cnt)))
    return a, b, cnt


@pytest.mark.parametrize("fast_nodes", [0xFFFFFFFF, 64, 0], ids=["default-limit", "limit-64", "all-slow"])
def test_compaction_equals_the_scalar_passes(batch, fast_nodes):
    a, b, cnt = _run(batch, fast_nodes)
    for t, ((rec, k, mv), (out, n)) in enumerate(zip(batch["cases"], batch["expect"])):
        lo, hi = int(batch["first"][t]), int(batch["first"][t + 1])
        what = (t, rec.shape[0], k, "moved" if mv else "in place")
        assert cnt[t] == n, what
        if mv:
            assert a[lo:hi].tobytes() == rec.tobytes(), what  # (the source is left alone)
            assert b[lo:lo + n].tobytes() == out.tobytes(), what
            assert (b[lo + n:hi] == 0xEEEEEEEE).all(), what
        else:
            assert a[lo:lo + n].tobytes() == out.tobytes(), what
            assert a[lo + n:hi].tobytes() == rec[n:].tobytes(), what  # (records from the count on are never written)
            assert (b[lo:hi] == 0xEEEEEEEE).all(), what


# ---- (b) self-play ------------------------------------------------------------------------------------------------------
KNOBS = [dict(), dict(AR_ADV_NODES="64"), dict(AR_ARENA_NODES="256"), dict(AR_NO_ADVANCE_OVERLAP="1")]
KNOB_IDS = ["default", "slow-path", "runs-change", "step-stream"]


@pytest.fixture(scope="module")
def oracle_5x5():
    cfg = O.make_config()
    return [O.play_game(O.Game(5, 5, 30).random_cheese(5, True, i), cfg, 300, 8, 0xA1FA0000 + i) for i in range(12)]


@pytest.fixture(scope="module")
def oracle_7x7():
    from test_gpu_pipeline_parity import HipEvaluator

    ev = HipEvaluator(GOLD / "mlp_7x7_h256.arnet", 7, 7, 50)
    cfg = O.make_config(**TUNED)
    return [O.play_game(O.Game(7, 7, 50).random_cheese(10, True, i), cfg, 500, 16, 0xA1FA0000 + i, backend=4, net=ev.backend,
                        game_index=i) for i in range(8)]


@pytest.mark.parametrize("knobs", KNOBS, ids=KNOB_IDS)
def test_selfplay_5x5_uniform_records_equal_the_oracle(knobs, oracle_5x5, monkeypatch):
    from alpharat_amd.sampling import rust_self_play
    from test_gpu_parity import _check_game

    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    games = {}
    stats = rust_self_play(width=5, height=5, cheese_count=5, max_turns=30, num_games=12, simulations=300, batch_size=8,
                           output_dir=None, seed=0, on_game=lambda g: games.__setitem__(g["game_index"], g))
    assert stats.total_games == 12 and sorted(games) == list(range(12))
    for i, want in enumerate(oracle_5x5):
        _check_game(games[i], want)


@pytest.mark.parametrize("knobs", KNOBS, ids=KNOB_IDS)
def test_selfplay_7x7_mlp_records_equal_the_oracle(knobs, oracle_7x7, monkeypatch):
    from alpharat_amd.sampling import rust_self_play
    from test_gpu_parity import _check_game

    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    games = {}
    stats = rust_self_play(width=7, height=7, cheese_count=10, max_turns=50, num_games=8, simulations=500, batch_size=16,
                           output_dir=None, seed=0, weights_path=str(GOLD / "mlp_7x7_h256.arnet"),
                           on_game=lambda g: games.__setitem__(g["game_index"], g), **TUNED)
    assert stats.total_games == 8 and sorted(games) == list(range(8)) and stats.total_nn_evals > 0
    for i, want in enumerate(oracle_7x7):
        _check_game(games[i], want)
