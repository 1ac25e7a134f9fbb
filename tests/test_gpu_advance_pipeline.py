"""-m gpu: the pipelined move of tree reuse (alpharat_amd/csrc/dev_advance.h: a source list per chunk of whole kept nodes,
the next chunks' loads in flight across a chunk's barrier) and the ticket by which k_advance's blocks take their trees.
(a) The cases of tests/test_advance_pipeline_cpu.py, and one tree on each side of the fast path's limit, through the
test entry ar_debug_advance in one launch, in place and moved, against the scalar compaction restated in NumPy, byte for
byte. (b) Self-play records against the oracle with a grid of two blocks, so that every block takes several trees."""
import numpy as np
import pytest

import _advance as A
import _advance_pipe as P
import _oracle as O

pytestmark = pytest.mark.gpu

ADV_MAX_NODES = 32768  # dev_advance.h: the fast path's tables


@pytest.fixture(scope="module")
def batch():
    trees = [(name, rec, k, P.expect(name)[:2]) for name, rec, k, _ in P.cases()]
    for name, hi in (("below-the-limit", ADV_MAX_NODES), ("above-the-limit", ADV_MAX_NODES + 2)):  # hi - keep_root = limit -+ 1
        rec = A.random_tree(hi, hi)
        trees.append((name, rec, 1, A.compact_np(rec, 1)))
    cases = [(rec, k, mv) for _, rec, k, _ in trees for mv in (0, 1)]
    expect = [e for _, _, _, e in trees for _ in (0, 1)]
    names = [name for name, _, _, _ in trees for _ in (0, 1)]
    first = np.cumsum([0] + [c[0].shape[0] for c in cases]).astype(np.uint64)
    return dict(cases=cases, first=first, expect=expect, names=names,
                records=np.ascontiguousarray(np.concatenate([c[0] for c in cases])))


def test_compaction_equals_the_scalar_passes(batch):
    from test_gpu_advance import _run

    a, b, cnt = _run(batch, 0xFFFFFFFF)
    for t, ((rec, k, mv), (out, n)) in enumerate(zip(batch["cases"], batch["expect"])):
        lo, hi = int(batch["first"][t]), int(batch["first"][t + 1])
        what = (batch["names"][t], rec.shape[0], k, "moved" if mv else "in place")
        assert cnt[t] == n, what
        if mv:
            assert a[lo:hi].tobytes() == rec.tobytes(), what  # (the source is left alone)
            assert b[lo:lo + n].tobytes() == out.tobytes(), what
            assert (b[lo + n:hi] == 0xEEEEEEEE).all(), what
        else:
            assert a[lo:lo + n].tobytes() == out.tobytes(), what
            assert a[lo + n:hi].tobytes() == rec[n:].tobytes(), what  # (records from the count on are never written)
            assert (b[lo:hi] == 0xEEEEEEEE).all(), what


def test_selfplay_5x5_uniform_with_two_blocks_equals_the_oracle(monkeypatch):
    """12 games share two blocks: each takes its first tree by its number and every later one through the ticket."""
    from alpharat_amd.sampling import rust_self_play
    from test_gpu_parity import _check_game

    cfg = O.make_config()
    want = [O.play_game(O.Game(5, 5, 30).random_cheese(5, True, i), cfg, 300, 8, 0xA1FA0000 + i) for i in range(12)]
    monkeypatch.setenv("AR_ADV_BLOCKS", "2")
    games = {}
    stats = rust_self_play(width=5, height=5, cheese_count=5, max_turns=30, num_games=12, simulations=300, batch_size=8,
                           output_dir=None, seed=0, on_game=lambda g: games.__setitem__(g["game_index"], g))
    assert stats.total_games == 12 and sorted(games) == list(range(12))
    for i, w in enumerate(want):
        _check_game(games[i], w)
