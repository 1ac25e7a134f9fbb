"""-m gpu: every network kernel on boards of 1 to 256 cells, against a high-precision reference.

Boards above 64 cells take the four-word instantiation of every evaluator (net_launch<4>), and several kernel paths are
picked by formulas in the board size. Each case's id names the path net_launch's rules send it to. PyRatMLP and
SymmetricMLP get seeded random weights (their first layers have an hw dimension); PyRatCNN and KataGoCNN get a golden's
trained weights written for the board at hand (none of their tensors depends on the board size). The positions
(tests/_random_nets.py) have one generated maze per leaf, cheese in every 64-bit word, players on high cells, mud
timers and unequal scores.

Every case: the device encoder equals the oracle's (1e-6); the six outputs are within 1e-5 of the reference (the
oracle's forward, accumulating in double; tests/_katago_np.py for KataGoCNN); and a position's outputs are the same
bits whether it is evaluated with the others, in reverse order or alone. The second half runs self-play and search at
NW = 4 against the oracle driven through the same device network, byte for byte."""
from pathlib import Path

import numpy as np
import pytest

import _katago_np
import _oracle as O
from _random_nets import positions, pyrat, random_mlp, random_symmetric, transplant
from test_gpu_parity import _check_game
from test_gpu_pipeline_parity import HipEvaluator

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).parent / "golden"
KEYS = ("logits_p1", "logits_p2", "policy_p1", "policy_p2", "value_p1", "value_p2")
TUNED = dict(c_puct=0.512, fpu_reduction=0.459, force_k=0.103, noise_epsilon=0.25)


def _blob(tmp_path, arch, w, h, t, name=""):
    from alpharat_amd.weights import write_blob

    return write_blob(tmp_path / f"{arch}{name}_{w}x{h}.arnet", arch, w, h, t)


def _run(blob, w, h, ogs, reference, atol=None):
    """encoder, outputs against `reference(obs)` (logits and values within `atol(want)` if given, else 1e-5), and the
    same bits together / backwards / alone; the outputs"""
    from alpharat_amd.nets import Net, encode

    games = [pyrat(og) for og in ogs]
    obs = np.stack([og.encode() for og in ogs])
    np.testing.assert_allclose(encode(games), obs, atol=1e-6, rtol=0)
    net = Net(blob)
    together = net.evaluate(games)
    want = reference(obs)
    for k in KEYS:
        if atol is not None and not k.startswith("policy"):
            bound = atol(want)[:, None] if together[k].ndim == 2 else atol(want)
            err = np.abs(together[k] - want[k])
            assert (err <= bound + 1e-5 * np.abs(want[k])).all(), (k, err.max())
        else:
            np.testing.assert_allclose(together[k], want[k], atol=1e-5, rtol=1e-5, err_msg=k)
    backwards = net.evaluate(games[::-1])
    alone = [net.evaluate([g]) for g in games]
    for k in KEYS:
        assert together[k].tobytes() == backwards[k][::-1].tobytes(), k
        assert together[k].tobytes() == np.concatenate([a[k] for a in alone]).tobytes(), k
    return net, games, together


def _same_bits(a, b, what):
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


# ---- PyRatMLP: k_mlp_mfma's first-layer variant FL is 2 while K2e = (hw+7)&~1 <= H+4, else 1; FL=0 needs
# K1e = (3hw+7)&~1 <= H+4; H 48 / 320 take k_mlp (scalar / wide first layer) --------------------------------------
MLP_CASES = [
    (8, 8, 64, "mfma-NW1-bit63-FL1"),
    (31, 2, 64, "mfma-NW1-FL2-row-full"),
    (9, 7, 64, "mfma-NW1-FL1"),
    (14, 9, 128, "mfma-NW4-FL2-row-full"),
    (16, 8, 128, "mfma-NW4-FL1"),
    (15, 11, 256, "mfma-NW4-FL2-odd"),
    (12, 7, 256, "mfma-NW4-FL012"),
    (13, 5, 256, "mfma-NW4-FL012"),
    (16, 16, 256, "mfma-NW4-FL1-limit"),
    (16, 16, 48, "k_mlp-scalar-NW4"),
    (16, 16, 320, "k_mlp-wide-NW4"),
]


@pytest.mark.parametrize("w,h,H,path", MLP_CASES, ids=[f"{w}x{h}-h{H}-{p}" for w, h, H, p in MLP_CASES])
def test_mlp_on_board(w, h, H, path, tmp_path, monkeypatch):
    t = random_mlp(w, h, H, seed=w * 100 + h + H)
    blob = _blob(tmp_path, "mlp", w, h, t)
    ogs = positions(w, h, 70, seed=w * 1000 + h)
    net, games, got = _run(blob, w, h, ogs, O.Net(blob).forward)
    if path.endswith("FL012"):
        for fl in ("0", "1", "2"):
            monkeypatch.setenv("AR_MLP_FL", fl)
            _same_bits(got, net.evaluate(games), f"AR_MLP_FL={fl}")


def test_mlp_one_maze_batch_at_the_cell_limit(tmp_path):
    """70 leaves of one maze share one pool entry and one set of maze constants"""
    t = random_mlp(16, 16, 256, seed=7)
    blob = _blob(tmp_path, "mlp", 16, 16, t)
    _run(blob, 16, 16, positions(16, 16, 70, seed=8, mazes=1), O.Net(blob).forward)


# ---- SymmetricMLP: k_symmetric_mfma2 while Kse = (hw+2)&~1 <= H+4, else k_symmetric ------------------------------
SYM_CASES = [
    (11, 6, 64, "mfma2-NW4-row-full"),
    (17, 4, 64, "k_symmetric-NW4"),
    (15, 11, 192, "mfma2-NW4-fma-same-bits"),
    (16, 16, 256, "mfma2-NW4-limit-fma-same-bits"),
    (13, 5, 48, "k_symmetric-NW4"),
]


@pytest.mark.parametrize("w,h,H,path", SYM_CASES, ids=[f"{w}x{h}-h{H}-{p}" for w, h, H, p in SYM_CASES])
def test_symmetric_on_board(w, h, H, path, tmp_path, monkeypatch):
    t = random_symmetric(w, h, H, seed=w * 100 + h + H)
    blob = _blob(tmp_path, "symmetric", w, h, t)
    ogs = positions(w, h, 70, seed=w * 1000 + h + 1)
    net, games, got = _run(blob, w, h, ogs, O.Net(blob).forward)
    if path.endswith("fma-same-bits"):
        monkeypatch.setenv("AR_SYM_FMA", "1")
        _same_bits(got, net.evaluate(games), "AR_SYM_FMA=1")


def test_symmetric_one_maze_batch_at_the_cell_limit(tmp_path):
    t = random_symmetric(16, 16, 256, seed=9)
    blob = _blob(tmp_path, "symmetric", 16, 16, t)
    _run(blob, 16, 16, positions(16, 16, 70, seed=10, mazes=1), O.Net(blob).forward)


# ---- PyRatCNN: k_cnn_mfma with MT = 1 (hw <= 128) or 2 tiles of 32 rows per wavefront and L = 128 MT / hw leaves per
# workgroup (fewer if the image would pass 64 KB); C = 16 takes k_cnn, whose conv3x3_tile_big walks row groups of
# 256 / C rows and column blocks of 8 ------------------------------------------------------------------------------
CNN_CASES = [
    ("cnn_gpool_7x7_c64", 8, 8, "mfma-MT1-L2-bit63"),
    ("cnn_pooled_7x7_c32", 8, 8, "mfma-MT1-L2-bit63"),
    ("cnn_res_15x11_c64", 11, 6, "mfma-MT1-L1"),
    ("cnn_gpool_15x11_c32", 16, 8, "mfma-MT1-L1-full-tile"),
    ("cnn_pooled_7x7_c32", 43, 3, "mfma-MT2-first"),
    ("cnn_res_15x11_c64", 13, 10, "mfma-MT2"),
    ("cnn_gpool_15x11_c32", 16, 16, "mfma-MT2-limit"),
    ("cnn_gpool_7x7_c64", 16, 16, "mfma-MT2-limit"),
    ("cnn_res_15x11_c64", 16, 16, "mfma-MT2-limit"),
    ("cnn_gpool_9x10_c16", 16, 16, "k_cnn-limit"),
    ("cnn_gpool_9x10_c16", 2, 40, "k_cnn-row-groups"),
    ("cnn_gpool_9x10_c16", 40, 2, "k_cnn-column-blocks"),
]


def _fp32_chain_atol(t):
    """An absolute bar for logits (and values) that scales with the logits, from the length of the fp32 chain.

    The device and the oracle round every activation to fp32 (u = 2^-24). A sum of K fp32 terms is off by about
    sqrt(K) u times the magnitudes summed; a logit is the end of n such sums in a row -- the stem, two convolutions per
    block (K = 9 C), the pooling, the combiner and the head -- each carrying at least the logit's own magnitude. So the
    bar is 1e-5 + n sqrt(9 C) u max|logit of the row|. A golden trained on 7x7 and moved to 16x16 reaches logits of
    ~13 (its pooled features grow with the board), where a flat 1e-5 is below 1 ulp of a 576-term chain."""
    C = t["stem.weight"].shape[0]
    n = 1 + 2 * sum(1 for k in t if k.endswith(".conv1.weight")) + 3
    k = n * np.sqrt(9 * C) * 2.0 ** -24
    return lambda want: 1e-5 + k * np.maximum(np.abs(want["logits_p1"]).max(axis=1), np.abs(want["logits_p2"]).max(axis=1))


@pytest.mark.parametrize("name,w,h,path", CNN_CASES, ids=[f"{n}-on-{w}x{h}-{p}" for n, w, h, p in CNN_CASES])
def test_cnn_on_board(name, w, h, path, tmp_path):
    arch, t = transplant(GOLD / "nets" / f"{name}.arnet", w, h)
    blob = _blob(tmp_path, arch, w, h, t)
    atol = _fp32_chain_atol(t) if (name, w, h) == ("cnn_gpool_7x7_c64", 16, 16) else None
    _run(blob, w, h, positions(w, h, 40, seed=w * 1000 + h + 2), O.Net(blob).forward, atol)


KATAGO_CASES = [(n, w, h) for n in ("katago_15x11_c32", "katago_7x7_c64") for w, h in ((11, 6), (16, 8), (13, 10), (16, 16),
                                                                                       (2, 40))]


@pytest.mark.parametrize("name,w,h", KATAGO_CASES,
                         ids=[f"{n}-on-{w}x{h}-mfma-MT{2 if w * h > 128 else 1}" for n, w, h in KATAGO_CASES])
def test_katago_on_board(name, w, h, tmp_path):
    arch, t = transplant(GOLD / "nets_katago" / f"{name}.arnet", w, h)
    blob = _blob(tmp_path, arch, w, h, t)
    _run(blob, w, h, positions(w, h, 40, seed=w * 1000 + h + 3), lambda obs: _katago_np.forward(t, w, h, obs))


def test_boards_above_256_cells_are_refused_at_load(tmp_path):
    from alpharat_amd.nets import Net

    blobs = [_blob(tmp_path, "mlp", 17, 16, random_mlp(17, 16, 64, seed=1)),
             _blob(tmp_path, "symmetric", 17, 16, random_symmetric(17, 16, 64, seed=1))]
    for name in ("nets/cnn_gpool_15x11_c32", "nets/cnn_gpool_9x10_c16", "nets_katago/katago_15x11_c32"):
        arch, t = transplant(GOLD / f"{name}.arnet", 17, 16)
        blobs.append(_blob(tmp_path, arch, 17, 16, t, name=Path(name).name))
    for blob in blobs:
        with pytest.raises(RuntimeError, match=r"17x16 board: boards of 1 to 256 cells are supported"):
            Net(blob)


# ---- the pipeline at NW = 4 ----------------------------------------------------------------------------------------
def _cost(og):
    return np.ascontiguousarray(og.cost().reshape(-1))


def _selfplay(blob, w, h, cheese, turns, n_games, resident, sims, seed, cache=0, wall=0.6, mud=0.2):
    from alpharat_amd.sampling import rust_self_play

    games = {}
    st = rust_self_play(width=w, height=h, cheese_count=cheese, max_turns=turns, num_games=n_games, simulations=sims,
                        batch_size=16, output_dir=None, seed=seed, concurrent_games=resident, cache_size=cache,
                        maze_type="random", wall_density=wall, mud_density=mud, weights_path=str(blob),
                        on_game=lambda g: games.__setitem__(g["game_index"], g), **TUNED)
    assert st.total_games == n_games and sorted(games) == list(range(n_games))
    return st, games


def _replay(blob, w, h, cheese, turns, sims, seed, i, wall=0.6, mud=0.2):
    og = O.Game(w, h, turns).random_maze(wall, mud, True, seed + i).random_cheese(cheese, True, seed + i)
    ev = HipEvaluator(blob, w, h, turns, cost=_cost(og))
    return O.play_game(og, O.make_config(**TUNED), sims, 16, 0xA1FA0000 + seed + i, backend=4, net=ev.backend,
                       game_index=i)


def _pipeline_blob(kind, tmp_path):
    if kind == "symmetric_15x11_h192":
        return _blob(tmp_path, "symmetric", 15, 11, random_symmetric(15, 11, 192, seed=31)), 15, 11
    if kind == "mlp_15x11_h256":
        return _blob(tmp_path, "mlp", 15, 11, random_mlp(15, 11, 256, seed=32)), 15, 11
    if kind == "cnn_gpool_15x11_c32_on_16x16":
        arch, t = transplant(GOLD / "nets" / "cnn_gpool_15x11_c32.arnet", 16, 16)
        return _blob(tmp_path, arch, 16, 16, t), 16, 16
    arch, t = transplant(GOLD / "nets_katago" / "katago_15x11_c32.arnet", 11, 6)
    return _blob(tmp_path, arch, 11, 6, t), 11, 6


PIPELINE = ["symmetric_15x11_h192-mfma2", "mlp_15x11_h256-FL2", "cnn_gpool_15x11_c32_on_16x16-MT2",
            "katago_15x11_c32_on_11x6-MT1"]


@pytest.mark.parametrize("kind", PIPELINE)
def test_selfplay_on_generated_mazes_above_64_cells(kind, tmp_path):
    """maze_type "random" with mud, 10 games in 8 resident slots (two refills rebind their slots' maze constants),
    tuned constants with noise: the first and the last game are the oracle's byte for byte"""
    blob, w, h = _pipeline_blob(kind.split("-")[0], tmp_path)
    cheese, turns, sims, seed = 20, 30, 300, 40  # (an even count: 16x16 and 11x6 have no centre cell)
    _, got = _selfplay(blob, w, h, cheese, turns, 10, 8, sims, seed)
    for i in (0, 9):
        want = _replay(blob, w, h, cheese, turns, sims, seed, i)
        _check_game(got[i], want)
        assert want["total_nn_evals"] > 0


@pytest.mark.parametrize("board", ["7x7", "15x11"])
def test_eval_cache_with_generated_mazes(board, tmp_path):
    """cache_size > 0 on generated mazes (the maze_game part of the cache key): the records of cache_size = 0, hits,
    and every request a hit or a miss"""
    if board == "7x7":
        blob, w, h, cheese, turns = GOLD / "nets" / "mlp_7x7_h256.arnet", 7, 7, 10, 50
    else:
        blob, w, h, cheese, turns = _blob(tmp_path, "mlp", 15, 11, random_mlp(15, 11, 256, seed=33)), 15, 11, 20, 30
    st0, base = _selfplay(blob, w, h, cheese, turns, 24, 8, 300, 50)
    st1, cached = _selfplay(blob, w, h, cheese, turns, 24, 8, 300, 50, cache=4096)
    assert st0.cache_hits == 0 and st0.cache_misses == 0
    assert st1.cache_hits > 0
    assert st1.cache_hits + st1.cache_misses == st1.total_nn_evals == st0.total_nn_evals
    for i, g in base.items():
        for k, v in g.items():
            if isinstance(v, np.ndarray):
                np.testing.assert_array_equal(v, cached[i][k], err_msg=f"game {i} {k}")
            else:
                assert v == cached[i][k], (i, k)


def test_search_at_the_cell_limit_bit_exact_vs_oracle(tmp_path):
    """one rust_mcts_search with a network on a 16x16 position of a generated maze"""
    from alpharat_amd.mcts import rust_mcts_search
    from alpharat_amd.nets import Net

    blob = _blob(tmp_path, "mlp", 16, 16, random_mlp(16, 16, 256, seed=34))
    og = positions(16, 16, 2, seed=35)[1]
    kw = dict(c_puct=0.512, fpu_reduction=0.459, force_k=0.103)
    got = rust_mcts_search(pyrat(og), simulations=400, batch_size=16, seed=9, net=Net(blob), **kw)
    ev = HipEvaluator(blob, 16, 16, 100, cost=_cost(og))
    want = O.search_once(og, O.make_config(**kw), 400, 16, seed=9, backend=4, net=ev.backend)
    for k in ("policy_p1", "policy_p2", "visit_counts_p1", "visit_counts_p2", "prior_p1", "prior_p2"):
        assert np.asarray(getattr(got, k), np.float32).tobytes() == np.asarray(want[k], np.float32).tobytes(), k
    assert (got.total_visits, got.value_p1, got.value_p2) == (want["total_visits"], float(want["value_p1"]),
                                                            float(want["value_p2"]))
