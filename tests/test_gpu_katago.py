"""-m gpu: KataGoCNN (``cnn_katago``, k_cnn_mfma's KataGo instantiation) and LocalValueMLP checkpoints on the device.

Golden vectors come from the reference's own classes (tools/gen_katago_golden.py); the pipeline and the search are
compared with the oracle driven through the HIP evaluator (oracle backend kind 4, as in
test_gpu_pipeline_parity.py), so both sides see the same network bits and records must be equal byte for byte."""
import shutil
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import _oracle as O
from test_gpu_nets import _game_from_obs
from test_gpu_parity import _check_game, _pyrat
from test_gpu_pipeline_parity import TUNED, HipEvaluator

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).parent / "golden"
NETS = GOLD / "nets_katago"
CKPT = GOLD / "ckpt_katago"
KEYS = ("logits_p1", "logits_p2", "policy_p1", "policy_p2", "value_p1", "value_p2")
CASES = {"katago_7x7_c64": (7, 7), "katago_7x5_c32": (7, 5), "katago_15x11_c32": (15, 11)}


def _games(name):
    w, h = CASES[name]
    gold = np.load(NETS / f"{name}.npz")
    return gold, [_game_from_obs(o, w, h) for o in gold["obs"]]


@pytest.mark.parametrize("name", sorted(CASES))
def test_katago_net_matches_reference_outputs(name):
    from alpharat_amd.nets import Net, encode

    gold, games = _games(name)
    np.testing.assert_allclose(encode(games), gold["obs"], atol=1e-6, rtol=0)
    out = Net(NETS / f"{name}.arnet").evaluate(games)
    for k in KEYS:
        np.testing.assert_allclose(out[k], gold[k], atol=1e-5, rtol=1e-5, err_msg=f"{name}:{k}")


@pytest.mark.parametrize("name", sorted(CASES))
def test_katago_leaf_results_do_not_depend_on_the_tile_row(name):
    """35 positions in one call (full and ragged tiles), in reverse order, and one at a time: the same bits."""
    from alpharat_amd.nets import Net

    _, games = _games(name)
    games = (games * 2)[:35]
    net = Net(NETS / f"{name}.arnet")
    together = net.evaluate(games)
    backwards = net.evaluate(games[::-1])
    alone = [net.evaluate([g]) for g in games]
    for k in KEYS:
        assert together[k].tobytes() == backwards[k][::-1].tobytes(), k
        assert together[k].tobytes() == np.concatenate([a[k] for a in alone]).tobytes(), k


@pytest.mark.parametrize("name", ["katago_7x5_c32", "local_value_5x5_h32"])
def test_checkpoint_evaluates_like_its_predict(name, tmp_path):
    from alpharat_amd.nets import Net

    pt = tmp_path / f"{name}.pt"
    shutil.copy(CKPT / f"{name}.pt", pt)
    gold = np.load(CKPT / f"{name}.npz")
    w, h = (int(v) for v in next(t for t in name.split("_") if t[0].isdigit()).split("x"))
    out = Net.from_checkpoint(pt).evaluate([_game_from_obs(o, w, h) for o in gold["obs"]])
    for k in KEYS:
        np.testing.assert_allclose(out[k], gold[k], atol=1e-5, rtol=1e-5, err_msg=f"{name}:{k}")


@pytest.mark.parametrize("cache", [0, 4096])
def test_katago_selfplay_records_bit_exact_vs_oracle(cache):
    from alpharat_amd.sampling import rust_self_play

    blob = NETS / "katago_7x7_c64.arnet"
    games = {}
    stats = rust_self_play(width=7, height=7, cheese_count=10, max_turns=50, num_games=6, simulations=300, batch_size=16,
                           output_dir=None, seed=6, concurrent_games=4, cache_size=cache, weights_path=str(blob),
                           on_game=lambda g: games.__setitem__(g["game_index"], g), **TUNED)
    assert stats.total_games == 6 and sorted(games) == list(range(6)) and stats.total_nn_evals > 0
    if cache:
        assert stats.cache_hits > 0 and stats.cache_misses > 0
    ev = HipEvaluator(blob, 7, 7, 50)
    cfg = O.make_config(**TUNED)
    for i in (0, 5):  # the last one started in a refilled slot
        want = O.play_game(O.Game(7, 7, 50).random_cheese(10, True, 6 + i), cfg, 300, 16, 0xA1FA0000 + 6 + i, backend=4,
                           net=ev.backend, game_index=i)
        _check_game(games[i], want)


def _same_search(got, want):
    for k in ("policy_p1", "policy_p2", "visit_counts_p1", "visit_counts_p2", "prior_p1", "prior_p2"):
        assert np.asarray(getattr(got, k), np.float32).tobytes() == np.asarray(want[k], np.float32).tobytes(), k
    assert (got.total_visits, got.value_p1, got.value_p2) == (want["total_visits"], float(want["value_p1"]),
                                                            float(want["value_p2"]))


def test_katago_search_bit_exact_vs_oracle():
    from alpharat_amd.mcts import rust_mcts_search
    from alpharat_amd.nets import Net

    blob = NETS / "katago_7x7_c64.arnet"
    og = O.Game(7, 7, 50).random_cheese(10, True, 17)
    og.make_move(1, 3)
    kw = dict(c_puct=0.512, fpu_reduction=0.459, force_k=0.103)  # RustMCTSConfig.for_evaluation(): no noise
    got = rust_mcts_search(_pyrat(og, 50), simulations=400, batch_size=16, seed=9, net=Net(blob), **kw)
    ev = HipEvaluator(blob, 7, 7, 50)
    _same_search(got, O.search_once(og, O.make_config(**kw), 400, 16, seed=9, backend=4, net=ev.backend))


def test_katago_checkpoint_through_the_searcher(tmp_path):
    """HipSearcher.from_config(checkpoint=<cnn_katago .pt>): the searcher agent's route, no new arguments."""
    from alpharat_amd.searcher import HipSearcher

    pt = tmp_path / "best_model.pt"
    shutil.copy(CKPT / "katago_7x5_c32.pt", pt)
    cfg = SimpleNamespace(simulations=200, c_puct=0.512, force_k=0.103, fpu_reduction=0.459, batch_size=8,
                          noise_epsilon=0.0, noise_concentration=10.83, collision_limit_min=1, collision_limit_max=256,
                          collision_scaling_start=800, collision_scaling_end=50_000, collision_scaling_power=1.0)
    s = HipSearcher.from_config(cfg, checkpoint=pt, seed=4)
    og = O.Game(7, 5, 40).random_cheese(6, True, 3)
    got = s.search(_pyrat(og, 40))
    ev = HipEvaluator(pt.with_suffix(".arnet"), 7, 5, 40)
    want = O.search_once(og, O.make_config(c_puct=0.512, force_k=0.103, fpu_reduction=0.459), 200, 8, seed=4, backend=4,
                         net=ev.backend)
    for k in ("visit_counts_p1", "visit_counts_p2", "prior_p1", "prior_p2"):
        assert np.array_equal(getattr(got, k), want[k].astype(np.float64)), k
    assert got.total_visits == want["total_visits"]


def _katago_tensors(name="katago_7x5_c32"):
    from alpharat_amd.weights import read_blob

    return read_blob(NETS / f"{name}.arnet")[3]


def test_katago_with_16_channels_is_refused(tmp_path):
    from alpharat_amd.nets import Net
    from alpharat_amd.weights import write_blob

    rng = np.random.default_rng(0)
    t = {k: v for k, v in _katago_tensors().items() if not k.startswith("blocks.")}
    shapes = {"stem.weight": (16, 7, 3, 3), "scalar_encoder.weight": (16, 6), "scalar_encoder.bias": (16,),
              "stem_bn.weight": (16,), "stem_bn.bias": (16,), "stem_bn.running_mean": (16,), "stem_bn.running_var": (16,),
              "pool_mlp.0.weight": (32, 32)}
    for k, s in shapes.items():
        t[k] = rng.standard_normal(s).astype(np.float32) ** (2 if "var" in k else 1)
    blob = write_blob(tmp_path / "c16.arnet", "cnn_katago", 7, 5, t)
    with pytest.raises(RuntimeError, match="16 trunk channels is not supported \\(supported widths: 32, 64\\)"):
        Net(blob)


def test_katago_with_a_wrongly_sized_head_is_refused(tmp_path):
    from alpharat_amd.nets import Net
    from alpharat_amd.weights import write_blob

    t = _katago_tensors()
    t["value_head.weight"] = np.zeros((3, 32), np.float32)
    with pytest.raises(RuntimeError, match=r"value_head\.weight must be \[2, 32\]"):
        Net(write_blob(tmp_path / "bad_head.arnet", "cnn_katago", 7, 5, t))
    t = _katago_tensors()
    t["blocks.1.pool_linear.bias"] = np.zeros(31, np.float32)
    with pytest.raises(RuntimeError, match=r"blocks\.1\.pool_linear\.bias must be \[32\]"):
        Net(write_blob(tmp_path / "bad_block.arnet", "cnn_katago", 7, 5, t))


def test_katago_on_a_board_of_another_size_is_refused():
    from alpharat_amd.game import PyRat
    from alpharat_amd.mcts import rust_mcts_search
    from alpharat_amd.nets import Net
    from alpharat_amd.sampling import rust_self_play

    blob = NETS / "katago_7x5_c32.arnet"
    with pytest.raises(ValueError, match="built for a 7x5 board"):
        rust_self_play(width=5, height=7, cheese_count=6, max_turns=30, num_games=2, simulations=16, output_dir=None,
                       weights_path=str(blob))
    with pytest.raises(ValueError, match="board size"):
        rust_mcts_search(PyRat.create_custom(7, 7, cheese=[(3, 3)], max_turns=30), simulations=16, net=Net(blob))
