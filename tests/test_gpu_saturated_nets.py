"""-m gpu: the evaluator kernels and the search at saturated network outputs (tests/_saturated_nets.py).

Every other network of the suite has logits of about +-1 and values of about 1, so softmax5 never saw a probability that
is a denormal or 0, softplusf never took its x > 20 branch nor an underflowing expf, and no fold met a near-dead channel.

1. Evaluators against float64. For every (architecture, family) Net(blob).evaluate(games) is compared with the float64
   restatement on the device's own encode(games). The fixed 1e-5 of test_gpu_nets.py means nothing at logits of +-100, so
   the tolerance is measured as tests/test_gpu_train.py measures its own: with E_ref = max|f32 restatement - f64| of an
   output kind (logits, values),
       max|dev - f64| <= 8 * max(E_ref, 2^-23 * max|f64 of that kind over the batch|):
   both sides are f32 evaluations of the same sums in different orders. Probabilities: where the float64 p is a normal f32
   (>= 2^-126; the issue asks it from 2^-100, the rest of the normal range is held to the same rule so that no entry goes
   unchecked) |log p_dev - log p64| <= twice the logit bound + 2^-22; where p64 < 2^-126, 0 <= p_dev <= 2^-125 (flushing
   and a denormal are both right). Every row is finite and sums to 1 within 1e-5.
2. The bit-equality claims of test_gpu_nets.py on the ``policy`` family: AR_SYM_FMA=1, AR_CNN_LDS=1, AR_MLP_FL=0/1,
   reversed leaf order.
3. Whole games with a ``policy+value+tie`` network: SelfPlaySession against O.play_game driven by the HIP evaluator on
   the same blob, record by record and counter by counter; gather / backup choices (the gather set up is asserted from
   session.info()) and the evaluation cache give the same bytes. The conditions of S.assert_saturated_records hold on the
   oracle's records: among the root priors of legal actions at least 10 below 1e-30 (0.0 included) and at least 10
   above 0.999, at least 10 roots with exactly tied top priors, a recorded value above 20.
   tests/test_saturated_nets_cpu.py asserts the same with the oracle's own network, without a device."""
import numpy as np
import pytest

import _oracle as O
import _saturated_nets as S
from _random_nets import pyrat

pytestmark = pytest.mark.gpu

KINDS = {"logits": ("logits_p1", "logits_p2"), "values": ("value_p1", "value_p2")}


@pytest.fixture(scope="module")
def blobs(tmp_path_factory):
    """(blob path, tensors) per (architecture, family), written when first asked for"""
    d = tmp_path_factory.mktemp("saturated")
    made = {}

    def get(name, kind):
        if (name, kind) not in made:
            made[name, kind] = (S.write(d / f"{name}_{kind.replace('+', '_')}.arnet", name, kind), S.family(name, kind))
        return made[name, kind]

    return get


@pytest.fixture(scope="module")
def games():
    made = {}

    def get(name):
        if name not in made:
            made[name] = [pyrat(og) for og in S.family_positions(name)]
        return made[name]

    return get


def _err(a, b, keys):
    return max(float(np.abs(np.asarray(a[k], np.float64) - b[k]).max()) for k in keys)


# ---- 1. evaluators against float64 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", S.FAMILIES)
@pytest.mark.parametrize("name", S.ARCHS)
def test_evaluator_against_float64(name, kind, blobs, games):
    from alpharat_amd.nets import Net, encode

    blob, t = blobs(name, kind)
    obs = encode(games(name))
    got = Net(blob).evaluate(games(name))
    f64 = S.forward(name, t, obs)
    f32 = S.forward(name, t, obs, dtype=np.float32)
    bound = {}
    for what, keys in KINDS.items():
        e_ref = _err(f32, f64, keys)
        top = max(float(np.abs(f64[k]).max()) for k in keys)
        bound[what] = 8.0 * max(e_ref, 2.0 ** -23 * top)
        err = _err(got, f64, keys)
        print(f"{name} {kind} {what}: E_ref {e_ref:.3e} device {err:.3e} bound {bound[what]:.3e} (max|f64| {top:.3e})")
        assert err <= bound[what], (what, err, bound[what])
    for k in ("policy_p1", "policy_p2"):
        p, p64 = got[k].astype(np.float64), f64[k]
        assert np.isfinite(got[k]).all() and np.abs(p.sum(axis=1) - 1).max() <= 1e-5, k
        normal = p64 >= 2.0 ** -126
        with np.errstate(divide="ignore"):
            dlog = np.abs(np.log(p[normal]) - np.log(p64[normal]))
        print(f"{name} {kind} {k}: max|dlog p| {dlog.max():.3e} bound {2 * bound['logits'] + 2.0 ** -22:.3e}; "
              f"{int((~normal).sum())} entries below 2^-126, device max there {p[~normal].max() if (~normal).any() else 0:.3e}")
        assert (dlog <= 2 * bound["logits"] + 2.0 ** -22).all(), (k, dlog.max())
        assert ((p[~normal] >= 0) & (p[~normal] <= 2.0 ** -125)).all(), k
    for k in KINDS["values"]:
        assert np.isfinite(got[k]).all() and (got[k] >= 0).all(), k


# ---- 2. the bit-equality claims, on saturated outputs ------------------------------------------------------------------------
def _same_bits(a, b, what):
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("name", S.ARCHS)
def test_leaf_order_does_not_change_the_bits(name, blobs, games):
    from alpharat_amd.nets import Net

    net = Net(blobs(name, "policy")[0])
    a = net.evaluate(games(name))
    b = net.evaluate(games(name)[::-1])
    _same_bits(a, {k: v[::-1] for k, v in b.items()}, "reversed")


def test_symmetric_fma_loops_give_the_same_bits(blobs, games, monkeypatch):
    from alpharat_amd.nets import Net

    name = "symmetric_5x5_h32"
    net = Net(blobs(name, "policy")[0])
    a = net.evaluate(games(name))
    monkeypatch.setenv("AR_SYM_FMA", "1")
    _same_bits(a, net.evaluate(games(name)), "AR_SYM_FMA=1")


@pytest.mark.parametrize("name", ["cnn_7x7_c32_pooled", "cnn_7x7_c64_gpool"])
def test_cnn_three_image_kernel_gives_the_same_bits(name, blobs, games, monkeypatch):
    from alpharat_amd.nets import Net

    blob = blobs(name, "policy")[0]
    a = Net(blob).evaluate(games(name))
    monkeypatch.setenv("AR_CNN_LDS", "1")  # chosen when the weights are loaded
    _same_bits(a, Net(blob).evaluate(games(name)), "AR_CNN_LDS=1")


def test_mlp_first_layer_variants_give_the_same_bits(blobs, games, monkeypatch):
    from alpharat_amd.nets import Net

    name = "mlp_5x5_h32"
    net = Net(blobs(name, "policy")[0])
    a = net.evaluate(games(name))
    for fl in ("0", "1"):
        monkeypatch.setenv("AR_MLP_FL", fl)
        _same_bits(a, net.evaluate(games(name)), f"AR_MLP_FL={fl}")


# ---- 3. whole games ----------------------------------------------------------------------------------------------------------
GATHER_KIND = {"lane": 0, "octet": 1, "wide": 2}  # ArSessionInfo.gather_kind


def _play(name, blob, noise, monkeypatch=None, env=None, gather="wide", **kw):
    """the 16 games of tests/_saturated_nets.py on the device, after checking that the gather asked for is the one set up"""
    from alpharat_amd.sampling import SelfPlaySession

    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    _, w, h, _ = S.ARCHS[name]
    got = {}
    with SelfPlaySession(width=w, height=h, cheese_count=S.GAME_BOARDS[name], max_turns=S.TURNS, num_games=S.GAMES,
                         simulations=S.SIMS, batch_size=S.BATCH, output_dir=None, seed=S.SEED, weights_path=str(blob),
                         noise_epsilon=noise, on_game=lambda g: got.__setitem__(g["game_index"], g), **kw) as s:
        assert s.info()["gather_kind"] == GATHER_KIND[gather], (env, s.info())
        while not s.finished:
            s.step(1024)
        stats = s.close()
    for k in env or {}:
        monkeypatch.delenv(k)
    assert sorted(got) == list(range(S.GAMES))
    return got, stats


def _same_records(a, b, what):
    for i, g in a.items():
        for k, v in g.items():
            if isinstance(v, np.ndarray):
                assert v.tobytes() == b[i][k].tobytes(), (what, i, k)
            else:
                assert v == b[i][k], (what, i, k)


@pytest.mark.parametrize("noise", [0.0, 0.25])
@pytest.mark.parametrize("name", S.GAME_BOARDS)
def test_whole_games_match_the_oracle(name, noise, blobs, monkeypatch):
    """the default kernels of the network path: the work-queue gather and k_backup16"""
    from test_gpu_pipeline_parity import HipEvaluator, _check_game

    monkeypatch.delenv("AR_GATHER", raising=False)
    monkeypatch.delenv("AR_BACKUP", raising=False)
    blob = blobs(name, "policy+value+tie")[0]
    got, stats = _play(name, blob, noise)
    _, w, h, _ = S.ARCHS[name]
    ev = HipEvaluator(blob, w, h, S.TURNS)
    wants = S.oracle_games(name, noise, ev.backend, 4)
    S.assert_saturated_records(wants)
    for i, want in enumerate(wants):
        _check_game(got[i], want)
    for k in ("total_simulations", "total_nn_evals", "total_terminals", "total_collisions"):
        assert getattr(stats, k) == sum(w_[k] for w_ in wants), k


def test_whole_games_do_not_depend_on_gather_backup_or_cache(blobs, monkeypatch):
    name = "mlp_5x5_h32"
    monkeypatch.delenv("AR_GATHER", raising=False)
    monkeypatch.delenv("AR_BACKUP", raising=False)
    blob = blobs(name, "policy+value+tie")[0]
    for noise in (0.0, 0.25):
        base, _ = _play(name, blob, noise)
        for env, gather in ((dict(AR_BACKUP="lane"), "wide"), (dict(AR_GATHER="lane"), "lane"), (dict(AR_GATHER="octet"), "octet")):
            _same_records(base, _play(name, blob, noise, monkeypatch, env, gather)[0], (noise, env))
    cached, stats = _play(name, blob, 0.25, cache_size=4096)
    assert stats.cache_hits > 0
    _same_records(base, cached, "cache_size=4096")
