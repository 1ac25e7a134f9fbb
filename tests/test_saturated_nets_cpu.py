"""CPU: what tests/test_gpu_saturated_nets.py stands on, before any GPU run.

- tests/_cnn_np.py, the float64 PyRatCNN, against every tests/golden/nets/cnn_*.npz (made by the reference's own class), at
  the project's 1e-5 on logits, policies and values.
- The band conditions of tests/_saturated_nets.py, from the float64 restatement alone: for every architecture, each band
  of logit spreads and of pre-softplus values holds at least 4 of the 70 x 2 player outputs, a quarter of every BatchNorm's
  channels is near-dead, and the ``deadbn`` logits stay below 1e3.
- The whole games of the GPU test, played by the oracle with its own network: root priors of 0.0, denormal and above 0.999
  on legal actions, exactly tied top priors, values above 20.
- The float32 run of each restatement (the E_ref of the GPU test) is close to the float64 one on a tame network, and the
  oracle's forward agrees with the float64 restatement on the saturated ones where that is well defined."""
from pathlib import Path

import numpy as np
import pytest

import _cnn_np
import _oracle as O
import _saturated_nets as S

GOLD = Path(__file__).parent / "golden" / "nets"
MIN_IN_BAND = 4


@pytest.mark.parametrize("path", sorted(GOLD.glob("cnn_*.npz")), ids=lambda p: p.stem)
def test_cnn_np_matches_the_reference_outputs(path):
    from alpharat_amd.weights import read_blob

    gold = np.load(path)
    arch, w, h, t = read_blob(path.with_suffix(".arnet"))
    assert arch == "cnn"
    got = _cnn_np.forward(t, w, h, gold["obs"])
    for k in S.KEYS:
        np.testing.assert_allclose(got[k], gold[k], atol=1e-5, rtol=1e-5, err_msg=f"{path.stem}:{k}")
    got32 = _cnn_np.forward(t, w, h, gold["obs"], dtype=np.float32)
    assert all(got32[k].dtype == np.float32 for k in S.KEYS)
    for k in S.KEYS:
        np.testing.assert_allclose(got32[k], gold[k], atol=1e-5, rtol=1e-5, err_msg=f"{path.stem}:{k} (float32)")


@pytest.fixture(scope="module")
def observations():
    made = {}

    def get(name):
        if name not in made:
            made[name] = np.stack([og.encode() for og in S.family_positions(name)])
        return made[name]

    return get


@pytest.mark.parametrize("name", S.ARCHS)
def test_policy_family_fills_every_spread_band(name, observations):
    out = S.forward(name, S.family(name, "policy"), observations(name))
    bands = S.policy_bands(S.spreads(out))
    print(name, bands)
    assert all(c >= MIN_IN_BAND for c in bands.values()), bands
    p = np.concatenate([out["policy_p1"], out["policy_p2"]])
    assert (p < 2.0 ** -149).sum() >= MIN_IN_BAND and ((p >= 2.0 ** -149) & (p < 2.0 ** -126)).sum() >= MIN_IN_BAND
    assert (p > 0.999).sum() >= MIN_IN_BAND


@pytest.mark.parametrize("name", S.ARCHS)
def test_value_family_fills_every_value_band(name, observations):
    v = S.prevalues(name, S.family(name, "value"), observations(name))
    bands = S.value_bands(v)
    print(name, bands, "min", v.min(), "max", v.max())
    assert all(c >= MIN_IN_BAND for c in bands.values()), bands
    assert np.abs(v).max() < 1e3


@pytest.mark.parametrize("name", S.ARCHS)
def test_combined_family_keeps_both_sets_of_bands(name, observations):
    t = S.family(name, "policy+value")
    assert all(c >= MIN_IN_BAND for c in S.policy_bands(S.spreads(S.forward(name, t, observations(name)))).values())
    assert all(c >= MIN_IN_BAND for c in S.value_bands(S.prevalues(name, t, observations(name))).values())


@pytest.mark.parametrize("name", S.ARCHS)
def test_deadbn_family_has_dead_channels_and_bounded_logits(name, observations):
    t0, t = S.base(name), S.family(name, "deadbn")
    bns = [k for k in t if k.endswith(".running_var")]
    assert bns
    for k in bns:
        dead = t[k] == np.float32(S.DEAD_VAR)
        assert dead.sum() == len(dead) // 4, k
        mean = k.replace("running_var", "running_mean")
        assert np.abs(t[mean] - t0[mean]).max() <= 1e-3 + 1e-7 and (t[mean][dead] != t0[mean][dead]).any(), k
        assert np.array_equal(t[k][~dead], t0[k][~dead]), k
    for k in t:
        if "head" in k:
            assert np.array_equal(t[k], t0[k]), k
    out, tame = S.forward(name, t, observations(name)), S.forward(name, t0, observations(name))
    top = max(np.abs(out[k]).max() for k in ("logits_p1", "logits_p2"))
    print(name, "max |logit|", top, "tame", max(np.abs(tame[k]).max() for k in ("logits_p1", "logits_p2")))
    assert top < 1e3
    assert np.abs(out["logits_p1"] - tame["logits_p1"]).max() > 1.0  # the dead channels reach the outputs


@pytest.mark.parametrize("name", [n for n in S.ARCHS if S.ARCHS[n][0] != "cnn_katago"])  # (the oracle has no KataGoCNN)
def test_families_are_blobs_the_oracle_reads(name, observations, tmp_path):
    """each family is a valid checkpoint of its architecture: the oracle loads it, and its f32 forward is near the float64
    one (logits relative to their size)"""
    for kind in S.FAMILIES + ("policy+value",):
        blob = S.write(tmp_path / f"{name}_{kind}.arnet", name, kind)
        got = O.Net(blob).forward(observations(name))
        want = S.forward(name, S.family(name, kind), observations(name))
        for k in ("logits_p1", "logits_p2"):
            scale = np.abs(want[k]).max()
            assert np.abs(got[k] - want[k]).max() <= 1e-4 * scale, (kind, k)
        assert all(np.isfinite(got[k]).all() for k in S.KEYS), kind


@pytest.mark.parametrize("noise", [0.0, 0.25])
@pytest.mark.parametrize("name", S.GAME_BOARDS)
def test_whole_games_meet_saturated_priors_ties_and_values(name, noise, tmp_path):
    """the games of tests/test_gpu_saturated_nets.py played by the oracle with its own forward of the same blob
    (backend 2): the conditions on root priors and values hold without trusting the device"""
    blob = S.write(tmp_path / f"{name}.arnet", name, "policy+value+tie")
    S.assert_saturated_records(S.oracle_games(name, noise, O.Net(blob), 2))
