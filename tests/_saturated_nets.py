"""Networks whose outputs saturate: seeded transforms of the suite's tame test networks -- test infrastructure only.

Every network the other tests evaluate has logits of about +-1 and values of about 1. The three families here change only
the heads and the BatchNorm tensors of such a network, so the result is still a checkpoint of its architecture:

- ``policy``: every policy row gets ``GAIN * U[a] * (g . x - OFFSET)`` added, x the head's input, g a seeded direction.
  Over the family's 70 positions the per-player logit spread (max - min) then lies below 20 for some rows, in 88..103
  (the smallest probability is an f32 denormal) for others and above 104 (exactly 0 in f32) for the rest.
- ``value``: the value row becomes ``CENTRE + A x_j - B x_k - C x_l + NOISE g . x``, x_j, x_k, x_l three ReLU units of the head's input.
  Where all three are off the pre-softplus value is within +-0.5 of 20 (on both sides, from the noise): softplusf's
  threshold. Unit j lifts it above 89 (expf overflows if the threshold is missing), unit k pushes it below -90 (expf
  underflows), unit l brings it back to the ordinary range, |v| < 10, where both terms of log1p(exp(v)) count.
- ``deadbn``: a quarter of the channels of every BatchNorm have running_var 1e-10 (the folded scale is
  weight / sqrt(1e-5 + 1e-10), about 316 times the weight) and a running_mean within 1e-3 of the one they had, which is
  the layer's typical pre-activation. Their pre-activations are not constant as a trained dead channel's are, so the
  channels' weights are multiplied by ``dead_gamma``, the largest power of two that keeps the float64 logits below 1e3 (the
  deeper the network, the smaller); heads stay as they were.

The constants in TUNED were found on the CPU by ``python tests/_saturated_nets.py`` (tune(), below) so that the float64
restatement alone puts at least four of the 70 x 2 player outputs into every band; tests/test_saturated_nets_cpu.py
asserts that, so a change of the base networks or the positions that empties a band fails there and not silently.
"""
from __future__ import annotations

import functools
from pathlib import Path

import numpy as np

import _cnn_np
import _katago_np
import _mlp_np
from _random_nets import positions, random_mlp, random_symmetric, transplant

GOLD = Path(__file__).resolve().parent / "golden"
N_POSITIONS = 70  # two full 32-leaf tiles and a ragged one
FAMILIES = ("policy", "value", "deadbn")
KEYS = ("logits_p1", "logits_p2", "policy_p1", "policy_p2", "value_p1", "value_p2")

# name: (architecture, width, height, tensors)
ARCHS = {
    "mlp_5x5_h32": ("mlp", 5, 5, lambda: random_mlp(5, 5, 32, 101)),             # k_mlp_mfma
    "mlp_5x5_h48": ("mlp", 5, 5, lambda: random_mlp(5, 5, 48, 102)),             # scalar tile loops
    "symmetric_5x5_h32": ("symmetric", 5, 5, lambda: random_symmetric(5, 5, 32, 103)),
    "cnn_7x5_c16": ("cnn", 7, 5, lambda: transplant(GOLD / "nets" / "cnn_gpool_7x5_c16.arnet", 7, 5)[1]),   # FMA kernel
    "cnn_7x7_c32_pooled": ("cnn", 7, 7, lambda: transplant(GOLD / "nets" / "cnn_pooled_7x7_c32.arnet", 7, 7)[1]),
    "cnn_7x7_c64_gpool": ("cnn", 7, 7, lambda: transplant(GOLD / "nets" / "cnn_gpool_7x7_c64.arnet", 7, 7)[1]),
    "katago_7x5_c32": ("cnn_katago", 7, 5, lambda: transplant(GOLD / "nets_katago" / "katago_7x5_c32.arnet", 7, 5)[1]),
}

U = np.array([1.0, -1.0, 0.375, -0.625, 0.125])  # what the gate adds to the five logits: a spread of 2 per unit of gate
DEAD_VAR = 1e-10
BANDS_POLICY = ("spread < 20", "88 <= spread <= 103", "spread > 104")
BANDS_VALUE = ("19.5 <= v < 20", "20 < v <= 20.5", "v > 89", "v < -90", "|v| < 10")

# policy: (OFFSET, GAIN); value: (j, k, l, A, B, C, NOISE, CENTRE) -- python tests/_saturated_nets.py
TUNED = {
    "mlp_5x5_h32": dict(policy=(0.36245623230934143, 82.6066665649414),
        value=(11, 31, 15, 282.2113342285156, 708.3343505859375,
               61.5181999206543, 0.019999999552965164, 19.999265670776367), dead_gamma=0.125),
    "mlp_5x5_h48": dict(policy=(-0.4883875846862793, 91.64903259277344),
        value=(1, 4, 47, 164.30624389648438, 375.8819885253906,
               115.99308776855469, 0.800000011920929, 19.72150993347168), dead_gamma=0.125),
    "symmetric_5x5_h32": dict(policy=(0.09971247613430023, 221.6085662841797),
        value=(45, 31, 59, 148.97840881347656, 579.1675415039062,
               124.65290069580078, 0.019999999552965164, 20.004562377929688), dead_gamma=0.03125),
    "cnn_7x5_c16": dict(policy=(-2.779048442840576, 56.44189453125),
        value=(25, 0, 16, 51.283023834228516, 118.48182678222656,
               19.699066162109375, 0.019999999552965164, 19.962793350219727), dead_gamma=0.03125),
    "cnn_7x7_c32_pooled": dict(policy=(0.558211088180542, 25.89737319946289),
        value=(19, 31, 18, 68.3829345703125, 225.43199157714844,
               131.87051391601562, 0.019999999552965164, 20.013473510742188), dead_gamma=0.015625),
    "cnn_7x7_c64_gpool": dict(policy=(-7.663400173187256, 14.128557205200195),
        value=(20, 9, 38, 25.779386520385742, 56.3913459777832,
               5.796771049499512, 0.019999999552965164, 19.99868392944336), dead_gamma=0.0078125),
    "katago_7x5_c32": dict(policy=(5.372305870056152, 39.237998962402344),
        value=(11, 7, 14, 53.09033203125, 110.80033874511719,
               264.000244140625, 0.019999999552965164, 20.036800384521484), dead_gamma=0.015625),
}


def base(name: str) -> dict:
    return {k: np.array(v, np.float32) for k, v in ARCHS[name][3]().items()}


@functools.lru_cache(maxsize=None)
def family_positions(name: str) -> tuple:
    """the family's 70 oracle games (tests/_random_nets.py positions), one maze each"""
    _, w, h, _ = ARCHS[name]
    return tuple(positions(w, h, N_POSITIONS, seed=7000 + 10 * w + h))


def forward(name: str, tensors: dict, obs: np.ndarray, dtype=np.float64, taps: dict | None = None) -> dict:
    arch, w, h, _ = ARCHS[name]
    if arch == "mlp":
        return _mlp_np.mlp_forward(tensors, obs, dtype, taps)
    if arch == "symmetric":
        return _mlp_np.symmetric_forward(tensors, w, h, obs, dtype, taps)
    return (_cnn_np if arch == "cnn" else _katago_np).forward(tensors, w, h, obs, dtype, taps)


def _heads(arch: str, t: dict) -> tuple:
    """([(policy tensor, its five rows)], [(value tensor, its row)]): one entry per player where the players have rows of
    their own, one for both where they share the head"""
    if arch == "mlp":
        return [("policy_p1_head", slice(0, 5)), ("policy_p2_head", slice(0, 5))], [("value_head", 0), ("value_head", 1)]
    if arch == "symmetric":
        return [("policy_head", slice(0, 5))], [("value_head", 0)]
    if arch == "cnn":
        return [("policy_head.linear", slice(0, 5))], [("value_head.linear" if "value_head.linear.weight" in t else "value_head.mlp.2", 0)]
    return [("policy_head", slice(0, 5)), ("policy_head", slice(5, 10))], [("value_head", 0), ("value_head", 1)]


def _gates(name: str, kind: str, n_rows: int, dim: int) -> np.ndarray:
    """the seeded directions of a family: one per head entry"""
    rng = np.random.default_rng([sorted(ARCHS).index(name), FAMILIES.index(kind), 20260])
    return rng.standard_normal((n_rows, dim)) / np.sqrt(dim)


def saturate_policy(name: str, t: dict, offset: float, gain: float) -> dict:
    t = dict(t)
    heads = _heads(ARCHS[name][0], t)[0]
    for (key, rows), g in zip(heads, _gates(name, "policy", len(heads), t[heads[0][0] + ".weight"].shape[1])):
        w, b = t[key + ".weight"].astype(np.float64), t[key + ".bias"].astype(np.float64)
        w[rows] += gain * np.outer(U, g)
        b[rows] -= gain * offset * U
        t[key + ".weight"], t[key + ".bias"] = w.astype(np.float32), b.astype(np.float32)
    return t


def saturate_value(name: str, t: dict, j: int, k: int, l: int, a: float, b: float, c: float, noise: float, centre: float) -> dict:
    t = dict(t)
    heads = _heads(ARCHS[name][0], t)[1]
    for (key, row), g in zip(heads, _gates(name, "value", len(heads), t[heads[0][0] + ".weight"].shape[1])):
        w, bias = t[key + ".weight"].astype(np.float64), t[key + ".bias"].astype(np.float64)
        w[row] = noise * g
        w[row, j] += a
        w[row, k] -= b
        w[row, l] -= c
        bias[row] = centre
        t[key + ".weight"], t[key + ".bias"] = w.astype(np.float32), bias.astype(np.float32)
    return t


def dead_bn(name: str, t: dict, dead_gamma: float) -> dict:
    t = dict(t)
    rng = np.random.default_rng([sorted(ARCHS).index(name), FAMILIES.index("deadbn"), 20260])
    for key in sorted(k[: -len(".running_var")] for k in t if k.endswith(".running_var")):
        n = t[key + ".running_var"].shape[0]
        dead = np.sort(rng.permutation(n)[: n // 4])
        var, mean, gamma = (t[key + s].copy() for s in (".running_var", ".running_mean", ".weight"))
        var[dead] = DEAD_VAR
        mean[dead] += rng.uniform(-1e-3, 1e-3, len(dead)).astype(np.float32)
        gamma[dead] *= dead_gamma
        t[key + ".running_var"], t[key + ".running_mean"], t[key + ".weight"] = var, mean, gamma
    return t


def tie_policy(name: str, t: dict) -> dict:
    """the row of action 2 becomes a copy of the row of action 0 in every policy block: the two logits are the same sum, so
    their priors are tied exactly, at 0.5 each where the gate is far above its offset (action 1 keeps the lowest logit
    there, so the priors below 1e-30 stay)"""
    t = dict(t)
    for key, rows in _heads(ARCHS[name][0], t)[0]:
        w, b = t[key + ".weight"].copy(), t[key + ".bias"].copy()
        w[rows.start + 2], b[rows.start + 2] = w[rows.start], b[rows.start]
        t[key + ".weight"], t[key + ".bias"] = w, b
    return t


def family(name: str, kind: str) -> dict:
    """the tensors of one family of one architecture; ``policy+value`` is both head transforms on one network, ``+tie``
    adds tie_policy"""
    t = base(name)
    if "policy" in kind:
        t = saturate_policy(name, t, *TUNED[name]["policy"])
    if "tie" in kind:
        t = tie_policy(name, t)
    if "value" in kind:
        t = saturate_value(name, t, *TUNED[name]["value"])
    if kind == "deadbn":
        t = dead_bn(name, t, TUNED[name]["dead_gamma"])
    return t


def write(path, name: str, kind: str) -> Path:
    from alpharat_amd.weights import write_blob

    arch, w, h, _ = ARCHS[name]
    return write_blob(path, arch, w, h, family(name, kind))


# ---- whole games with a ``policy+value+tie`` network --------------------------------------------------------------------
GAMES, SIMS, BATCH, TURNS, SEED = 16, 64, 16, 12, 3
GAME_BOARDS = {"mlp_5x5_h32": 5, "symmetric_5x5_h32": 5, "cnn_7x5_c16": 7}  # name: cheese


def oracle_games(name: str, noise: float, net, backend: int) -> list:
    """the 16 games as the oracle plays them with the given evaluator (2: the oracle's own net, 4: a callback)"""
    import _oracle as O

    _, w, h, _ = ARCHS[name]
    cfg = O.make_config(noise_epsilon=noise)
    return [O.play_game(O.Game(w, h, TURNS).random_cheese(GAME_BOARDS[name], True, SEED + i), cfg, SIMS, BATCH,
                        0xA1FA0000 + SEED + i, backend=backend, net=net, game_index=i) for i in range(GAMES)]


def legal_priors(want: dict) -> list:
    """per recorded position and player of one oracle game: (the five root priors, the legal actions) -- STAY, and a
    direction with no wall for a player that is not in mud"""
    out = []
    for i in range(want["n"]):
        for p in range(2):
            x, y = want["ints"][i, 2 * p: 2 * p + 2]
            stuck = want["ints"][i, 4 + p] != 0
            legal = [d for d in range(4) if not stuck and want["maze"][y, x, d] >= 0] + [4]
            out.append((want["floats"][i, 14 + 5 * p: 19 + 5 * p], legal))
    return out


def assert_saturated_records(wants: list) -> None:
    """the conditions on the oracle's records: among the root priors of legal actions at least 10 below 1e-30 (0.0
    included) and at least 10 above 0.999; at least 10 roots whose two largest legal priors are tied exactly; a recorded
    value above 20"""
    rows = [r for w in wants for r in legal_priors(w)]
    pri = np.array([p[a] for p, legal in rows for a in legal], np.float32)
    ties = sum(1 for p, legal in rows if len(legal) > 1 and np.sort(p[legal])[-1] == np.sort(p[legal])[-2])
    values = np.concatenate([w["floats"][:, 2:4].reshape(-1) for w in wants])
    print(f"legal root priors: {len(pri)}, {int((pri < 1e-30).sum())} below 1e-30 ({int((pri == 0).sum())} zero), "
          f"{int((pri > 0.999).sum())} above 0.999; {ties} roots with tied top priors; max value {values.max():.3f}")
    assert (pri < 1e-30).sum() >= 10 and (pri > 0.999).sum() >= 10
    assert ties >= 10
    assert values.max() > 20


# ---- the bands -----------------------------------------------------------------------------------------------------------
def spreads(out: dict) -> np.ndarray:
    """per-player logit spreads, 2n of them"""
    return np.concatenate([out[k].max(axis=1) - out[k].min(axis=1) for k in ("logits_p1", "logits_p2")])


def prevalues(name: str, t: dict, obs: np.ndarray) -> np.ndarray:
    """the pre-softplus values of tensors `t` in float64, 2n of them: the value rows over their inputs"""
    taps = {}
    forward(name, t, obs, taps=taps)
    return _head_outputs(name, t, taps)["prevalues"]


def policy_bands(sp: np.ndarray) -> dict:
    return dict(zip(BANDS_POLICY, (int((sp < 20).sum()), int(((sp >= 88) & (sp <= 103)).sum()), int((sp > 104).sum()))))


def value_bands(v: np.ndarray) -> dict:
    return dict(zip(BANDS_VALUE, (int(((v >= 19.5) & (v < 20)).sum()), int(((v > 20) & (v <= 20.5)).sum()),
                                  int((v > 89).sum()), int((v < -90).sum()), int((np.abs(v) < 10).sum()))))


# ---- finding the constants ---------------------------------------------------------------------------------------------
def _head_outputs(name: str, t: dict, taps: dict) -> dict:
    """logits and pre-softplus values of tensors `t` from the head inputs of one forward of the base network"""
    pol, val = _heads(ARCHS[name][0], t)

    def rows(heads, p, x):
        key, r = heads[p % len(heads)]  # a shared head serves both players
        return x @ t[key + ".weight"][r].astype(np.float64).T + t[key + ".bias"][r]

    lg = [rows(pol, p, taps["policy"][p]) for p in range(2)]
    return dict(logits_p1=lg[0], logits_p2=lg[1], prevalues=np.concatenate([rows(val, p, taps["value"][p]) for p in range(2)]))


def tune(name: str) -> dict:
    """the constants of TUNED for one architecture: one forward of the base network, then the heads alone"""
    obs = np.stack([og.encode() for og in family_positions(name)])
    t = base(name)
    taps = {}
    forward(name, t, obs, taps=taps)
    # policy: the gate is centred on its median; the gain that fills the emptiest band best
    heads = _heads(ARCHS[name][0], t)[0]
    g = _gates(name, "policy", len(heads), taps["policy"][0].shape[1])
    z = np.concatenate([taps["policy"][0] @ g[0], taps["policy"][1] @ g[-1]])
    offset = float(np.float32(np.median(z)))
    best = None
    for gain in np.geomspace(5, 5000, 400):
        gain = float(np.float32(gain))
        c = min(policy_bands(spreads(_head_outputs(name, saturate_policy(name, t, offset, gain), taps))).values())
        if best is None or c > best[0]:
            best = (c, gain)
    policy = (offset, best[1])
    # value: three units that are each on often enough, and off together often enough
    x = np.concatenate(taps["value"])
    on = x > 1e-9
    frac = on.mean(axis=0)
    gv = _gates(name, "value", len(_heads(ARCHS[name][0], t)[1]), x.shape[1])
    gz = np.concatenate([taps["value"][0] @ gv[0], taps["value"][1] @ gv[-1]])
    cand = [int(i) for i in np.argsort(np.abs(frac - 0.3)) if 0.04 < frac[i] < 0.8][:16]
    best = None
    for j in cand:
        for k in cand:
            for l in cand:
                if len({j, k, l}) < 3:
                    continue
                a = 80.0 / np.percentile(x[on[:, j], j], 70)
                b = 125.0 / np.percentile(x[on[:, k], k], 70)
                c = 20.0 / np.median(x[on[:, l], l])
                off = ~(on[:, j] | on[:, k] | on[:, l])
                if off.sum() < 8:
                    continue
                for noise in (0.02, 0.05, 0.1, 0.2, 0.4, 0.8):
                    centre = 20.0 - noise * float(np.median(gz[off]))
                    args = (j, k, l, *(float(np.float32(q)) for q in (a, b, c, noise, centre)))
                    v = _head_outputs(name, saturate_value(name, t, *args), taps)["prevalues"]
                    score = min(value_bands(v).values()) - (100 if np.abs(v).max() > 900 else 0)
                    if best is None or score > best[0]:
                        best = (score, args)
    dead_gamma = 1.0
    while max(np.abs(o).max() for o in list(forward(name, dead_bn(name, t, dead_gamma), obs).values())[:2]) >= 1e3:
        dead_gamma /= 2
    return dict(policy=policy, value=best[1], dead_gamma=dead_gamma)


if __name__ == "__main__":
    import sys

    for _name in sys.argv[1:] or ARCHS:
        _c = tune(_name)
        _obs = np.stack([og.encode() for og in family_positions(_name)])
        _p = forward(_name, saturate_policy(_name, base(_name), *_c["policy"]), _obs)
        _d = forward(_name, dead_bn(_name, base(_name), _c["dead_gamma"]), _obs)
        print(f'    "{_name}": dict(policy={_c["policy"]!r}, value={_c["value"]!r}, dead_gamma={_c["dead_gamma"]!r}),')
        print("    #", policy_bands(spreads(_p)), value_bands(prevalues(_name, saturate_value(_name, base(_name), *_c["value"]), _obs)), "deadbn max|logit|",
              max(np.abs(_d[k]).max() for k in ("logits_p1", "logits_p2")), flush=True)
