"""The tree code at the edges of what an evaluator may return, through the callback: priors of exactly 0.0 and 1.0,
denormal priors, exact ties, values of 0, of 1e-40 and of 1e4.

Every other search test feeds the tree uniform priors, a tame network's, or the constant (1.5, 0.5) callback, so
reduce_prior, the PUCT score and its forced-playout threshold sqrt(force_k * prior * visits), compute_fpu, the Welford
updates of the backups, policy pruning and the Dirichlet mixing never saw such inputs. One pure function from a leaf to
(p1, p2, v1, v2), keyed on a CRC of positions, turn, mud and cheese, is given to the oracle as its CallbackBackend and to
rust_mcts_search as predict_fn; results must be equal bit for bit (_assert_result of tests/test_gpu_parity.py).

It stays within what a network can emit: priors in [0, 1] on legal actions that sum to 1 within 1e-6, values in [0, 1e4],
no NaN, no Inf. Two regimes, because with both at once the 1e4 values decide everything and every root collapses to one
action:
- ``priors``: degenerate priors (PATTERNS) with ordinary values (0, 1e-30, 0.5, nextafter(0.5), 1.5, 3);
- ``values``: ordinary priors with extreme values (0, 1e-40, 20, 1e4, 0.5, 7).
The searched root itself gets an ordinary prior in both.

Which kernels this reaches: a search with a predict_fn always runs the one-lane-per-game gather and backup (k_gather,
k_backup); AR_GATHER and AR_BACKUP are read on the network path only, so they are not varied here. The work-queue and
eight-lane gathers and k_backup16 meet priors of 0.0, denormals, priors above 0.999, exact ties and values of 0 to 125
through the whole games of tests/test_gpu_saturated_nets.py, which asserts the kernel chosen; values of 1e4 and the
``1 - 2^-24`` prior reach only the kernels of this file. In the ``values`` regime every root keeps one action after
pruning, so pruning and the Dirichlet mixing act on more than one action only with the values of the ``priors`` regime.

Two conditions are asserted from counts kept in the callback on the oracle's side alone (no GPU needed): every (pattern,
value) class is met at least 10 times per regime, and in at least half of the searches with noise (all of the ``priors``
regime's; see test_noise_on_roots_keep_more_than_one_action) each player's root has two or more visited actions."""
import zlib
from collections import Counter

import numpy as np
import pytest

import _oracle as O

F = np.float32
PATTERNS = ("one-hot", "tie", "denormals beside 1.0", "1 - 2^-24 beside 1e-30s", "uniform", "0.75 / 0.25")
VALUES = {"priors": (F(0), F(1e-30), F(0.5), np.nextafter(F(0.5), F(1)), F(1.5), F(3)),
          "values": (F(0), F(1e-40), F(20), F(1e4), F(0.5), F(7))}
TUNED = dict(c_puct=0.512, fpu_reduction=0.459, force_k=0.103)
SIMS = 400


def _positions():
    yield "5x5 open", O.Game(5, 5, 100, p1=(0, 0), p2=(4, 4), cheese=[(2, 2), (1, 3), (3, 1), (4, 0), (0, 3)]), 100
    yield "7x7 maze", O.Game(7, 7, 50).random_maze(0.5, 0.3, True, 17).random_cheese(10, True, 5), 50


def _key(p1, p2, turn, m1, m2, cheese) -> int:
    head = bytes([p1[0], p1[1], p2[0], p2[1], turn & 255, turn >> 8, m1, m2])
    return zlib.crc32(head + np.ascontiguousarray(cheese, np.uint8).tobytes())


def _legal(cost, pos, mud):
    """the distinct effective actions of a player: STAY, and the open directions unless it is stuck in mud"""
    return ([d for d in range(4) if cost[pos[1], pos[0], d]] if mud == 0 else []) + [4]


def _ordinary(c, legal):
    w = np.array([1 + ((c >> (3 * a + 5)) & 7) for a in legal], F)
    p = np.zeros(5, F)
    p[legal] = w / w.sum(dtype=F)
    return p


def _degenerate(pattern, c, legal):
    p = np.zeros(5, F)
    k = len(legal)
    a = legal[(c >> 20) % k]
    b = legal[((c >> 20) % k + 1 + (c >> 24) % max(k - 1, 1)) % k]  # another legal action where there is one
    if pattern == 0 or k == 1:
        p[a] = 1
    elif pattern == 1:
        p[a] = p[b] = 0.5
    elif pattern == 2:
        p[legal] = F(1e-40)
        p[a] = 1
    elif pattern == 3:
        p[legal] = F(1e-30)
        p[a] = F(1 - 2.0 ** -24)
    elif pattern == 4:
        p[legal] = F(1) / F(k)
    else:
        p[a], p[b] = 0.75, 0.25
    return p


class Adversary:
    """the evaluator of one (regime, root): a pure function of the leaf, with counts of the classes it met"""

    def __init__(self, regime, og):
        self.regime = regime
        self.w, self.h = og.w, og.h
        self.cost = og.cost()
        st = og.state()
        self.root = _key(st["p1"], st["p2"], st["turn"], st["p1_mud"], st["p2_mud"], og.cheese_mask())
        self.classes = Counter()

    def leaf(self, p1, p2, turn, m1, m2, cheese):
        c = _key(p1, p2, turn, m1, m2, cheese)
        out = []
        for player, (pos, mud) in enumerate(((p1, m1), (p2, m2))):
            bits = c >> (5 * player)
            pattern, value = bits % 6, (bits // 6) % 6
            legal = _legal(self.cost, pos, mud)
            if self.regime == "values" or c == self.root:
                pattern = "ordinary"
                prior = _ordinary(bits, legal)
            else:
                prior = _degenerate(pattern, bits, legal)
                pattern = 0 if len(legal) == 1 else pattern  # one legal action: whatever was drawn, it is one-hot
            self.classes[pattern, value] += 1
            out += [prior, VALUES[self.regime][value]]
        return out[0], out[2], out[1], out[3]

    def _batch(self, leaves):
        r = [self.leaf(*l) for l in leaves]
        return (np.stack([x[0] for x in r]), np.stack([x[1] for x in r]), np.array([x[2] for x in r], F),
                np.array([x[3] for x in r], F))

    def oracle(self, leaves):
        hw = self.w * self.h
        return self._batch([(l["p1"], l["p2"], l["turn"], l["p1_mud"], l["p2_mud"], l["cheese"][:hw]) for l in leaves])

    def predict_fn(self, games):
        xy = lambda p: (int(p.x), int(p.y))  # noqa: E731
        return self._batch([(xy(g.player1_position), xy(g.player2_position), int(g.turn), int(g.player1_mud_turns),
                             int(g.player2_mud_turns), np.asarray(g.cheese_array(), np.uint8).reshape(-1)) for g in games])


def _cases():
    for name, og, mt in _positions():
        for batch in (4, 16):
            for noise in (0.0, 0.25):
                yield name, og, mt, batch, noise


_oracle_runs = {}


def oracle_runs(regime):
    """[(case, result, adversary)] of a regime, searched by the oracle once"""
    if regime not in _oracle_runs:
        runs = []
        for i, (name, og, mt, batch, noise) in enumerate(_cases()):
            adv = Adversary(regime, og)
            cfg = O.make_config(noise_epsilon=noise, **TUNED)
            want = O.search_once(og, cfg, SIMS, batch, seed=300 + i, backend=4, net=O.CallbackBackend(adv.oracle))
            runs.append(((name, og, mt, batch, noise, 300 + i), want, adv))
        _oracle_runs[regime] = runs
    return _oracle_runs[regime]


@pytest.mark.parametrize("regime", VALUES)
def test_evaluator_is_within_what_a_network_emits_and_meets_every_class(regime):
    runs = oracle_runs(regime)
    classes = sum((adv.classes for _, _, adv in runs), Counter())
    patterns = range(6) if regime == "priors" else ["ordinary"]
    for p in patterns:
        for v in range(6):
            assert classes[p, v] >= 10, (regime, PATTERNS[p] if p != "ordinary" else p, float(VALUES[regime][v]), classes[p, v])
    assert sum(classes["ordinary", v] for v in range(6)) > 0  # the roots
    # the function itself: legal priors in [0, 1] summing to 1 within 1e-6, values in [0, 1e4], a pure function
    adv = runs[-1][2]
    rng = np.random.default_rng(5)
    for _ in range(300):
        leaf = (tuple(rng.integers(0, 7, 2)), tuple(rng.integers(0, 7, 2)), int(rng.integers(0, 50)), int(rng.integers(0, 3)),
                int(rng.integers(0, 3)), rng.integers(0, 2, 49).astype(np.uint8))
        p1, p2, v1, v2 = adv.leaf(*leaf)
        again = adv.leaf(*leaf)
        for p, (pos, mud) in ((p1, (leaf[0], leaf[3])), (p2, (leaf[1], leaf[4]))):
            assert p.dtype == F and (p >= 0).all() and (p <= 1).all() and abs(float(p.astype(np.float64).sum()) - 1) <= 1e-6
            assert not p[[a for a in range(5) if a not in _legal(adv.cost, pos, mud)]].any()
        assert 0 <= v1 <= 1e4 and 0 <= v2 <= 1e4 and np.isfinite([v1, v2]).all()
        assert all(np.array_equal(a, b) for a, b in zip((p1, p2, v1, v2), again))


def test_noise_on_roots_keep_more_than_one_action():
    """Counted over the noise-on searches of both regimes: in ``values`` a subtree that holds a 1e4 leaf outweighs every
    other, however rare that leaf is made (tried at 1 leaf in 32), so after pruning those roots keep one action; the
    ``priors`` regime is where the root's policy, its pruning and the noise have more than one action to work on."""
    noisy = {r: [w for (_, _, _, _, noise, _), w, _ in oracle_runs(r) if noise > 0] for r in VALUES}
    spread = {r: [min((w["visit_counts_p1"] > 0).sum(), (w["visit_counts_p2"] > 0).sum()) >= 2 for w in ws]
              for r, ws in noisy.items()}
    print({r: f"{sum(v)} of {len(v)}" for r, v in spread.items()})
    assert 2 * sum(sum(v) for v in spread.values()) >= sum(len(v) for v in spread.values())
    assert all(spread["priors"])


@pytest.mark.gpu
@pytest.mark.parametrize("regime", VALUES)
def test_search_with_adversarial_evaluator_bit_exact(regime):
    """k_gather and k_backup, the one-lane-per-game kernels: with a predict_fn ar_search launches them whatever AR_GATHER
    and AR_BACKUP say (see the module's docstring)"""
    from alpharat_amd.mcts import rust_mcts_search
    from test_gpu_parity import _assert_result, _pyrat

    for (name, og, mt, batch, noise, seed), want, _ in oracle_runs(regime):
        adv = Adversary(regime, og)
        got = rust_mcts_search(_pyrat(og, mt), predict_fn=adv.predict_fn, simulations=SIMS, batch_size=batch, seed=seed,
                               noise_epsilon=noise, **TUNED)
        _assert_result(got, want, (regime, name, batch, noise))
