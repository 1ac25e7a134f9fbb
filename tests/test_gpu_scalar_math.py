"""The device's scalar arithmetic against the oracle's, call by call: collision budgets (powf), the random draws of
dev_rng.h (f64 exp / log / sqrt inside accept/reject tests) and dirichlet_mix. tests/hostsim runs the same headers with the
host's math library, the one the oracle uses, so only the real device can differ here. The library's test entries
ar_debug_budgets and ar_debug_draws run each routine with one thread per item (-m gpu); the conditions that keep these
cases sharp are checked on the oracle alone and need no GPU."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O

gpu = pytest.mark.gpu

ZIG_R = 3.654152885361008796  # AR_ZIG_R (dev_rng.h), AR_ZIG_NORM_R (oracle): where the normal sampler's tail begins

# (min, max, start, end, power): four settings at which one ulp of pow moves a budget (WIDE: the first two, by a lot), the
# three of test_gpu_collisions.py, and the default with its power of 1
BUDGETS = [
    (1, 65536, 0, 50000, 0.5),
    (1, 65536, 0, 50000, 3.0),
    (1, 256, 800, 50000, 0.5),
    (1, 4096, 100, 20000, 1.7),
    (1, 512, 20, 1500, 0.5),
    (1, 512, 20, 1500, 2.0),
    (0, 256, 20, 1500, 2.0),
    (1, 256, 800, 50000, 1.0),
]
WIDE = BUDGETS[:2]


def _budget_cfg(lo, hi, start, end, power):
    return O.make_config(collision_limit_min=lo, collision_limit_max=hi, collision_scaling_start=start,
                         collision_scaling_end=end, collision_scaling_power=power)


def _budgets_np(lo, hi, start, end, power, nudge=0):
    """calculate_collisions_left (search.rs:437-450) for every node count start..end in f32 NumPy; `nudge` = -1 / +1 moves
    the result of pow one ulp down / up before it is used."""
    f = np.float32
    n = np.arange(start, end + 1, dtype=np.int64)
    ratio = (n - start).astype(f) / f(end - start)
    pw = np.power(ratio.astype(np.float64), np.float64(f(power))).astype(f)
    if nudge:
        pw = np.nextafter(pw, f(np.inf if nudge > 0 else -np.inf))
    scaled = f(lo) + (f(hi) - f(lo)) * pw
    v = np.floor(scaled.astype(np.float64) + 0.5)  # f32::round on a value >= 0
    v = np.clip(v, lo, hi).astype(np.uint32)
    v[n <= start] = lo
    v[n >= end] = hi
    return n.astype(np.uint32), v


@pytest.mark.parametrize("case", BUDGETS, ids=str)
def test_numpy_restatement_of_the_budget_is_the_oracles(case):
    n, v = _budgets_np(*case)
    np.testing.assert_array_equal(v, O.collisions_left(_budget_cfg(*case), n))


@pytest.mark.parametrize("case", WIDE, ids=str)
def test_wide_budget_settings_react_to_one_ulp_of_pow(case):
    """Measured when the cases were chosen: 212 / 169 node counts (power 0.5) and 77 / 63 (power 3.0) change their budget
    when pow comes out one ulp low / high. At least 50 each, or the sweep below could no longer see such a pow."""
    n, _ = _budgets_np(*case)
    want = O.collisions_left(_budget_cfg(*case), n)
    for nudge in (-1, 1):
        changed = int((_budgets_np(*case, nudge=nudge)[1] != want).sum())
        print(case, "pow one ulp", "low" if nudge < 0 else "high", "->", changed, "budgets change")
        assert changed >= 50, (case, nudge, changed)


def _lib():
    from alpharat_amd import _lib

    L = _lib.load()
    L.ar_debug_budgets.restype = C.c_int
    L.ar_debug_budgets.argtypes = [C.POINTER(_lib.ArSearchConfig), C.c_void_p, C.c_uint32, C.c_void_p]
    L.ar_debug_draws.restype = C.c_int
    L.ar_debug_draws.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(O.OrDraw), C.c_void_p, C.c_void_p]
    return _lib, L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _device_budgets(case, n):
    _lib_mod, L = _lib()
    lo, hi, start, end, power = case
    cfg = _lib_mod.ArSearchConfig(1.5, 0.2, 2.0, 0.0, 10.83, lo, hi, start, end, power)
    out = np.zeros(len(n), dtype=np.uint32)
    _lib_mod.check(L.ar_debug_budgets(C.byref(cfg), _p(n), len(n), _p(out)))
    return out


@gpu
@pytest.mark.parametrize("case", BUDGETS, ids=str)
def test_device_budgets_equal_the_oracles_at_every_node_count(case):
    lo, hi, start, end, power = case
    n = np.arange(start, end + 1, dtype=np.uint32)
    want = O.collisions_left(_budget_cfg(*case), n)
    got = _device_budgets(case, n)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{bad.size} node counts with another budget than the oracle's; (node count, oracle, device): "
                           f"{[(int(n[i]), int(want[i]), int(got[i])) for i in bad[:10]]}")
    assert want[0] == lo and want[-1] == hi and len(np.unique(want)) > 100


@gpu
def test_budget_table_limit():
    """A power other than 1 is served from a table over start + 1 .. end - 1: end - start may be 2^22 at the most, and the
    last entry of the largest table is the right one. A power of 1 needs no table and keeps any range."""
    top = 1 << 22
    n = np.array([0, 1, 2, top // 4, top - 1, top, top + 1], dtype=np.uint32)
    for case in ((1, 65536, 0, top, 0.5), (1, 65536, 0, 4000000000, 1.0)):
        np.testing.assert_array_equal(_device_budgets(case, n), O.collisions_left(_budget_cfg(*case), n))
    with pytest.raises(ValueError, match="collision_scaling_end - collision_scaling_start <= 4194304"):
        _device_budgets((1, 65536, 0, top + 1, 0.5), n)


def _device_fill(seeds, d):
    """ar_debug_draws: the same streams and draws as O.rng_fill, on the device"""
    _lib_mod, L = _lib()
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    out, states = O.draw_buffers(len(seeds), d)
    _lib_mod.check(L.ar_debug_draws(_p(seeds), len(seeds), C.byref(d), _p(out), _p(states)))
    return out, states


def _where_first(differs):
    """'stream s, draw i' of the first difference in the first stream that has one"""
    s = int(np.flatnonzero(differs.reshape(differs.shape[0], -1).any(axis=1))[0])
    per_draw = differs[s].reshape(differs.shape[1], -1).any(axis=1)
    return s, int(np.flatnonzero(per_draw)[0])


def _assert_same_draws(seeds, d, what, skip=None):
    """Every draw's bits and every stream's final state equal the oracle's; `skip`: draws compared by the caller instead.
    Returns (device draws, oracle draws)."""
    want, want_states, _ = O.rng_fill(seeds, d)
    got, got_states = _device_fill(seeds, d)
    bits = {4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    differs = got.view(bits) != want.view(bits)
    if skip is not None:
        differs &= ~skip
    if differs.any():
        s, i = _where_first(differs)
        raise AssertionError(f"{what}: {int(differs.sum())} values differ, first in the stream of seed {int(seeds[s])} at "
                             f"draw {i}: device {got[s, i]!r} ({got.view(bits)[s, i]}), oracle {want[s, i]!r} "
                             f"({want.view(bits)[s, i]})")
    bad = np.flatnonzero((got_states != want_states).any(axis=1))
    assert bad.size == 0, f"{what}: the generator ends in another state for seeds {[int(seeds[s]) for s in bad[:8]]}"
    return got, want


INT_SEEDS = np.arange(256, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(3)  # 256 streams of 4096: 2^20
INT_SEEDS[0] = 0
INT_SEEDS[1] = 0xFFFFFFFFFFFFFFFF


@gpu
def test_u64_draws_and_seeding():
    got, _ = _assert_same_draws(INT_SEEDS, O.make_draw(O.DRAW_U64, 4096), "rng_u64")
    assert len(np.unique(got)) > (1 << 20) - 8


@gpu
@pytest.mark.parametrize("n", [1, 2, 3, 5, 25, (1 << 31) + 1])
def test_range_draws(n):
    got, _ = _assert_same_draws(INT_SEEDS, O.make_draw(O.DRAW_BELOW, 4096, n=n), f"rng_below({n})")
    assert got.max() < n and len(np.unique(got)) >= min(n, 1000)


@gpu
@pytest.mark.parametrize("w,values", [
    ((1, 1, 1, 1, 1), {0, 1, 2, 3, 4}),
    ((0.2, 0.2, 0.2, 0.2, 0.2), {0, 1, 2, 3, 4}),
    ((0, 0, 1, 0, 0), {2}),
    ((0, 0.7, 0, 0.3, 0), {1, 3}),
    ((0.5, 0, 0, 0, 1e-4), {0, 4}),
    ((0.01, 0.02, 0.9, 0.03, 0.04), {0, 1, 2, 3, 4}),
    ((0, 0, 0, 0, 0), {-1}),
    ((0.3, -0.1, 0.3, 0.3, 0.2), {-1}),
], ids=["ones", "flat", "one-hot", "two-zeros", "tiny-last", "peaked", "all-zero", "negative"])
def test_weighted_draws(w, values):
    got, _ = _assert_same_draws(INT_SEEDS, O.make_draw(O.DRAW_WEIGHTED5, 4096, w=w), f"rng_weighted5({w})")
    assert set(np.unique(got).tolist()) == values


NORMAL_SEEDS = np.arange(64, dtype=np.uint64) + np.uint64(0xA1FA0000)  # the seeds self-play gives its first 64 games
NORMAL_DRAWS = 1 << 16                                                 # per stream: 2^22 in all


@pytest.fixture(scope="module")
def normal_want():
    return O.rng_fill(NORMAL_SEEDS, O.make_draw(O.DRAW_NORMAL, NORMAL_DRAWS))


def test_normal_seeds_reach_the_tail_and_the_wedge_test(normal_want):
    """The tail (log of two uniforms, probability 2.7e-4 a draw: about 1100 of 2^22) and the wedge test (exp) are where the
    device's libm decides or shapes a draw."""
    want, _, (tail, wedge) = normal_want
    print("normal draws:", want.size, "tail entries:", tail, "wedge tests:", wedge)
    assert want.size == 1 << 22
    assert tail >= 500 and wedge >= 10000
    assert int((np.abs(want) > ZIG_R).sum()) == tail


@gpu
def test_normal_draws(normal_want):
    """Every accept/reject decision agrees (the final states) and every value outside the tail is the oracle's f64. A tail
    value is log(e1) / R moved by R: glibc and OCML both document at most 1 ulp for f64 log, the division and the
    subtraction round once each, so those are held to a relative difference of 2^-50."""
    want, want_states, _ = normal_want
    d = O.make_draw(O.DRAW_NORMAL, NORMAL_DRAWS)
    tail = np.abs(want) > ZIG_R
    got, _ = _assert_same_draws(NORMAL_SEEDS, d, "rng_normal", skip=tail)
    rel = np.abs(got[tail] - want[tail]) / np.abs(want[tail])
    print(f"rng_normal: {int(tail.sum())} tail draws, {int((rel > 0).sum())} differ from the oracle's, largest relative "
          f"difference {rel.max():.3e} (2^-50 = {2.0 ** -50:.3e})")
    assert rel.max() <= 2.0 ** -50, (int((rel > 2.0 ** -50).sum()), float(rel.max()))


GAMMA_SHAPES = [1.00002, float(np.float32(10.83) / np.float32(5)), 10.83, 80.0]


@gpu
@pytest.mark.parametrize("shape", GAMMA_SHAPES, ids=lambda s: f"{s:.6g}")
def test_gamma_draws(shape):
    """sqrt sets c, log sits on both sides of the acceptance test; the value d * v passes through no libm call."""
    got, _ = _assert_same_draws(NORMAL_SEEDS, O.make_draw(O.DRAW_GAMMA, 1 << 14, shape=shape), f"rng_gamma({shape})")
    assert got.min() > 0 and abs(got.mean() - shape) < 0.01 * shape


def _priors(n):
    """uniform, peaked and one with a zero entry, over n outcomes (entries from n on are 0 and stay 0)"""
    if n == 1:
        return [(1.0, 0, 0, 0, 0)]
    uniform = [np.float32(1) / np.float32(n)] * n
    peaked = [0.94] + [0.06 / (n - 1)] * (n - 1)
    with_zero = [0.0] + [1.0 / (n - 1)] * (n - 1)
    return [tuple(p + [0.0] * (5 - n)) for p in (uniform, peaked, with_zero)]


@gpu
@pytest.mark.parametrize("epsilon,concentration", [(0.25, 10.83), (1.0, 5.001), (0.6, 400.0)])
def test_dirichlet_mix(epsilon, concentration):
    """2^16 mixes for every outcome count and prior: these f32 go into a record, so they are the oracle's bits."""
    seeds = NORMAL_SEEDS + np.uint64(1000)
    for n in range(1, 6):
        for prior in _priors(n):
            d = O.make_draw(O.DRAW_DIRICHLET, 1 << 10, n=n, w=prior, epsilon=epsilon, concentration=concentration)
            got, _ = _assert_same_draws(seeds, d, f"dirichlet_mix(n={n}, prior={prior})")
            assert np.all(got[:, :, n:] == 0)
            if n == 1:
                assert np.all(got[:, :, 0] == 1)
            else:
                np.testing.assert_allclose(got.sum(axis=2), 1.0, atol=1e-5)
                assert len(np.unique(got[:, :, 0])) > 1000
