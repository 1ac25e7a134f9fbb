"""CPU: the dropout mask of the training steps. alpharat_amd/csrc/dev_dropout.h compiled for the host
(tests/hostsim_dropout), its NumPy restatement (tests/_dropout_np.py) and literals worked out from the definition in plain
integers are held against one another, so the three cannot drift together; then what a mask must be whatever its bits are:
all ones at p = 0, another mask for another step or call, and the dropped count and the agreement of two masks where
independent draws at rate p put them."""
import itertools

import numpy as np
import pytest

import _dropout_np as D
import _train_dropout as TD

SHAPES = [(2, 32), (33, 32), (129, 64), (300, 256)]
SEEDS = [0, 1, 2 ** 63 + 5]
STEPS = [0, 1, 2 ** 32 + 1]
CALLS = list(range(7))
RATES = [0.0, 0.1, 0.5, 0.9, 1.0 - 2.0 ** -24]

# (seed, step, call, p): the key, the 64 bits of element 0 and keep() of elements 0 .. 63 (bit e of the word: element e),
# from the definition in include/alpharat_hip.h with Python integers
LITERALS = [((0, 0, 0, 0.5), 0x238275BC38FCBE91, 0x2130748AAAC80268, 0x5D7E68852A71BCAC),
            ((1, 1, 1, 0.1), 0x7D8E67D8F2AF75D5, 0x7D1B8A2FD9432750, 0xFFF37FBF9EFFFFDF),
            ((2 ** 63 + 5, 2 ** 32 + 1, 6, 0.9), 0x6FE96CF593F60AF2, 0x2CDCF76A56F573F4, 0x8000180014804200)]
# p -> (thr, scale)
PINNED = {0.0: (0, 1.0), 0.1: (429496736, 1.1111111640930176), 0.5: (2147483648, 2.0), 0.9: (3865470464, 9.999998092651367),
          1.0 - 2.0 ** -24: (4294967040, 16777216.0)}


def _word(mask_row) -> int:
    return sum(1 << e for e in range(64) if mask_row[e])


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{H}" for n, H in SHAPES])
def test_hostsim_equals_numpy_bit_for_bit(shape):
    n, H = shape
    for seed, step, call in itertools.product(SEEDS, STEPS, CALLS):
        assert TD.sim().ds_key(seed, step, call) == int(D.key(seed, step, call)), (seed, step, call)
        want_bits = D.bits(seed, step, call, n, H)
        for i, p in enumerate(RATES):
            got, bits = TD.sim_mask(seed, step, call, n, H, p, with_bits=True)
            assert got.tobytes() == D.mask(seed, step, call, n, H, p).tobytes(), (seed, step, call, p)
            if i == 0:
                assert bits.tobytes() == want_bits.tobytes(), (seed, step, call)


def test_p_zero_keeps_every_element():
    for seed, step, call in itertools.product(SEEDS, STEPS, (0, 6)):
        assert TD.sim_mask(seed, step, call, 300, 256, 0.0).all()
        assert D.mask(seed, step, call, 300, 256, 0.0).all()


def test_thr_and_scale_are_pinned():
    for p, (thr, scale) in PINNED.items():
        assert TD.sim().ds_thr(p) == thr == D.thr(p), p
        assert float(TD.sim().ds_scale(p)) == scale == float(D.scale(p)), p
    assert set(PINNED) == set(RATES)


def test_literals_from_the_definition():
    for (seed, step, call, p), key, bits0, word in LITERALS:
        assert int(D.key(seed, step, call)) == key == TD.sim().ds_key(seed, step, call)
        got, bits = TD.sim_mask(seed, step, call, 2, 32, p, with_bits=True)  # elements 0 .. 63 are rows 0 and 1 at H = 32
        assert int(bits[0, 0]) == bits0 == int(D.bits(seed, step, call, 2, 32)[0, 0])
        assert _word(got.reshape(-1)) == word == _word(D.mask(seed, step, call, 2, 32, p).reshape(-1))
        # the element index is row * H + column: the same 64 elements as the first row of a wider call
        assert _word(D.mask(seed, step, call, 1, 64, p).reshape(-1)) == word
    assert TD.sim().ds_mix(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF  # SplitMix64's first output from state 0


def test_step_and_call_change_the_mask():
    base = D.mask(1, 0, 0, 33, 32, 0.5)
    assert not np.array_equal(base, D.mask(1, 1, 0, 33, 32, 0.5))
    assert not np.array_equal(base, D.mask(1, 0, 1, 33, 32, 0.5))
    assert not np.array_equal(base, D.mask(2, 0, 0, 33, 32, 0.5))
    assert not np.array_equal(TD.sim_mask(1, 0, 0, 33, 32, 0.5), TD.sim_mask(1, 1, 0, 33, 32, 0.5))
    assert not np.array_equal(TD.sim_mask(1, 0, 0, 33, 32, 0.5), TD.sim_mask(1, 0, 1, 33, 32, 0.5))


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_dropped_count_and_pair_agreement(p):
    """independent draws at rate p: the dropped count of a mask is Binomial(N, p), the agreeing elements of two masks
    Binomial(N, (1 - p)^2 + p^2); both within 5 standard deviations, over four seeds, steps 0 .. 2 and calls 0, 1, 6"""
    n, H = 4096, 256
    N = n * H
    masks = {}
    for seed, step, call in itertools.product([0, 1, 12345, 2 ** 63 + 5], range(3), (0, 1, 6)):
        m = D.mask(seed, step, call, n, H, p).reshape(-1)
        dropped = int(N - m.sum())
        z = (dropped - N * p) / np.sqrt(N * p * (1 - p))
        assert abs(z) <= 5.0, (seed, step, call, dropped, z)
        masks[(seed, step, call)] = np.packbits(m)
    q = (1 - p) ** 2 + p ** 2
    sd = np.sqrt(N * q * (1 - q))
    worst = 0.0
    for (ka, a), (kb, b) in itertools.combinations(masks.items(), 2):
        agree = N - int(np.unpackbits(a ^ b).sum())
        z = (agree - N * q) / sd
        worst = max(worst, abs(z))
        assert abs(z) <= 5.0, (ka, kb, agree, z)
    print(f"p={p}: {len(masks)} masks, worst pair agreement {worst:.2f} standard deviations")
