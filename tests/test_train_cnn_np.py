"""CPU: the float64 restatements of PyRatCNN's training step (tests/_train_cnn_np.py, tests/_cnn_train_torch.py) against the
reference's own step (tests/golden/train_cnn), the ReLU guards of every fixture the device test runs, the exchange of P1 and
P2 under all-swapped rows, and dev_train_cnn.h through its CPU harness (tests/hostsim_train_cnn): the neighbour function
against literals, the split of a row, the player cells and the two partitions against a table of literals."""
import numpy as np
import pytest

import _train_cnn as TC
import _train_cnn_np as NC

REL = 1e-12


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max()
    assert err <= REL * max(1.0, np.abs(want).max()), (what, err)


def _check(res, want, what, n_blocks):
    for k in NC.LOSS_KEYS:
        _close(res["losses"][k], want["losses"][k], f"{what} {k}")
    for k in NC.OUT_KEYS:
        _close(res[k], want[k], f"{what} {k}")
    for k in NC.param_keys(n_blocks):
        _close(res["grads"][k], want["grads"][k], f"{what} grad {k}")
    for k in NC.running_keys(n_blocks):
        _close(res["running"][k], want["running"][k], f"{what} {k}")


# ---- the restatements against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TC.GOLDEN)
def test_numpy_step_reproduces_the_reference_in_float64(name):
    case = TC.golden_case(name)
    B = NC.n_blocks_of(case["sd"])
    assert case["f64"]["grads"]["stem.weight"].dtype == np.float64 and case["f32"]["grads"]["stem.weight"].dtype == np.float32
    assert set(case["f64"]["grads"]) == set(NC.param_keys(B)) and len(NC.param_keys(B)) == 11 + 6 * B
    assert len(NC.running_keys(B)) == 2 + 4 * B
    res = NC.step(case)
    assert len(res["pre"]) == 1 + 2 * B + 4
    _check(res, case["f64"], name, B)


@pytest.mark.parametrize("name", TC.GOLDEN)
def test_torch_restatement_reproduces_the_reference_in_float64(name):
    import torch

    import _cnn_train_torch as CT

    case = TC.golden_case(name)
    _check(CT.step(case, torch.float64), case["f64"], name, NC.n_blocks_of(case["sd"]))


@pytest.mark.parametrize("name", TC.GOLDEN)
def test_golden_rows_are_the_boards_rows(name):
    """the device test uploads the board's games and sets the golden's order: the rows must be those"""
    case = TC.golden_case(name)
    again = TC.make_case(case["board"], case["sd"], case["order"], case["swap"])
    for k in ("observation", "policy_p1", "policy_p2", "value_p1", "value_p2"):
        assert np.asarray(again[k]).reshape(-1).tobytes() == np.asarray(case[k]).reshape(-1).tobytes(), k


def test_goldens_are_the_agreed_ones():
    assert len(TC.GOLDEN) == 3 and any(c[1] == "7x5" for c in TC.GOLDEN_CASES)  # one board is not square
    for name, board, Ch, B, n in TC.GOLDEN_CASES:
        case = TC.golden_case(name)
        assert TC.dims_of(case) == (Ch, 32, 64, B) and len(case["order"]) == n and case["board"] == board


# ---- the ReLU guards: conditions on the fixtures, not tolerances ----------------------------------------------------------------
@pytest.mark.parametrize("name", TC.GOLDEN)
def test_relu_guard_goldens(name):
    """the generator's two numbers, and the second one again from the restatement: no pre-ReLU value of the float64 run is
    nearer to zero than eight times the largest difference between the float32 and the float64 run"""
    case = TC.golden_case(name)
    pre = NC.step(case)["pre"]
    # Small enough for a seed to exist: "at most about 50 000" pre-ReLU values. The limit here is 56 000 because the largest of
    # the agreed cases, 7x5 / C = 64 / B = 1 / n = 8, has 3 * 280 * 64 + 2 * 8 * (32 + 64) = 55 296 of them.
    assert sum(a.size for a in pre) <= 56_000
    print(f"{name}: pre_min {case['pre_min']:.3e} pre_err {case['pre_err']:.3e}")
    assert case["pre_min"] >= TC.GUARD_FACTOR * case["pre_err"] > 0
    assert abs(NC.relu_margin(case) - case["pre_min"]) <= 1e-9


@pytest.mark.parametrize("shape", TC.SHAPES, ids=TC.SHAPE_IDS)
def test_relu_guard_shapes(shape):
    margin = NC.relu_margin(TC.shape_case(*shape))
    print(f"min|pre64| {margin:.3f}")
    assert margin >= TC.DECIDED_MARGIN


def test_relu_guard_windows_swaps_and_player_cells():
    whole, windows = TC.window_cases()
    for case in windows + list(TC.swap_cases()) + [TC.player_cell_case()]:
        assert NC.relu_margin(case) >= TC.DECIDED_MARGIN


def test_shapes_are_the_agreed_ones():
    got = [(b, Ch, B, n) for b, Ch, B, n, _, _, _ in TC.SHAPES]
    assert got == [("5x5 open", 32, 0, 3), ("5x5 open", 32, 1, 2), ("7x5", 64, 2, 33), ("7x7", 96, 1, 5), ("5x5 open", 256, 1, 3),
                   ("16x16", 32, 1, 2), ("5x5 open", 32, 8, 2), ("5x5 open", 32, 1, 4), ("5x5 open", 32, 1, None)]
    assert TC.SHAPES[7][4:6] == (24, 32)
    n = TC.caps_rows(25)
    P, rpp = TC.sim_cols(n, 25, 32)
    S, kps = TC.sim_rows_split(n, 25)
    max_parts, part_rows, max_splits, split_rows = TC.sim_caps()
    rows = n * 25
    assert -(-rows // part_rows) > max_parts and -(-rows // split_rows) > max_splits  # more parts and ranges asked than the caps
    assert P <= max_parts and rpp > part_rows and S <= max_splits and kps > split_rows  # ... so both hold them longer
    assert (n - 1) * 25 <= max(max_parts * part_rows, max_splits * split_rows)  # and the smallest such n


# ---- swapped rows --------------------------------------------------------------------------------------------------------------
def test_all_swapped_rows_exchange_the_players_and_keep_the_gradients():
    plain, swapped = (NC.step(c) for c in TC.swap_cases())
    for a, b in (("logits_p1", "logits_p2"), ("value_p1", "value_p2")):
        _close(swapped[a], plain[b], a)
        _close(swapped[b], plain[a], b)
    for a, b in (("loss_p1", "loss_p2"), ("loss_value_p1", "loss_value_p2")):
        _close(swapped["losses"][a], plain["losses"][b], a)
    _close(swapped["losses"]["loss"], plain["losses"]["loss"], "loss")
    assert np.abs(plain["logits_p1"] - plain["logits_p2"]).max() > 1e-3
    for k in plain["grads"]:
        _close(swapped["grads"][k], plain["grads"][k], f"grad {k}")
    for k in plain["running"]:
        _close(swapped["running"][k], plain["running"][k], k)


# ---- dev_train_cnn.h on the CPU ------------------------------------------------------------------------------------------------
# tap t = 3 ky + kx reads (y + ky - 1, x + kx - 1); cells of a 3x2 board (3 wide, 2 high): 0 1 2 / 3 4 5
NBR_3x2 = [[-1, -1, -1, -1, 0, 1, -1, 3, 4], [-1, -1, -1, 0, 1, 2, 3, 4, 5], [-1, -1, -1, 1, 2, -1, 4, 5, -1],
           [-1, 0, 1, -1, 3, 4, -1, -1, -1], [0, 1, 2, 3, 4, 5, -1, -1, -1], [1, 2, -1, 4, 5, -1, -1, -1, -1]]
# a 2x3 board (2 wide, 3 high): 0 1 / 2 3 / 4 5
NBR_2x3 = [[-1, -1, -1, -1, 0, 1, -1, 2, 3], [-1, -1, -1, 0, 1, -1, 2, 3, -1], [-1, 0, 1, -1, 2, 3, -1, 4, 5],
           [0, 1, -1, 2, 3, -1, 4, 5, -1], [-1, 2, 3, -1, 4, 5, -1, -1, -1], [2, 3, -1, 4, 5, -1, -1, -1, -1]]


@pytest.mark.parametrize("bw,bh,table", [(3, 2, NBR_3x2), (2, 3, NBR_2x3)], ids=["3x2", "2x3"])
def test_neighbour_function_against_literals(bw, bh, table):
    for cell in range(bw * bh):
        assert [TC.sim_nbr(cell, tap, bw, bh) for tap in range(9)] == table[cell], cell
    for cell in range(bw * bh):  # a mirrored tap is the inverse: it leads back where the tap came from
        for tap in range(9):
            nb = TC.sim_nbr(cell, tap, bw, bh)
            if nb >= 0:
                assert TC.sim_nbr(nb, TC.sim_mirror(tap), bw, bh) == cell, (cell, tap)
    assert [TC.sim_mirror(t) for t in range(9)] == [8, 7, 6, 5, 4, 3, 2, 1, 0]


def test_split_of_a_row_and_player_cells():
    case = TC.player_cell_case()
    w, h = case["width"], case["height"]
    x = np.asarray(case["observation"], np.float32)
    n, hw = len(x), w * h
    x5, side, cells = TC.sim_split(x, w, h)
    spatial, sides, masks = NC.parse_obs(x.astype(np.float64), w, h)
    assert np.array_equal(x5.reshape(n, h, w, 5), spatial.astype(np.float32))
    assert np.array_equal(side, np.concatenate(sides).astype(np.float32))
    assert np.array_equal(cells, np.concatenate([m.argmax(axis=1) for m in masks]))
    assert all((m.sum(axis=1) == 1).all() for m in masks)
    # what the case is for: both players on one cell, and every corner, among the first five rows, swapped or not
    assert any(cells[r] == cells[n + r] for r in range(5))
    assert {0, w - 1, hw - w, hw - 1} <= set(cells[:5]) | set(cells[n:n + 5])
    # literals: a row whose planes are its column numbers
    row = np.arange(7 * 6 + 6, dtype=np.float32)[None]
    x5, side, cells = TC.sim_split(row, 3, 2)
    assert x5.tolist() == [[0, 1, 2, 3, 36], [4, 5, 6, 7, 37], [8, 9, 10, 11, 38], [12, 13, 14, 15, 39], [16, 17, 18, 19, 40],
                           [20, 21, 22, 23, 41]]
    assert side.tolist() == [[46, 44, 43], [47, 45, 43]]
    assert cells.tolist() == [0, 0]  # the first non-zero of columns [24, 30) and [30, 36)
    empty = np.zeros((1, 48), np.float32)
    assert TC.sim_split(empty, 3, 2)[2].tolist() == [-1, -1]


# (n, hw, C) -> (P, rpp), (S, kps); the last three rows at and over a cap
PARTITIONS = [((2, 25, 32), (1, 50), (1, 64)),
              ((3, 25, 256), (2, 38), (1, 80)),
              ((33, 35, 64), (19, 61), (3, 400)),
              ((5, 49, 96), (4, 62), (1, 256)),
              ((2, 256, 32), (8, 64), (1, 512)),
              ((4096, 49, 64), (256, 784), (64, 3136)),
              ((656, 25, 32), (253, 65), (33, 512)),       # the first n of 5x5 over the parts' cap: 257 parts of 64 rows asked
              ((1310, 25, 32), (256, 128), (64, 512)),     # 32750 rows: the splits' cap reached, not passed
              ((1311, 25, 32), (255, 129), (63, 528)),     # over both: 65 ranges of 512 rows asked
              ((65536, 64, 32), (256, 16384), (64, 65536))]


@pytest.mark.parametrize("shape,cols,split", PARTITIONS, ids=[f"n{s[0][0]}-hw{s[0][1]}-c{s[0][2]}" for s in PARTITIONS])
def test_partitions_against_literals(shape, cols, split):
    n, hw, Ch = shape
    assert TC.sim_cols(n, hw, Ch) == cols
    assert TC.sim_rows_split(n, hw) == split
    P, rpp = cols
    S, kps = split
    assert (P - 1) * rpp < n * hw <= P * rpp and (S - 1) * kps < n * hw <= S * kps and kps % 16 == 0


def test_partition_caps():
    assert TC.sim_caps() == (256, 64, 64, 512)
    for n, hw in ((2, 4), (17, 49), (65536, 64), (16384, 256)):
        assert TC.sim_cols(n, hw, 32)[0] <= 256 and TC.sim_rows_split(n, hw)[0] <= 64
