"""CPU: the float64 restatements of PyRatCNN's training step with GPoolResBlocks and dropout (tests/_train_gpool_np.py,
tests/_gpool_train_torch.py) against the reference's own step (tests/golden/train_gpool), the two guards -- the ReLU's and
the maximum's -- of every fixture the device test runs, amax's tie rule, the dropout's call numbering, and
dev_train_gpool.h through its CPU harness (tests/hostsim_train_gpool) against literals."""
import numpy as np
import pytest

import _dropout_np as D
import _train_cnn as TC
import _train_cnn_np as NC
import _train_gpool as TG
import _train_gpool_np as NG

REL = 1e-12


def _close(got, want, what, rel=REL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max()
    assert err <= rel * max(1.0, np.abs(want).max()), (what, err)


def _check(res, want, what, blocks, rel=REL):
    for k in NC.LOSS_KEYS:
        _close(res["losses"][k], want["losses"][k], f"{what} {k}", rel)
    for k in NC.OUT_KEYS:
        _close(res[k], want[k], f"{what} {k}", rel)
    for k in NG.param_keys(blocks):
        _close(res["grads"][k], want["grads"][k], f"{what} grad {k}", rel)
    for k in NG.running_keys(blocks):
        _close(res["running"][k], want["running"][k], f"{what} {k}", rel)


# ---- the restatements against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TG.GOLDEN)
def test_numpy_step_reproduces_the_reference_in_float64(name):
    case = TG.golden_case(name)
    blocks = NG.blocks_of(case["sd"])
    P = sum(1 for g in blocks if g)
    assert case["f64"]["grads"]["stem.weight"].dtype == np.float64 and case["f32"]["grads"]["stem.weight"].dtype == np.float32
    assert set(case["f64"]["grads"]) == set(NG.param_keys(blocks)) and len(NG.param_keys(blocks)) == 11 + 6 * len(blocks) + 5 * P
    assert len(NG.running_keys(blocks)) == 2 + 4 * len(blocks) + 2 * P
    res = NG.step(case)
    assert len(res["pre"]) == 1 + 2 * len(blocks) + P + 4 and len(res["pz"]) == P
    _check(res, case["f64"], name, blocks)


@pytest.mark.parametrize("name", TG.GOLDEN)
def test_torch_restatement_reproduces_the_reference_in_float64(name):
    import torch

    import _gpool_train_torch as GT

    case = TG.golden_case(name)
    _check(GT.step(case, torch.float64), case["f64"], name, NG.blocks_of(case["sd"]))


@pytest.mark.parametrize("name", TG.GOLDEN)
def test_golden_rows_are_the_boards_rows(name):
    case = TG.golden_case(name)
    again = TG.make_case(case["board"], case["sd"], case["order"], case["swap"])
    for k in ("observation", "policy_p1", "policy_p2", "value_p1", "value_p2"):
        assert np.asarray(again[k]).reshape(-1).tobytes() == np.asarray(case[k]).reshape(-1).tobytes(), k


def test_goldens_are_the_agreed_ones():
    got = [(board, Ch, blocks, n, p) for _, board, Ch, blocks, n, p in TG.GOLDEN_CASES]
    assert got == [("5x5 open", 32, (32,), 2, 0.0), ("5x5 open", 32, (0, 16), 12, 0.1), ("7x5", 32, (32, 0), 8, 0.0)]
    for name, board, Ch, blocks, n, p in TG.GOLDEN_CASES:
        case = TG.golden_case(name)
        assert TG.dims_of(case) == (Ch, 32, 64, len(blocks)) and NG.blocks_of(case["sd"]) == blocks
        assert len(case["order"]) == n and case["board"] == board
        assert ("masks" in case) == (p != 0)
        if p:  # the masks are the library's, under the call numbering of the header
            assert case["p"] == float(np.float32(p)) and (case["dropout_seed"], case["dropout_step"]) == TG.GOLDEN_DROPOUT
            for call, m in enumerate(case["masks"]):
                assert np.array_equal(m, D.mask(*TG.GOLDEN_DROPOUT, call, n, 32 if call < 2 else 64, p)), call
    largest = max(f.stat().st_size for f in TC.GOLD.glob("*.npz"))
    assert all(f.stat().st_size <= largest for f in TG.GOLD.glob("*.npz")) and len(list(TG.GOLD.glob("*.npz"))) == 6


def test_a_resblock_network_without_masks_is_the_cnn_restatement_exactly():
    case = TC.shape_case(*TC.SHAPES[1])
    a, b = NC.step(case), NG.step(case)
    for k in a["grads"]:
        assert a["grads"][k].tobytes() == b["grads"][k].tobytes(), k
    assert a["losses"]["loss"] == b["losses"]["loss"]
    ones = dict(case, masks=[np.ones((2, 32), bool)] * 2 + [np.ones((2, 64), bool)] * 2, scale=1.0)
    c = NG.step(ones)
    for k in a["grads"]:
        assert a["grads"][k].tobytes() == c["grads"][k].tobytes(), k


# ---- the guards: conditions on the fixtures, not tolerances -----------------------------------------------------------------------
@pytest.mark.parametrize("name", TG.GOLDEN)
def test_guards_goldens(name):
    """the generator's four numbers, and the float64 ones again from the restatement: no ReLU and no maximum of the float64
    run is nearer to changing than eight times the largest difference between the float32 and the float64 run"""
    case = TG.golden_case(name)
    res = NG.step(case)
    print(f"{name}: pre_min {case['pre_min']:.3e} pre_err {case['pre_err']:.3e} max_gap {case['max_gap']:.3e} pz_err {case['pz_err']:.3e}")
    assert case["pre_min"] >= TG.GUARD_FACTOR * case["pre_err"] > 0
    assert case["max_gap"] >= TG.GUARD_FACTOR * case["pz_err"] > 0
    assert abs(NG.relu_margin(res) - case["pre_min"]) <= 1e-9
    assert abs(NG.max_gap(res["pz"]) - case["max_gap"]) <= 1e-9


@pytest.mark.parametrize("shape", TG.SHAPES, ids=TG.SHAPE_IDS)
def test_guards_shapes(shape):
    g = TG.guards(TG.shape_case(*shape))
    print({k: f"{v:.3e}" for k, v in g.items()})
    assert g["pre_min"] >= TG.DECIDED_MARGIN and TG.guards_hold(g)


def test_guards_windows_swaps_player_cells_dropout_and_trajectory():
    whole, windows = TC.window_cases()
    cases = [TG.with_trunk(c) for c in windows + list(TC.swap_cases()) + [TC.player_cell_case()]]
    shipped = TG.shape_case(*TG.SHAPES[5])
    cases += [NG.with_masks(shipped, TG.DROPOUT_SEED, s, TG.DROPOUT_P) for s in (0, 1)]
    cases.append(NG.with_masks(TG.shape_case(*TG.SHAPES[8]), TG.DROPOUT_SEED, 3, TG.DROPOUT_P))
    # the trajectory's batches under their steps' masks, at the weights it starts from (two steps at lr 1e-3 move them little)
    (Ch, PD, HD), (w, h) = TG.TRAJ_DIMS, TG.BOARDS[TG.TRAJ_BOARD][1:3]
    sd0 = NG.random_gpool_cnn(w, h, Ch, PD, HD, TG.TRAJ_BLOCKS, TG.TRAJ_SEED)
    epochs, steps = TG.trajectory_plan()
    plans = {e: (o, m) for e, o, m in epochs}
    for s, (e, first) in enumerate(steps):
        idx = plans[e][0][first:first + TG.TRAJ_BATCH]
        cases.append(NG.with_masks(TG.make_case(TG.TRAJ_BOARD, sd0, idx, plans[e][1][idx]), TG.DROPOUT_SEED, s, TG.DROPOUT_P))
    for case in cases:
        g = TG.guards(case)
        assert g["pre_min"] >= TG.DECIDED_MARGIN and TG.guards_hold(g), g


def test_tie_cases_tie_exactly_and_keep_the_relu_guard():
    every, some = TG.tie_cases()
    for case, tied in ((every, 16), (some, 5)):
        res = NG.step(case)
        g = TG.guards(case, res)
        assert g["pre_min"] >= TG.DECIDED_MARGIN and TG.guards_hold(g, with_max=False)
        pz = res["pz"][0]
        is_max = pz == pz.max(axis=1, keepdims=True)
        assert (is_max.sum(axis=1) == pz.shape[1]).all(axis=0).sum() == tied  # channels all of whose cells hold the maximum
        if tied == 5:
            assert NG.max_gap([pz[:, :, 5:]]) >= TG.GUARD_FACTOR * g["pz_err"]  # the other channels are decided


def test_shapes_are_the_agreed_ones():
    got = [(b, Ch, blocks, n) for b, Ch, blocks, n, _, _, _ in TG.SHAPES]
    assert got == [("5x5 open", 32, (0, 8), 3), ("5x5 open", 32, (0, 36), 3), ("5x5 open", 256, (256,), 2), ("5x5 open", 32, (16, 0), 4),
                   ("5x5 open", 32, (16, 32), 3), ("7x7", 64, (0, 0, 32), 4), ("2x1", 32, (8,), 5), ("16x16", 32, (0, 16), 2),
                   ("7x5", 32, (0, 16), 33)]
    P, rpp = TC.sim_cols(33, 35, 32)
    S, kps = TC.sim_rows_split(33, 35)
    assert P > 1 and S > 1 and (33 * 35) % 64 != 0  # several parts and several split ranges, none a multiple of 64


# ---- amax's rule -------------------------------------------------------------------------------------------------------------------
def test_amax_shares_its_gradient_among_ties():
    import torch

    x = torch.tensor([[1.0, 3.0], [3.0, 0.0]], dtype=torch.float64, requires_grad=True)
    x.amax(dim=(0, 1)).backward()
    assert x.grad.tolist() == [[0.0, 0.5], [0.5, 0.0]]


def test_tie_gradients_match_autograd_in_float64():
    import torch

    import _gpool_train_torch as GT

    for case in TG.tie_cases():
        blocks = NG.blocks_of(case["sd"])
        _check(NG.step(case), GT.step(case, torch.float64), "ties", blocks, rel=1e-10)


# ---- the dropout's call numbering -------------------------------------------------------------------------------------------------
def test_dropout_calls_are_encoder_p1_p2_then_combiner_p1_p2():
    assert NG.CNN_CALLS == ("player_encoder/p1", "player_encoder/p2", "combiner/p1", "combiner/p2")
    case = NG.with_masks(TG.shape_case(*TG.SHAPES[0]), 9, 4, 0.25)
    n = len(case["order"])
    assert [m.shape for m in case["masks"]] == [(n, 32), (n, 32), (n, 64), (n, 64)]
    for call, m in enumerate(case["masks"]):
        H = m.shape[1]
        e = np.arange(n * H, dtype=np.uint64)
        with np.errstate(over="ignore"):
            bits = D.mix(D.key(9, 4, call) + (e + np.uint64(1)) * D.G).reshape(n, H)
        assert np.array_equal(m, (bits >> np.uint64(32)) >= np.uint64(D.thr(0.25))), call
    assert case["scale"] == float(np.float32(1) / np.float32(0.75))
    # the masks matter, and each call's own: exchanging two of them changes the step
    a = NG.step(case)["losses"]["loss"]
    b = NG.step(dict(case, masks=[case["masks"][1], case["masks"][0]] + case["masks"][2:]))["losses"]["loss"]
    c = NG.step(dict(case, masks=None))["losses"]["loss"]
    assert a != b and a != c


# ---- dev_train_gpool.h on the CPU --------------------------------------------------------------------------------------------------
def test_mean_and_max_of_a_row_against_literals():
    assert TG.sim_reduce([1.0, 3.0, 2.0, -2.0]) == (1.0, 3.0, 1)
    assert TG.sim_reduce([-5.0]) == (-5.0, -5.0, 1)
    assert TG.sim_reduce([-1.0, -4.0]) == (-2.5, -1.0, 1)
    # a stride: the cells of channel 0 of a [3][2] array
    assert TG.sim_reduce([1.0, 9.0, 4.0, 9.0, 1.0, 9.0], stride=2) == (2.0, 4.0, 1)
    # the sum is formed in double and rounded once: 2^24 + 1 + 1 + 1 + 1 is 2^24 + 4, not 2^24 as a float32 sum would stay
    z = [16777216.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0]
    assert TG.sim_reduce(z)[0] == (16777216.0 + 4.0) / 8.0


def test_tie_counts_against_literals():
    assert TG.sim_reduce([1.0, 3.0, 3.0, 0.0])[2] == 2
    assert TG.sim_reduce([3.0, 1.0, 3.0, 3.0])[2] == 3
    assert TG.sim_reduce([2.0, 2.0, 5.0, 2.0])[2] == 1     # ties below the maximum do not count
    assert TG.sim_reduce([0.0] * 7)[2] == 7
    assert TG.sim_reduce([5.0, 5.0, 7.0, 7.0])[1:] == (7.0, 2)  # the count starts again at a new maximum


def test_dpz_with_one_two_and_hw_tied_cells():
    # dmean = 4 over 4 cells is 1 a cell; dmax = 1 goes to the maximum, shared evenly among the cells that equal it
    assert TG.sim_dpz([1.0, 3.0, 2.0, 0.0], 4.0, 1.0).tolist() == [1.0, 2.0, 1.0, 1.0]
    assert TG.sim_dpz([1.0, 3.0, 3.0, 0.0], 4.0, 1.0).tolist() == [1.0, 1.5, 1.5, 1.0]
    assert TG.sim_dpz([3.0, 3.0, 3.0, 3.0], 4.0, 1.0).tolist() == [1.25, 1.25, 1.25, 1.25]
    assert TG.sim_dpz([0.0, 7.0], 0.0, -2.0).tolist() == [0.0, -2.0]
    assert TG.sim_dpz([1.0, 3.0, 3.0, 0.0], 4.0, 1.0).sum() == 5.0  # nothing of either gradient is lost or doubled
