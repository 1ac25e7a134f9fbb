"""The training step of PyRatMLP on the device: ar_rows_grad_mlp (alpharat_amd/csrc/train_mlp.h), RowSet.grad_mlp_into,
alpharat_amd/train.py MLPGradStep and RowDataset.grad_iter, against the reference's own step (tests/golden/train) and the
float64 restatement (tests/_train_np.py) over rows of tests/_rows.py boards with the NumPy augmentation.

The gradient tolerance is measured, not chosen (tests/_train.py grad_bounds): with g64 the float64 gradient and g_ref32 the
reference's own float32 evaluation (the golden's f32 arrays; tests/_mlp_torch.py with autograd in float32 on the device
elsewhere, tied to the reference by tests/test_train_np.py), the library must satisfy
    max|g_lib - g64| <= 8 * max(max|g_ref32 - g64|, 2^-23 * max|g64 of the same layer's weight gradient|).
Both sides are float32 evaluations of the same sums in different orders. Every fixture passes the ReLU guard
(tests/test_train_np.py): no BatchNorm output is within 1e-4 of zero, so no ReLU mask depends on rounding."""
import numpy as np
import pytest
import torch  # before anything loads libalpharat_hip: a process brings up one HIP runtime, and torch ships its own

import _mlp_torch as MT
import _train as TR
import _train_np as N

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def sets():
    """one uploaded row set per board, made when first asked for; row i of the board's stacked rows is stored position i"""
    from alpharat_amd.shards import RowSet

    made = {}

    def get(board):
        if board not in made:
            games, plain = TR.board(board)
            rs = RowSet(TR.BOARDS[board][1], TR.BOARDS[board][2], len(plain["value_p1"]))
            rs.add_games(games)
            assert rs.count()[1] == len(plain["value_p1"])
            made[board] = rs
        return made[board]

    yield get
    for rs in made.values():
        rs.close()


def _device_tensors(sd):
    params = {k: torch.tensor(np.asarray(sd[k], np.float32), device=DEV) for k in N.PARAM_KEYS}
    running = {k: torch.tensor(np.asarray(sd[k], np.float32), device=DEV) for k in N.RUNNING_KEYS}
    grads = {k: torch.full_like(v, float("nan")) for k, v in params.items()}
    return params, grads, running


def _out(n):
    return dict(losses=torch.full((6,), float("nan"), device=DEV), logits_p1=torch.empty((n, 5), device=DEV),
                logits_p2=torch.empty((n, 5), device=DEV), value_p1=torch.empty(n, device=DEV), value_p2=torch.empty(n, device=DEV))


def _numpy(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _run(rs, case, first=0, n=None, set_order=True):
    """the step over rows first .. first + n of the case's order: numpy grads (NaN-filled before), running, out"""
    if set_order:
        rs.set_order(np.asarray(case["order"], np.uint64), case["swap"])
    n = len(case["order"]) - first if n is None else n
    H = case["sd"]["trunk.0.weight"].shape[0]
    params, grads, running = _device_tensors(case["sd"])
    out = _out(n)
    rs.grad_mlp_into(first, n, H, params, grads, running, case["policy_weight"], case["value_weight"], out)
    return _numpy(grads), _numpy(running), _numpy(out)


def _check_forward(out, running, want, what):
    for k in N.OUT_KEYS:
        np.testing.assert_allclose(out[k], want[k], rtol=1e-5, atol=1e-5, err_msg=f"{what} {k}")
    losses = np.array([float(want["losses"][k]) for k in N.LOSS_KEYS])
    print(what, "losses", out["losses"], "err", np.abs(out["losses"] - losses).max())
    np.testing.assert_allclose(out["losses"], losses, rtol=1e-6, atol=1e-6, err_msg=f"{what} losses")
    for k in N.RUNNING_KEYS:
        np.testing.assert_allclose(running[k], want["running"][k], rtol=1e-6, atol=1e-6, err_msg=f"{what} {k}")


def _check_case(rs, case, what, **kw):
    """a step against the float64 restatement, with the float32 autograd restatement on the device as the reference error"""
    want = N.step(case)
    ref32 = MT.step(case, torch.float32, DEV)
    grads, running, out = _run(rs, case, **kw)
    _check_forward(out, running, want, what)
    TR.assert_grads_within(grads, want["grads"], ref32["grads"], what)
    return grads


# ---- 1. the reference's own step -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TR.GOLDEN)
def test_goldens(sets, name):
    case = TR.golden_case(name)
    grads, running, out = _run(sets(case["board"]), case)
    _check_forward(out, running, case["f64"], name)
    TR.assert_grads_within(grads, case["f64"]["grads"], case["f32"]["grads"], name)


# ---- 2. shapes: tails of rows and of K, several row blocks and batch partitions, the full width, NW = 4 -------------------
@pytest.mark.parametrize("shape", TR.SHAPES, ids=TR.SHAPE_IDS)
def test_shapes(sets, shape):
    _check_case(sets(shape[0]), TR.shape_case(*shape), TR.SHAPE_IDS[TR.SHAPES.index(shape)])


def test_value_family_head(sets):
    """pre-softplus outputs within 0.5 of 20 on both sides, above 89 and below -90 (tests/test_train_np.py asserts that
    of the float64 step): the softplus of dev_train.h and its derivative on every branch, under the measured bound"""
    case = TR.value_family_case()
    _check_case(sets(case["board"]), case, "value family")


# ---- 3. windows of one order; swapped rows ----------------------------------------------------------------------------------
def test_windows_of_one_order(sets):
    whole, windows = TR.window_cases()
    rs = sets(TR.WINDOW_BOARD)
    rs.set_order(np.asarray(whole["order"], np.uint64), whole["swap"])
    for (first, n), case in zip(TR.WINDOWS, windows):
        want = N.step(case)
        ref32 = MT.step(case, torch.float32, DEV)
        grads, running, out = _run(rs, whole, first=first, n=n, set_order=False)
        _check_forward(out, running, want, f"window {first}+{n}")
        TR.assert_grads_within(grads, want["grads"], ref32["grads"], f"window {first}+{n}")


def test_swapped_rows(sets):
    plain, swapped = TR.swap_cases()
    rs = sets(TR.SWAP_BOARD)
    g_plain = _check_case(rs, plain, "unswapped")
    g_swapped = _check_case(rs, swapped, "all swapped")
    assert not np.array_equal(g_plain["trunk.0.weight"], g_swapped["trunk.0.weight"])


# ---- 4. determinism, and overwriting rather than accumulating --------------------------------------------------------------
def test_same_request_same_bytes(sets):
    case = TR.shape_case(*TR.SHAPES[3])  # several row blocks, several batch partitions
    rs = sets(case["board"])
    a, ra, oa = _run(rs, case)
    b, rb, ob = _run(rs, case, set_order=False)
    for k in N.PARAM_KEYS:
        assert not np.isnan(a[k]).any(), k
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in oa:
        assert oa[k].tobytes() == ob[k].tobytes(), k
    for k in ra:
        assert ra[k].tobytes() == rb[k].tobytes(), k


# ---- 5. MLPGradStep on a stream of torch's -------------------------------------------------------------------------------------
def test_step_on_a_side_stream(sets):
    from alpharat_amd.train import MLPGradStep

    case = TR.shape_case(*TR.SHAPES[2])
    rs = sets(case["board"])
    rs.set_order(np.asarray(case["order"], np.uint64), case["swap"])
    n, H = len(case["order"]), case["sd"]["trunk.0.weight"].shape[0]
    model = MT.MLP(case["observation"].shape[1], H, sd=case["sd"]).to(DEV)
    step = MLPGradStep(model, case["policy_weight"], case["value_weight"])
    want = N.step(case)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        model.train()
        model.zero_grad(set_to_none=True)
        losses, l1, l2, v1, v2 = step.step(rs, 0, n, outputs=True)
    side.synchronize()
    named = dict(model.named_parameters())
    for k in N.PARAM_KEYS:
        assert named[k].grad is step.grads[k], k
    assert int(model.trunk[1].num_batches_tracked) == 1 and int(model.trunk[5].num_batches_tracked) == 1
    out = dict(losses=losses.cpu().numpy(), logits_p1=l1.cpu().numpy(), logits_p2=l2.cpu().numpy(), value_p1=v1.cpu().numpy(),
               value_p2=v2.cpu().numpy())
    running = {k: dict(model.named_buffers())[k].cpu().numpy() for k in N.RUNNING_KEYS}
    _check_forward(out, running, want, "side stream")
    ref32 = MT.step(case, torch.float32, DEV)
    TR.assert_grads_within({k: step.grads[k].cpu().numpy() for k in N.PARAM_KEYS}, want["grads"], ref32["grads"], "side stream")
    # eval mode: the running statistics and the counters stay
    model.eval()
    before = {k: v.clone() for k, v in model.named_buffers()}
    losses2 = step.step(rs, 0, n)
    torch.cuda.synchronize()
    for k, v in model.named_buffers():
        assert torch.equal(v, before[k]), k
    assert losses2.cpu().numpy().tobytes() == out["losses"].tobytes()  # the weights did not move: the same batch statistics


# ---- 6. five steps of SGD ------------------------------------------------------------------------------------------------------
def test_trajectory(sets):
    from alpharat_amd.dataset import RowDataset
    from alpharat_amd.train import MLPGradStep

    f64 = TR.trajectory_cases_f64()
    rs = sets(TR.TRAJ_BOARD)
    ds = RowDataset(rs)
    sd0 = f64[0]["case"]["sd"]
    D = f64[0]["case"]["observation"].shape[1]
    # the library: grad_iter + SGD
    model = MT.MLP(D, TR.TRAJ_H, sd=sd0).to(DEV).train()
    step = MLPGradStep(model, TR.WEIGHTS["policy_weight"], TR.WEIGHTS["value_weight"])
    opt = torch.optim.SGD(model.parameters(), lr=TR.TRAJ_LR)
    lib_losses, epoch = [], 0
    while len(lib_losses) < TR.TRAJ_STEPS:
        for n, losses in ds.grad_iter(step, TR.TRAJ_BATCH, epoch=epoch, seed=TR.TRAJ_PLAN_SEED):
            opt.step()
            lib_losses.append(losses)
            if len(lib_losses) == TR.TRAJ_STEPS:
                break
        epoch += 1
    lib_losses = [float(l.cpu()[5]) for l in lib_losses]
    lib = {k: v.detach().cpu().numpy() for k, v in model.named_parameters()}
    # the reference error: the restated model with autograd, float32, the same batches from epoch_iter
    p = {k: torch.tensor(np.asarray(sd0[k], np.float32), device=DEV, requires_grad=True) for k in N.PARAM_KEYS}
    running = {k: torch.tensor(np.asarray(sd0[k], np.float32), device=DEV) for k in N.RUNNING_KEYS}
    opt = torch.optim.SGD(list(p.values()), lr=TR.TRAJ_LR)
    ref_losses, epoch = [], 0
    while len(ref_losses) < TR.TRAJ_STEPS:
        for b in ds.epoch_iter(TR.TRAJ_BATCH, epoch=epoch, seed=TR.TRAJ_PLAN_SEED):
            opt.zero_grad()
            ls = MT.losses(MT.forward(p, b["observation"], running), b["policy_p1"], b["policy_p2"], b["value_p1"], b["value_p2"],
                           TR.WEIGHTS["policy_weight"], TR.WEIGHTS["value_weight"])
            ls["loss"].backward()
            opt.step()
            ref_losses.append(float(ls["loss"].detach().cpu()))
            if len(ref_losses) == TR.TRAJ_STEPS:
                break
        epoch += 1
    ref = {k: v.detach().cpu().numpy() for k, v in p.items()}
    final = f64[-1]["after"]
    skip = ("trunk.0.bias", "trunk.4.bias")  # their gradient is rounding noise: no two implementations agree on them
    TR.assert_grads_within(lib, {k: final[k] for k in N.PARAM_KEYS}, ref, "after five steps", skip=skip)
    for i, s in enumerate(f64):
        want = float(s["result"]["losses"]["loss"])
        bound = 8.0 * max(abs(ref_losses[i] - want), 2.0 ** -23 * abs(want))
        print(f"step {i}: loss {lib_losses[i]!r} f64 {want!r} ref32 {ref_losses[i]!r} bound {bound:.3e}")
        assert abs(lib_losses[i] - want) <= bound, i


# ---- 7. refusals: an exception, and nothing written -----------------------------------------------------------------------------
def test_refusals(sets):
    from alpharat_amd.shards import RowSet
    from _random_nets import random_mlp

    case = TR.shape_case(*TR.SHAPES[1])
    rs = sets(case["board"])
    H, n = 32, len(case["order"])
    params, grads, running = _device_tensors(case["sd"])

    def refused(rowset, first, rows, hidden=H, p=params, g=grads, r=running):
        with pytest.raises(ValueError):
            rowset.grad_mlp_into(first, rows, hidden, p, g, r, 1.0, 0.5, _out(rows))
        torch.cuda.synchronize()
        for k, t in g.items():
            if t.is_cuda:
                assert torch.isnan(t).all(), k

    games, plain = TR.board(case["board"])
    with RowSet(5, 5, len(plain["value_p1"])) as fresh:  # no order
        fresh.add_games(games)
        refused(fresh, 0, 2)
    rs.set_order(np.asarray(case["order"], np.uint64), case["swap"])
    refused(rs, n - 3, 4)   # a window beyond the order
    refused(rs, n, 2)
    refused(rs, 0, 1)       # a training BatchNorm over one row
    p40, g40, r40 = _device_tensors(random_mlp(5, 5, 40, 1))
    refused(rs, 0, n, hidden=40, p=p40, g=g40, r=r40)
    refused(rs, 0, n, g=dict(grads, **{"trunk.4.weight": torch.full((H, H), float("nan"))}))  # a CPU tensor among the grads
    grads_after, _, out = _run(rs, case)  # and the set still works
    assert np.isfinite(out["losses"]).all() and all(np.isfinite(v).all() for v in grads_after.values())


# ---- 8. ar_rows_clear waits for a pending step ------------------------------------------------------------------------------------
def test_clear_waits_for_the_step():
    """clear, and new games over the old records, right behind a launch: the step still read the rows it was asked for"""
    from alpharat_amd.shards import RowSet

    case = TR.shape_case(*TR.SHAPES[3])
    games, plain = TR.board(case["board"])
    n, H = len(case["order"]), case["sd"]["trunk.0.weight"].shape[0]
    with RowSet(TR.BOARDS[case["board"]][1], TR.BOARDS[case["board"]][2], len(plain["value_p1"])) as rs:
        rs.add_games(games)
        want, _, want_out = _run(rs, case)
        params, grads, running = _device_tensors(case["sd"])
        out = _out(n)
        torch.cuda.synchronize()
        rs.grad_mlp_into(0, n, H, params, grads, running, 1.0, 0.5, out)
        rs.clear()
        assert rs.count() == (0, 0)
        rs.add_games(games[::-1])  # other records where the step's rows were
        losses = out["losses"].cpu().numpy()
        assert np.isfinite(losses).all() and losses.tobytes() == want_out["losses"].tobytes()
        for k in N.PARAM_KEYS:
            assert grads[k].cpu().numpy().tobytes() == want[k].tobytes(), k
        with pytest.raises(ValueError):  # the order went with the games
            rs.grad_mlp_into(0, n, H, params, grads, running, 1.0, 0.5, out)
