"""The training step of LocalValueMLP on the device: ar_rows_grad_local_value (alpharat_amd/csrc/train_lv.h),
RowSet.grad_local_value_into, alpharat_amd/train.py LocalValueGradStep and RowDataset.grad_iter, against the reference's own
step (tests/golden/train_lv) and the float64 restatement (tests/_train_lv_np.py) over rows of tests/_rows.py boards with the
NumPy augmentation. Section by section tests/test_gpu_train_sym.py.

Every tolerance is measured, not chosen (tests/_train.py grad_bounds): with a64 the float64 array and a_ref32 the reference's
own float32 evaluation (the golden's f32 arrays; tests/_lv_torch.py with autograd in float32 on the device elsewhere, tied to
the reference by tests/test_train_lv_np.py), the library must satisfy
    max|a_lib - a64| <= 8 * max(max|a_ref32 - a64|, 2^-23 * floor),
floor = max|g64 of the same layer's weight gradient| for a gradient (ownership_head.N.bias -> ownership_head.N.weight) and
max|a64| for an output, a loss or a running statistic; loss_ownership counts as a loss and ownership_logits as an output.
Error and bound of every array are printed. Every fixture passes the ReLU guard (tests/test_train_lv_np.py): neither
BatchNorm output of the trunk nor the ownership head's hidden pre-activation is within 1e-4 of zero, so no ReLU mask depends
on rounding.

Measured on an MI355X, the largest err / bound over this file: 0.34 for a gradient (trunk.5.weight), 0.32 for an output
(logits_p1), 0.65 for a loss (loss_value_p2) and 0.22 for a running statistic (trunk.1.running_mean), all four at 15x11 H96
n=40. Of the new arrays: 0.23 for ownership_head.0.bias, 0.20 for ownership_head.0.weight, 0.21 for ownership_head.2.weight,
0.15 for ownership_head.2.bias, 0.27 for ownership_logits and 0.07 for loss_ownership."""
import numpy as np
import pytest
import torch  # before anything loads libalpharat_hip: a process brings up one HIP runtime, and torch ships its own

import _lv_torch as LT
import _mlp_torch as MT
import _train_lv as TL
import _train_lv_np as NL
import _train_np as N

pytestmark = pytest.mark.gpu

DEV = "cuda"
OUT_KEYS = NL.OUT_KEYS


@pytest.fixture(scope="module")
def sets():
    """one uploaded row set per board, made when first asked for; row i of the board's stacked rows is stored position i"""
    from alpharat_amd.shards import RowSet

    made = {}

    def get(board):
        if board not in made:
            games, plain = TL.board(board)
            rs = RowSet(TL.BOARDS[board][1], TL.BOARDS[board][2], len(plain["value_p1"]))
            rs.add_games(games)
            assert rs.count()[1] == len(plain["value_p1"])
            made[board] = rs
        return made[board]

    yield get
    for rs in made.values():
        rs.close()


def _device_tensors(sd, keys=NL.PARAM_KEYS):
    params = {k: torch.tensor(np.asarray(sd[k], np.float32), device=DEV) for k in keys}
    running = {k: torch.tensor(np.asarray(sd[k], np.float32), device=DEV) for k in NL.RUNNING_KEYS}
    grads = {k: torch.full_like(v, float("nan")) for k, v in params.items()}
    return params, grads, running


def _out(n, h, w):
    return dict(losses=torch.full((7,), float("nan"), device=DEV), logits_p1=torch.empty((n, 5), device=DEV),
                logits_p2=torch.empty((n, 5), device=DEV), value_p1=torch.empty(n, device=DEV), value_p2=torch.empty(n, device=DEV),
                ownership_logits=torch.full((n, h, w, 4), float("nan"), device=DEV))


def _numpy(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _hidden(case):
    return case["sd"]["trunk.4.weight"].shape[0]


def _run(rs, case, first=0, n=None, set_order=True, ownership_weight=None):
    """the step over rows first .. first + n of the case's order: numpy grads (NaN-filled before), running, out"""
    if set_order:
        rs.set_order(np.asarray(case["order"], np.uint64), case["swap"])
    n = len(case["order"]) - first if n is None else n
    params, grads, running = _device_tensors(case["sd"])
    out = _out(n, case["height"], case["width"])
    ow = case["ownership_weight"] if ownership_weight is None else ownership_weight
    rs.grad_local_value_into(first, n, _hidden(case), params, grads, running, case["policy_weight"], case["value_weight"], ow, out)
    return _numpy(grads), _numpy(running), _numpy(out)


def _check_forward(out, running, want, ref32, what):
    TL.assert_values_within(out, want, ref32, OUT_KEYS, what)
    TL.assert_values_within(dict(zip(NL.LOSS_KEYS, out["losses"])), want["losses"], ref32["losses"], NL.LOSS_KEYS, what)
    TL.assert_values_within(running, want["running"], ref32["running"], NL.RUNNING_KEYS, what)


def _check_case(rs, case, what, **kw):
    """a step against the float64 restatement, with the float32 autograd restatement on the device as the reference error"""
    want = NL.step(case)
    ref32 = LT.step(case, torch.float32, DEV)
    grads, running, out = _run(rs, case, **kw)
    _check_forward(out, running, want, ref32, what)
    TL.assert_grads_within(grads, want["grads"], ref32["grads"], what)
    return grads, out, want


# ---- 1. the reference's own step -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TL.GOLDEN)
def test_goldens(sets, name):
    case = TL.golden_case(name)
    grads, running, out = _run(sets(case["board"]), case)
    _check_forward(out, running, case["f64"], case["f32"], name)
    TL.assert_grads_within(grads, case["f64"]["grads"], case["f32"]["grads"], name)


# ---- 2. shapes: a batch of two, tails of rows, of N and of K (4 hw = 100), several column parts and batch splits, NW = 4,
# ---- 4 hw = 1024 rows of dWo2 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", TL.SHAPES, ids=TL.SHAPE_IDS)
def test_shapes(sets, shape):
    _check_case(sets(shape[0]), TL.shape_case(*shape), TL.SHAPE_IDS[TL.SHAPES.index(shape)])


# ---- 3. windows of one order -------------------------------------------------------------------------------------------------
def test_windows_of_one_order(sets):
    whole, windows = TL.window_cases()
    rs = sets(TL.WINDOW_BOARD)
    rs.set_order(np.asarray(whole["order"], np.uint64), whole["swap"])
    for (first, n), case in zip(TL.WINDOWS, windows):
        want = NL.step(case)
        ref32 = LT.step(case, torch.float32, DEV)
        grads, running, out = _run(rs, whole, first=first, n=n, set_order=False)
        _check_forward(out, running, want, ref32, f"window {first}+{n}")
        TL.assert_grads_within(grads, want["grads"], ref32["grads"], f"window {first}+{n}")


# ---- 4. swapped rows: the players exchanged, and with them the outcome classes 0 and 3 ----------------------------------------
def test_swapped_rows(sets):
    plain, swapped = TL.swap_cases()
    assert ((plain["cheese_outcomes"] == 0) | (plain["cheese_outcomes"] == 3)).any()
    rs = sets(TL.SWAP_BOARD)
    g_plain, _, _ = _check_case(rs, plain, "unswapped")
    g_swapped, _, want = _check_case(rs, swapped, "all swapped")
    # the step with the unswapped targets over the swapped rows is a different one, further away than the bound
    wrong = NL.step(dict(swapped, cheese_outcomes=plain["cheese_outcomes"]))["grads"]["ownership_head.2.bias"]
    bound = TL.TR.grad_bounds(want["grads"], LT.step(swapped, torch.float32, DEV)["grads"])["ownership_head.2.bias"]
    assert np.abs(wrong - want["grads"]["ownership_head.2.bias"]).max() > 100 * bound
    assert np.abs(g_swapped["ownership_head.2.bias"] - g_plain["ownership_head.2.bias"]).max() > 100 * bound


# ---- 5. determinism, and overwriting rather than accumulating --------------------------------------------------------------
def test_same_request_same_bytes(sets):
    case = TL.shape_case(*TL.SHAPES[3])  # several row blocks, several batch partitions, several row parts of cells
    rs = sets(case["board"])
    a, ra, oa = _run(rs, case)
    b, rb, ob = _run(rs, case, set_order=False)
    for k in NL.PARAM_KEYS:
        assert np.isfinite(a[k]).all(), k  # NaN before the step: overwritten, not accumulated into
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in oa:
        assert np.isfinite(oa[k]).all(), k
        assert oa[k].tobytes() == ob[k].tobytes(), k
    for k in ra:
        assert ra[k].tobytes() == rb[k].tobytes(), k


# ---- 6. cells that are never active in the window: exactly zero ----------------------------------------------------------------
@pytest.mark.parametrize("shape", [TL.SHAPES[1], TL.SHAPES[4]], ids=[TL.SHAPE_IDS[1], TL.SHAPE_IDS[4]])
def test_never_active_cells_get_exactly_zero(sets, shape):
    case = TL.shape_case(*shape)
    grads, _, _ = _run(sets(case["board"]), case)
    never = ~(case["cheese_outcomes"].reshape(len(case["order"]), -1) >= 0).any(axis=0)
    assert never.any() and not never.all()
    gw = grads["ownership_head.2.weight"].reshape(len(never), 4, -1)
    gb = grads["ownership_head.2.bias"].reshape(len(never), 4)
    assert not gw[never].any() and not gb[never].any()
    assert all(gw[c].any() and gb[c].any() for c in np.flatnonzero(~never))


# ---- 7. ownership_weight 0: PyRatMLP's fourteen gradients -----------------------------------------------------------------------
def test_ownership_weight_zero_gives_the_mlps_gradients(sets):
    case = TL.shape_case(*TL.SHAPES[2])
    mlp = TL.mlp_case(case)
    want, ref32 = N.step(mlp), MT.step(mlp, torch.float32, DEV)
    grads, running, out = _run(sets(case["board"]), case, ownership_weight=0.0)
    TL.assert_grads_within({k: grads[k] for k in N.PARAM_KEYS}, want["grads"], ref32["grads"], "ownership_weight 0")
    for k in NL.OWN_KEYS:
        assert not grads[k].any(), k
    losses = dict(zip(NL.LOSS_KEYS, out["losses"]))
    TL.assert_values_within(losses, want["losses"], ref32["losses"], N.LOSS_KEYS, "ownership_weight 0")
    assert losses["loss_ownership"] > 0.1  # reported, not weighted in
    # and the weight is where it belongs: with it, the loss moves by ownership_weight * loss_ownership
    _, _, out_w = _run(sets(case["board"]), case, set_order=False)
    assert abs(float(out_w["losses"][5]) - float(out["losses"][5]) - case["ownership_weight"] * float(out["losses"][6])) <= 1e-5


# ---- 8. LocalValueGradStep on a stream of torch's ---------------------------------------------------------------------------------
def test_step_on_a_side_stream(sets):
    from alpharat_amd.train import LocalValueGradStep

    case = TL.shape_case(*TL.SHAPES[2])
    rs = sets(case["board"])
    rs.set_order(np.asarray(case["order"], np.uint64), case["swap"])
    n = len(case["order"])
    model = LT.LocalValue(case["width"], case["height"], _hidden(case), sd=case["sd"]).to(DEV)
    step = LocalValueGradStep(model, case["policy_weight"], case["value_weight"], case["ownership_weight"])
    want = NL.step(case)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        model.train()
        model.zero_grad(set_to_none=True)
        losses, l1, l2, v1, v2, lo = step.step(rs, 0, n, outputs=True)
    side.synchronize()
    assert losses.shape == (7,) and lo.shape == (n, case["height"], case["width"], 4)
    named = dict(model.named_parameters())
    for k in NL.PARAM_KEYS:
        assert named[k].grad is step.grads[k], k
    buffers = dict(model.named_buffers())
    assert [int(buffers[f"{bn}.num_batches_tracked"]) for bn in ("trunk.1", "trunk.5")] == [1, 1]
    out = dict(losses=losses.cpu().numpy(), logits_p1=l1.cpu().numpy(), logits_p2=l2.cpu().numpy(), value_p1=v1.cpu().numpy(),
               value_p2=v2.cpu().numpy(), ownership_logits=lo.cpu().numpy())
    running = {k: buffers[k].cpu().numpy() for k in NL.RUNNING_KEYS}
    ref32 = LT.step(case, torch.float32, DEV)
    _check_forward(out, running, want, ref32, "side stream")
    TL.assert_grads_within({k: step.grads[k].cpu().numpy() for k in NL.PARAM_KEYS}, want["grads"], ref32["grads"], "side stream")
    # eval mode: the running statistics and the counters stay
    model.eval()
    before = {k: v.clone() for k, v in model.named_buffers()}
    losses2 = step.step(rs, 0, n)
    torch.cuda.synchronize()
    for k, v in model.named_buffers():
        assert torch.equal(v, before[k]), k
    assert losses2.cpu().numpy().tobytes() == out["losses"].tobytes()  # the weights did not move: the same batch statistics


# ---- 9. five steps of SGD, the player swap on -------------------------------------------------------------------------------------
def test_trajectory(sets):
    from alpharat_amd.dataset import RowDataset
    from alpharat_amd.train import LocalValueGradStep

    f64 = TL.trajectory_cases_f64()
    rs = sets(TL.TRAJ_BOARD)
    ds = RowDataset(rs)
    sd0 = f64[0]["case"]["sd"]
    w, h = TL.BOARDS[TL.TRAJ_BOARD][1], TL.BOARDS[TL.TRAJ_BOARD][2]
    W = TL.WEIGHTS
    # the library: grad_iter + SGD
    model = LT.LocalValue(w, h, TL.TRAJ_H, sd=sd0).to(DEV).train()
    step = LocalValueGradStep(model, **W)
    opt = torch.optim.SGD(model.parameters(), lr=TL.TRAJ_LR)
    lib_losses, epoch = [], 0
    while len(lib_losses) < TL.TRAJ_STEPS:
        for n, losses in ds.grad_iter(step, TL.TRAJ_BATCH, epoch=epoch, seed=TL.TRAJ_PLAN_SEED):
            opt.step()
            lib_losses.append(losses)
            if len(lib_losses) == TL.TRAJ_STEPS:
                break
        epoch += 1
    lib_losses = [float(l.cpu()[5]) for l in lib_losses]
    lib = {k: v.detach().cpu().numpy() for k, v in model.named_parameters()}
    # the reference error: the restated model with autograd, float32, the same batches from epoch_iter
    p = {k: torch.tensor(np.asarray(sd0[k], np.float32), device=DEV, requires_grad=True) for k in NL.PARAM_KEYS}
    running = {k: torch.tensor(np.asarray(sd0[k], np.float32), device=DEV) for k in NL.RUNNING_KEYS}
    opt = torch.optim.SGD(list(p.values()), lr=TL.TRAJ_LR)
    ref_losses, epoch = [], 0
    while len(ref_losses) < TL.TRAJ_STEPS:
        for b in ds.epoch_iter(TL.TRAJ_BATCH, epoch=epoch, seed=TL.TRAJ_PLAN_SEED):
            opt.zero_grad()
            ls = LT.losses(LT.forward(p, b["observation"], w, h, running), b["policy_p1"], b["policy_p2"], b["value_p1"],
                           b["value_p2"], b["cheese_outcomes"], W["policy_weight"], W["value_weight"], W["ownership_weight"])
            ls["loss"].backward()
            opt.step()
            ref_losses.append(float(ls["loss"].detach().cpu()))
            if len(ref_losses) == TL.TRAJ_STEPS:
                break
        epoch += 1
    ref = {k: v.detach().cpu().numpy() for k, v in p.items()}
    final = f64[-1]["after"]
    # the two biases in front of a BatchNorm: their gradient is rounding noise, no two implementations agree on them
    TL.assert_grads_within(lib, {k: final[k] for k in NL.PARAM_KEYS}, ref, "after five steps", skip=("trunk.0.bias", "trunk.4.bias"))
    for i, s in enumerate(f64):
        want = float(s["result"]["losses"]["loss"])
        bound = 8.0 * max(abs(ref_losses[i] - want), 2.0 ** -23 * abs(want))
        print(f"step {i}: loss {lib_losses[i]!r} f64 {want!r} ref32 {ref_losses[i]!r} bound {bound:.3e}")
        assert abs(lib_losses[i] - want) <= bound, i


# ---- 10. refusals: an exception, and nothing written ------------------------------------------------------------------------------
def test_refusals(sets):
    import ctypes as C

    from alpharat_amd import _lib
    from alpharat_amd.shards import LV_PARAM_KEYS, RowSet

    case = TL.shape_case(*TL.SHAPES[1])
    rs = sets(case["board"])
    H, n = 32, len(case["order"])
    params, grads, running = _device_tensors(case["sd"])

    def untouched(g):
        torch.cuda.synchronize()
        for k, t in g.items():
            if t.is_cuda:
                assert torch.isnan(t).all(), k

    def refused(rowset, first, rows, hidden=H, p=params, g=grads, r=running, out=None):
        out = _out(rows, 5, 5) if out is None else out
        with pytest.raises(ValueError):
            rowset.grad_local_value_into(first, rows, hidden, p, g, r, 1.0, 0.5, 0.25, out)
        untouched(g)
        untouched({k: v for k, v in out.items() if k in ("losses", "ownership_logits")})

    games, plain = TL.board(case["board"])
    with RowSet(5, 5, len(plain["value_p1"])) as fresh:  # no order
        fresh.add_games(games)
        refused(fresh, 0, 2)
    rs.set_order(np.asarray(case["order"], np.uint64), case["swap"])
    refused(rs, n - 3, 4)   # a window beyond the order
    refused(rs, n, 2)
    refused(rs, 0, 1)       # a training BatchNorm over one row
    p40, g40, r40 = _device_tensors(TL.random_lv(5, 5, 40, 1, 0))
    refused(rs, 0, n, hidden=40, p=p40, g=g40, r=r40)     # not a multiple of 32
    p288, g288, r288 = _device_tensors(TL.random_lv(5, 5, 288, 1, 0))
    refused(rs, 0, n, hidden=288, p=p288, g=g288, r=r288)  # above 256
    refused(rs, 0, n, g=dict(grads, **{"ownership_head.2.weight": torch.full((100, H), float("nan"))}))  # a CPU tensor among the grads
    p14, g14, _ = _device_tensors(case["sd"], N.PARAM_KEYS)
    refused(rs, 0, n, p=p14, g=g14)  # a PyRatMLP's fourteen
    with pytest.raises(ValueError):  # and the MLP's step does not take the eighteen's outputs
        rs.grad_mlp_into(0, n, H, p14, g14, running, 1.0, 0.5, dict(losses=torch.empty(7, device=DEV)))
    # a row count above the cap, and a null or a host pointer among the tensors: at the C interface, where the wrapper's checks are not
    big = np.arange(65537, dtype=np.uint64) % len(plain["value_p1"])
    rs.set_order(big, None)
    refused(rs, 0, 65537, out=dict(losses=torch.full((7,), float("nan"), device=DEV)))
    rs.set_order(np.asarray(case["order"], np.uint64), case["swap"])
    p_c = _lib.ArLvTensors(*[params[k].data_ptr() for k in LV_PARAM_KEYS])
    g_c = _lib.ArLvTensors(*[grads[k].data_ptr() if k != "ownership_head.0.bias" else None for k in LV_PARAM_KEYS])
    call = _lib.load().ar_rows_grad_local_value
    rc = call(rs._handle(), 0, n, H, C.byref(p_c), C.byref(g_c), None, 1.0, 0.5, 0.25, None, None)
    assert rc == _lib.AR_E_INVALID and "null tensor: own0_b" in _lib.last_error()
    untouched(grads)
    host = np.zeros(100, np.float32)  # host memory among the grads
    g_c = _lib.ArLvTensors(*[grads[k].data_ptr() if k != "ownership_head.2.bias" else host.ctypes.data for k in LV_PARAM_KEYS])
    rc = call(rs._handle(), 0, n, H, C.byref(p_c), C.byref(g_c), None, 1.0, 0.5, 0.25, None, None)
    assert rc == _lib.AR_E_INVALID and "not device memory" in _lib.last_error()
    untouched(grads)
    assert not host.any()
    g_c = _lib.ArLvTensors(*[grads[k].data_ptr() for k in LV_PARAM_KEYS])
    hostl = np.zeros(n * 100, np.float32)  # host memory for the logits
    o_c = _lib.ArLvTrainOut(None, None, None, None, None, hostl.ctypes.data)
    rc = call(rs._handle(), 0, n, H, C.byref(p_c), C.byref(g_c), None, 1.0, 0.5, 0.25, C.byref(o_c), None)
    assert rc == _lib.AR_E_INVALID and "not device memory" in _lib.last_error()
    untouched(grads)
    assert not hostl.any()
    grads_after, _, out = _run(rs, case)  # and the set still works
    assert all(np.isfinite(v).all() for v in out.values()) and all(np.isfinite(v).all() for v in grads_after.values())
