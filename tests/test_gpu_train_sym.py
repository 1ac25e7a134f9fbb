"""The training step of SymmetricMLP on the device: ar_rows_grad_symmetric (alpharat_amd/csrc/train_sym.h),
RowSet.grad_symmetric_into, alpharat_amd/train.py SymmetricGradStep and RowDataset.grad_iter, against the reference's own
step (tests/golden/train_sym) and the float64 restatement (tests/_train_sym_np.py) over rows of tests/_rows.py boards with the
NumPy augmentation. Section by section tests/test_gpu_train.py.

Every tolerance is measured, not chosen (tests/_train.py grad_bounds): with a64 the float64 array and a_ref32 the reference's
own float32 evaluation (the golden's f32 arrays; tests/_sym_torch.py with autograd in float32 on the device elsewhere, tied
to the reference by tests/test_train_sym_np.py), the library must satisfy
    max|a_lib - a64| <= 8 * max(max|a_ref32 - a64|, 2^-23 * floor),
floor = max|g64 of the same layer's weight gradient| for a gradient and max|a64| for an output, a loss or a running
statistic. Error and bound of every array are printed. Every fixture passes the ReLU guard (tests/test_train_sym_np.py): none
of the seven BatchNorm outputs is within 1e-4 of zero, so no ReLU mask depends on rounding.

Measured on an MI355X, the largest err / bound over this file: 0.20 for a gradient (trunk.5.bias, the unswapped rows), 0.19
for an output, 0.34 for a loss and 0.34 for a running statistic (shared_encoder.1.running_mean at 16x16); the all-swapped
logits_p1 were the unswapped logits_p2 bit for bit."""
import numpy as np
import pytest
import torch  # before anything loads libalpharat_hip: a process brings up one HIP runtime, and torch ships its own

import _sym_torch as ST
import _train_sym as TS
import _train_sym_np as NS

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def sets():
    """one uploaded row set per board, made when first asked for; row i of the board's stacked rows is stored position i"""
    from alpharat_amd.shards import RowSet

    made = {}

    def get(board):
        if board not in made:
            games, plain = TS.board(board)
            rs = RowSet(TS.BOARDS[board][1], TS.BOARDS[board][2], len(plain["value_p1"]))
            rs.add_games(games)
            assert rs.count()[1] == len(plain["value_p1"])
            made[board] = rs
        return made[board]

    yield get
    for rs in made.values():
        rs.close()


def _device_tensors(sd):
    params = {k: torch.tensor(np.asarray(sd[k], np.float32), device=DEV) for k in NS.PARAM_KEYS}
    running = {k: torch.tensor(np.asarray(sd[k], np.float32), device=DEV) for k in NS.RUNNING_KEYS}
    grads = {k: torch.full_like(v, float("nan")) for k, v in params.items()}
    return params, grads, running


def _out(n):
    return dict(losses=torch.full((6,), float("nan"), device=DEV), logits_p1=torch.empty((n, 5), device=DEV),
                logits_p2=torch.empty((n, 5), device=DEV), value_p1=torch.empty(n, device=DEV), value_p2=torch.empty(n, device=DEV))


def _numpy(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _hidden(case):
    return case["sd"]["trunk.4.weight"].shape[0]


def _run(rs, case, first=0, n=None, set_order=True):
    """the step over rows first .. first + n of the case's order: numpy grads (NaN-filled before), running, out"""
    if set_order:
        rs.set_order(np.asarray(case["order"], np.uint64), case["swap"])
    n = len(case["order"]) - first if n is None else n
    params, grads, running = _device_tensors(case["sd"])
    out = _out(n)
    rs.grad_symmetric_into(first, n, _hidden(case), params, grads, running, case["policy_weight"], case["value_weight"], out)
    return _numpy(grads), _numpy(running), _numpy(out)


def _check_forward(out, running, want, ref32, what):
    TS.assert_values_within(out, want, ref32, NS.OUT_KEYS, what)
    TS.assert_values_within(dict(zip(NS.LOSS_KEYS, out["losses"])), want["losses"], ref32["losses"], NS.LOSS_KEYS, what)
    TS.assert_values_within(running, want["running"], ref32["running"], NS.RUNNING_KEYS, what)


def _check_case(rs, case, what, **kw):
    """a step against the float64 restatement, with the float32 autograd restatement on the device as the reference error"""
    want = NS.step(case)
    ref32 = ST.step(case, torch.float32, DEV)
    grads, running, out = _run(rs, case, **kw)
    _check_forward(out, running, want, ref32, what)
    TS.assert_grads_within(grads, want["grads"], ref32["grads"], what)
    return grads, out


# ---- 1. the reference's own step -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TS.GOLDEN)
def test_goldens(sets, name):
    case = TS.golden_case(name)
    grads, running, out = _run(sets(case["board"]), case)
    _check_forward(out, running, case["f64"], case["f32"], name)
    TS.assert_grads_within(grads, case["f64"]["grads"], case["f32"]["grads"], name)


# ---- 2. shapes: a batch of two, tails of rows and of K, several column partitions and batch splits, the full width, NW = 4 --
@pytest.mark.parametrize("shape", TS.SHAPES, ids=TS.SHAPE_IDS)
def test_shapes(sets, shape):
    _check_case(sets(shape[0]), TS.shape_case(*shape), TS.SHAPE_IDS[TS.SHAPES.index(shape)])


# ---- 3. windows of one order -------------------------------------------------------------------------------------------------
def test_windows_of_one_order(sets):
    whole, windows = TS.window_cases()
    rs = sets(TS.WINDOW_BOARD)
    rs.set_order(np.asarray(whole["order"], np.uint64), whole["swap"])
    for (first, n), case in zip(TS.WINDOWS, windows):
        want = NS.step(case)
        ref32 = ST.step(case, torch.float32, DEV)
        grads, running, out = _run(rs, whole, first=first, n=n, set_order=False)
        _check_forward(out, running, want, ref32, f"window {first}+{n}")
        TS.assert_grads_within(grads, want["grads"], ref32["grads"], f"window {first}+{n}")


# ---- 4. swapped rows: the players exchanged ---------------------------------------------------------------------------------
def test_swapped_rows(sets):
    plain, swapped = TS.swap_cases()
    rs = sets(TS.SWAP_BOARD)
    _, out_plain = _check_case(rs, plain, "unswapped")
    _, out_swapped = _check_case(rs, swapped, "all swapped")
    want = NS.step(plain)
    ref32 = ST.step(plain, torch.float32, DEV)
    bound = TS.value_bound(want["logits_p2"], ref32["logits_p2"])
    err = float(np.abs(out_swapped["logits_p1"].astype(np.float64) - out_plain["logits_p2"]).max())
    print(f"swapped logits_p1 against unswapped logits_p2: {err:.3e}, the output bound {bound:.3e}")
    assert err <= bound
    assert np.abs(out_swapped["logits_p1"] - out_plain["logits_p1"]).max() > 1e-3


# ---- 5. determinism, and overwriting rather than accumulating --------------------------------------------------------------
def test_same_request_same_bytes(sets):
    case = TS.shape_case(*TS.SHAPES[3])  # several row blocks, several batch partitions
    rs = sets(case["board"])
    a, ra, oa = _run(rs, case)
    b, rb, ob = _run(rs, case, set_order=False)
    for k in NS.PARAM_KEYS:
        assert np.isfinite(a[k]).all(), k  # NaN before the step: overwritten, not accumulated into
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in oa:
        assert oa[k].tobytes() == ob[k].tobytes(), k
    for k in ra:
        assert ra[k].tobytes() == rb[k].tobytes(), k


# ---- 6. SymmetricGradStep on a stream of torch's -----------------------------------------------------------------------------
def test_step_on_a_side_stream(sets):
    from alpharat_amd.train import SymmetricGradStep

    case = TS.shape_case(*TS.SHAPES[2])
    rs = sets(case["board"])
    rs.set_order(np.asarray(case["order"], np.uint64), case["swap"])
    n = len(case["order"])
    model = ST.Symmetric(case["width"], case["height"], _hidden(case), sd=case["sd"]).to(DEV)
    step = SymmetricGradStep(model, case["policy_weight"], case["value_weight"])
    want = NS.step(case)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        model.train()
        model.zero_grad(set_to_none=True)
        losses, l1, l2, v1, v2 = step.step(rs, 0, n, outputs=True)
    side.synchronize()
    named = dict(model.named_parameters())
    for k in NS.PARAM_KEYS:
        assert named[k].grad is step.grads[k], k
    buffers = dict(model.named_buffers())
    assert [int(buffers[f"{bn}.num_batches_tracked"]) for bn in NS.BN_MODULES] == [1, 2, 2, 2]
    out = dict(losses=losses.cpu().numpy(), logits_p1=l1.cpu().numpy(), logits_p2=l2.cpu().numpy(), value_p1=v1.cpu().numpy(),
               value_p2=v2.cpu().numpy())
    running = {k: buffers[k].cpu().numpy() for k in NS.RUNNING_KEYS}
    ref32 = ST.step(case, torch.float32, DEV)
    _check_forward(out, running, want, ref32, "side stream")
    TS.assert_grads_within({k: step.grads[k].cpu().numpy() for k in NS.PARAM_KEYS}, want["grads"], ref32["grads"], "side stream")
    # eval mode: the running statistics and the counters stay
    model.eval()
    before = {k: v.clone() for k, v in model.named_buffers()}
    losses2 = step.step(rs, 0, n)
    torch.cuda.synchronize()
    for k, v in model.named_buffers():
        assert torch.equal(v, before[k]), k
    assert losses2.cpu().numpy().tobytes() == out["losses"].tobytes()  # the weights did not move: the same batch statistics


# ---- 7. five steps of SGD ------------------------------------------------------------------------------------------------------
def test_trajectory(sets):
    from alpharat_amd.dataset import RowDataset
    from alpharat_amd.train import SymmetricGradStep

    f64 = TS.trajectory_cases_f64()
    rs = sets(TS.TRAJ_BOARD)
    ds = RowDataset(rs)
    sd0 = f64[0]["case"]["sd"]
    w, h = TS.BOARDS[TS.TRAJ_BOARD][1], TS.BOARDS[TS.TRAJ_BOARD][2]
    # the library: grad_iter + SGD
    model = ST.Symmetric(w, h, TS.TRAJ_H, sd=sd0).to(DEV).train()
    step = SymmetricGradStep(model, TS.WEIGHTS["policy_weight"], TS.WEIGHTS["value_weight"])
    opt = torch.optim.SGD(model.parameters(), lr=TS.TRAJ_LR)
    lib_losses, epoch = [], 0
    while len(lib_losses) < TS.TRAJ_STEPS:
        for n, losses in ds.grad_iter(step, TS.TRAJ_BATCH, epoch=epoch, seed=TS.TRAJ_PLAN_SEED, augment=False):
            opt.step()
            lib_losses.append(losses)
            if len(lib_losses) == TS.TRAJ_STEPS:
                break
        epoch += 1
    lib_losses = [float(l.cpu()[5]) for l in lib_losses]
    lib = {k: v.detach().cpu().numpy() for k, v in model.named_parameters()}
    # the reference error: the restated model with autograd, float32, the same batches from epoch_iter
    p = {k: torch.tensor(np.asarray(sd0[k], np.float32), device=DEV, requires_grad=True) for k in NS.PARAM_KEYS}
    running = {k: torch.tensor(np.asarray(sd0[k], np.float32), device=DEV) for k in NS.RUNNING_KEYS}
    opt = torch.optim.SGD(list(p.values()), lr=TS.TRAJ_LR)
    ref_losses, epoch = [], 0
    while len(ref_losses) < TS.TRAJ_STEPS:
        for b in ds.epoch_iter(TS.TRAJ_BATCH, epoch=epoch, seed=TS.TRAJ_PLAN_SEED, augment=False):
            opt.zero_grad()
            ls = ST.losses(ST.forward(p, b["observation"], w, h, running), b["policy_p1"], b["policy_p2"], b["value_p1"],
                           b["value_p2"], TS.WEIGHTS["policy_weight"], TS.WEIGHTS["value_weight"])
            ls["loss"].backward()
            opt.step()
            ref_losses.append(float(ls["loss"].detach().cpu()))
            if len(ref_losses) == TS.TRAJ_STEPS:
                break
        epoch += 1
    ref = {k: v.detach().cpu().numpy() for k, v in p.items()}
    final = f64[-1]["after"]
    # the four biases in front of a BatchNorm: their gradient is rounding noise, no two implementations agree on them
    TS.assert_grads_within(lib, {k: final[k] for k in NS.PARAM_KEYS}, ref, "after five steps", skip=NS.NOISE_BIASES)
    for i, s in enumerate(f64):
        want = float(s["result"]["losses"]["loss"])
        bound = 8.0 * max(abs(ref_losses[i] - want), 2.0 ** -23 * abs(want))
        print(f"step {i}: loss {lib_losses[i]!r} f64 {want!r} ref32 {ref_losses[i]!r} bound {bound:.3e}")
        assert abs(lib_losses[i] - want) <= bound, i


# ---- 8. refusals: an exception, and nothing written -----------------------------------------------------------------------------
def test_refusals(sets):
    from alpharat_amd import _lib
    from alpharat_amd.shards import SYM_PARAM_KEYS, RowSet
    from _random_nets import random_symmetric
    import ctypes as C

    case = TS.shape_case(*TS.SHAPES[1])
    rs = sets(case["board"])
    H, n = 32, len(case["order"])
    params, grads, running = _device_tensors(case["sd"])

    def untouched(g):
        torch.cuda.synchronize()
        for k, t in g.items():
            if t.is_cuda:
                assert torch.isnan(t).all(), k

    def refused(rowset, first, rows, hidden=H, p=params, g=grads, r=running):
        with pytest.raises(ValueError):
            rowset.grad_symmetric_into(first, rows, hidden, p, g, r, 1.0, 0.5, _out(rows))
        untouched(g)

    games, plain = TS.board(case["board"])
    with RowSet(5, 5, len(plain["value_p1"])) as fresh:  # no order
        fresh.add_games(games)
        refused(fresh, 0, 2)
    rs.set_order(np.asarray(case["order"], np.uint64), case["swap"])
    refused(rs, n - 3, 4)   # a window beyond the order
    refused(rs, n, 2)
    refused(rs, 0, 1)       # a training BatchNorm over one row
    p40, g40, r40 = _device_tensors(random_symmetric(5, 5, 40, 1))
    refused(rs, 0, n, hidden=40, p=p40, g=g40, r=r40)     # not a multiple of 32
    p288, g288, r288 = _device_tensors(random_symmetric(5, 5, 288, 1))
    refused(rs, 0, n, hidden=288, p=p288, g=g288, r=r288)  # above 256
    refused(rs, 0, n, g=dict(grads, **{"trunk.4.weight": torch.full((H, H), float("nan"))}))  # a CPU tensor among the grads
    # a row count above the cap, and a null pointer among the tensors: at the C interface, where the wrapper's checks are not
    big = np.arange(65537, dtype=np.uint64) % len(plain["value_p1"])
    rs.set_order(big, None)
    refused(rs, 0, 65537)
    rs.set_order(np.asarray(case["order"], np.uint64), case["swap"])
    p_c = _lib.ArSymTensors(*[params[k].data_ptr() for k in SYM_PARAM_KEYS])
    g_c = _lib.ArSymTensors(*[grads[k].data_ptr() if k != "trunk.1.bias" else None for k in SYM_PARAM_KEYS])
    rc = _lib.load().ar_rows_grad_symmetric(rs._handle(), 0, n, H, C.byref(p_c), C.byref(g_c), None, 1.0, 0.5, None, None)
    assert rc == _lib.AR_E_INVALID and "null tensor" in _lib.last_error()
    untouched(grads)
    host = np.zeros(H, np.float32)  # host memory among the grads
    g_c = _lib.ArSymTensors(*[grads[k].data_ptr() if k != "trunk.1.bias" else host.ctypes.data for k in SYM_PARAM_KEYS])
    rc = _lib.load().ar_rows_grad_symmetric(rs._handle(), 0, n, H, C.byref(p_c), C.byref(g_c), None, 1.0, 0.5, None, None)
    assert rc == _lib.AR_E_INVALID and "not device memory" in _lib.last_error()
    untouched(grads)
    assert not host.any()
    grads_after, _, out = _run(rs, case)  # and the set still works
    assert np.isfinite(out["losses"]).all() and all(np.isfinite(v).all() for v in grads_after.values())


# ---- 9. ar_rows_clear waits for a pending step ------------------------------------------------------------------------------------
def test_clear_waits_for_the_step():
    """clear, and new games over the old records, right behind a launch: the step still read the rows it was asked for"""
    from alpharat_amd.shards import RowSet

    case = TS.shape_case(*TS.SHAPES[3])
    games, plain = TS.board(case["board"])
    n, H = len(case["order"]), _hidden(case)
    with RowSet(TS.BOARDS[case["board"]][1], TS.BOARDS[case["board"]][2], len(plain["value_p1"])) as rs:
        rs.add_games(games)
        want, _, want_out = _run(rs, case)
        params, grads, running = _device_tensors(case["sd"])
        out = _out(n)
        torch.cuda.synchronize()
        rs.grad_symmetric_into(0, n, H, params, grads, running, 1.0, 0.5, out)
        rs.clear()
        assert rs.count() == (0, 0)
        rs.add_games(games[::-1])  # other records where the step's rows were
        losses = out["losses"].cpu().numpy()
        assert np.isfinite(losses).all() and losses.tobytes() == want_out["losses"].tobytes()
        for k in NS.PARAM_KEYS:
            assert grads[k].cpu().numpy().tobytes() == want[k].tobytes(), k
        with pytest.raises(ValueError):  # the order went with the games
            rs.grad_symmetric_into(0, n, H, params, grads, running, 1.0, 0.5, out)
