"""The training step of PyRatCNN on the device: ar_rows_grad_cnn (alpharat_amd/csrc/train_cnn.h), RowSet.grad_cnn_into,
alpharat_amd/train.py CNNGradStep and RowDataset.grad_iter, against the reference's own step (tests/golden/train_cnn) and
the float64 restatement (tests/_train_cnn_np.py) over rows of tests/_rows.py boards. Section by section
tests/test_gpu_train_sym.py.

Every tolerance is measured, not chosen (tests/_train.py grad_bounds, tests/_train_sym.py assert_values_within): with a64
the float64 array and a_ref32 the reference's own float32 evaluation (the golden's f32 arrays; elsewhere
tests/_cnn_train_torch.py with autograd in float32 ON THE CPU, tied to the reference by tests/test_train_cnn_np.py), the
library must satisfy
    max|a_lib - a64| <= 8 * max(max|a_ref32 - a64|, 2^-23 * floor),
floor = max|g64 of the same layer's weight gradient| for a gradient and max|a64| for an output, a loss or a running
statistic. Error and bound of every array are printed. No test runs a torch convolution on the device: MIOpen compiles
kernels at first use. Every fixture passes its ReLU guard (tests/test_train_cnn_np.py).

Measured on an MI355X, the largest err / bound over this file: 0.65 for a gradient (blocks.0.bn2.weight of the golden
cnn_5x5_c32_b2_n12), 0.71 for an output (value_p1 of the same golden), 0.61 for a loss and 0.91 for a running statistic
(blocks.0.bn2.running_var at C = 256); after two AdamW steps 0.13 for a parameter."""
import ctypes as C

import numpy as np
import pytest
import torch  # before anything loads libalpharat_hip: a process brings up one HIP runtime, and torch ships its own

import _cnn_train_torch as CT
import _train_cnn as TC
import _train_cnn_np as NC

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD, SENTINEL = 64, 12345.0


@pytest.fixture(scope="module")
def sets():
    """one uploaded row set per board, made when first asked for; row i of the board's stacked rows is stored position i.
    "player cells" is the 5x5 set of tests/_train_cnn.py player_cell_games."""
    from alpharat_amd.shards import RowSet

    made = {}

    def get(board):
        if board not in made:
            if board == "player cells":
                games, plain, _ = TC.player_cell_games()
                w, h = 5, 5
            else:
                games, plain = TC.board(board)
                w, h = TC.BOARDS[board][1], TC.BOARDS[board][2]
            rs = RowSet(w, h, len(plain["value_p1"]))
            rs.add_games(games)
            assert rs.count()[1] == len(plain["value_p1"])
            made[board] = rs
        return made[board]

    yield get
    for rs in made.values():
        rs.close()


def _guarded(shape, fill):
    """a contiguous device tensor of `shape` filled with `fill`, inside a buffer with GUARD sentinel floats on either side"""
    count = int(np.prod(shape)) if len(shape) else 1
    buf = torch.full((count + 2 * GUARD,), SENTINEL, device=DEV)
    t = buf[GUARD:GUARD + count].view(*shape)
    t.fill_(fill)
    return t, buf


def _device_tensors(sd, B):
    bufs = []

    def put(a, fill=None):
        a = np.asarray(a, np.float32)
        t, buf = _guarded(a.shape, 0.0)
        if fill is None:
            t.copy_(torch.from_numpy(a))
        else:
            t.fill_(fill)
        bufs.append(buf)
        return t

    params = {k: put(sd[k]) for k in NC.param_keys(B)}
    running = {k: put(sd[k]) for k in NC.running_keys(B)}
    grads = {k: put(sd[k], float("nan")) for k in NC.param_keys(B)}
    return params, grads, running, bufs


def _out(n, bufs=None):
    out = {}
    for k, shape in (("losses", (6,)), ("logits_p1", (n, 5)), ("logits_p2", (n, 5)), ("value_p1", (n,)), ("value_p2", (n,))):
        out[k], buf = _guarded(shape, float("nan"))
        if bufs is not None:
            bufs.append(buf)
    return out


def _guards_intact(bufs):
    torch.cuda.synchronize()
    return all(bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all()) for b in bufs)


def _numpy(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _run(rs, case, first=0, n=None, set_order=True, with_running=True):
    """the step over rows first .. first + n of the case's order: numpy grads (NaN-filled before), running, out; the guard
    floats around every tensor it was given are checked"""
    dims = TC.dims_of(case)
    if set_order:
        rs.set_order(np.asarray(case["order"], np.uint64), case["swap"])
    n = len(case["order"]) - first if n is None else n
    params, grads, running, bufs = _device_tensors(case["sd"], dims[3])
    out = _out(n, bufs)
    rs.grad_cnn_into(first, n, dims, params, grads, running if with_running else None, case["policy_weight"], case["value_weight"], out)
    assert _guards_intact(bufs)
    return _numpy(grads), _numpy(running), _numpy(out)


def _check_forward(out, running, want, ref32, what, B):
    TC.assert_values_within(out, want, ref32, NC.OUT_KEYS, what)
    TC.assert_values_within(dict(zip(NC.LOSS_KEYS, out["losses"])), want["losses"], ref32["losses"], NC.LOSS_KEYS, what)
    TC.assert_values_within(running, want["running"], ref32["running"], NC.running_keys(B), what)


def _check_case(rs, case, what, **kw):
    """a step against the float64 restatement, with the float32 autograd restatement on the CPU as the reference error"""
    B = NC.n_blocks_of(case["sd"])
    TC.use_layer_weights(B)
    want = NC.step(case)
    ref32 = CT.step(case, torch.float32, "cpu")
    grads, running, out = _run(rs, case, **kw)
    _check_forward(out, running, want, ref32, what, B)
    TC.assert_grads_within(grads, want["grads"], ref32["grads"], what)
    return grads, out


# ---- 1. the reference's own step -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TC.GOLDEN)
def test_goldens(sets, name):
    case = TC.golden_case(name)
    B = NC.n_blocks_of(case["sd"])
    TC.use_layer_weights(B)
    grads, running, out = _run(sets(case["board"]), case)
    _check_forward(out, running, case["f64"], case["f32"], name, B)
    TC.assert_grads_within(grads, case["f64"]["grads"], case["f32"]["grads"], name)


# ---- 2. shapes, with decided networks: each the smallest that reaches one thing (tests/_train_cnn.py SHAPES) ------------------
@pytest.mark.parametrize("shape", TC.SHAPES, ids=TC.SHAPE_IDS)
def test_shapes(sets, shape):
    _check_case(sets(shape[0]), TC.shape_case(*shape), TC.SHAPE_IDS[TC.SHAPES.index(shape)])


# ---- 3. windows of one order -------------------------------------------------------------------------------------------------
def test_windows_of_one_order(sets):
    whole, windows = TC.window_cases()
    B = NC.n_blocks_of(whole["sd"])
    TC.use_layer_weights(B)
    rs = sets(TC.WINDOW_BOARD)
    rs.set_order(np.asarray(whole["order"], np.uint64), whole["swap"])
    for (first, n), case in zip(TC.WINDOWS, windows):
        want = NC.step(case)
        ref32 = CT.step(case, torch.float32, "cpu")
        grads, running, out = _run(rs, whole, first=first, n=n, set_order=False)
        _check_forward(out, running, want, ref32, f"window {first}+{n}", B)
        TC.assert_grads_within(grads, want["grads"], ref32["grads"], f"window {first}+{n}")


# ---- 4. the player cells: both players on one cell, a player in each corner ------------------------------------------------------
def test_player_cells(sets):
    case = TC.player_cell_case()
    _check_case(sets("player cells"), case, "player cells")


# ---- 5. determinism, and overwriting rather than accumulating --------------------------------------------------------------
def test_same_request_same_bytes(sets):
    case = TC.shape_case(*TC.SHAPES[2])  # several parts, several splits
    rs = sets(case["board"])
    a, ra, oa = _run(rs, case)
    b, rb, ob = _run(rs, case, set_order=False)
    for k in a:
        assert np.isfinite(a[k]).all(), k  # NaN before the step: overwritten, not accumulated into
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in oa:
        assert oa[k].tobytes() == ob[k].tobytes(), k
    for k in ra:
        assert ra[k].tobytes() == rb[k].tobytes(), k


# ---- 6. running statistics -----------------------------------------------------------------------------------------------------
def test_running_statistics(sets):
    from alpharat_amd.train import CNNGradStep

    case = TC.shape_case(*TC.SHAPES[2])
    dims = TC.dims_of(case)
    B = dims[3]
    TC.use_layer_weights(B)
    rs = sets(case["board"])
    n = len(case["order"])
    # running=None: nothing is written to them
    _, running, _ = _run(rs, case, with_running=False)
    for k in NC.running_keys(B):
        assert running[k].tobytes() == np.asarray(case["sd"][k], np.float32).tobytes(), k
    # training mode: they match, and every num_batches_tracked grows by one; eval mode: they and the counters stay
    w, h = case["width"], case["height"]
    model = CT.CNN(w, h, dims[0], dims[1], dims[2], B, sd=case["sd"]).to(DEV).train()
    step = CNNGradStep(model, case["policy_weight"], case["value_weight"])
    losses, l1, l2, v1, v2 = step.step(rs, 0, n, outputs=True)
    torch.cuda.synchronize()
    named, buffers = dict(model.named_parameters()), dict(model.named_buffers())
    for k in NC.param_keys(B):
        assert named[k].grad is step.grads[k], k
    assert [int(buffers[f"{bn}.num_batches_tracked"]) for bn in NC.bn_modules(B)] == [1] * (1 + 2 * B)
    want = NC.step(case)
    ref32 = CT.step(case, torch.float32, "cpu")
    out = dict(losses=losses.cpu().numpy(), logits_p1=l1.cpu().numpy(), logits_p2=l2.cpu().numpy(), value_p1=v1.cpu().numpy(),
               value_p2=v2.cpu().numpy())
    _check_forward(out, {k: buffers[k].cpu().numpy() for k in NC.running_keys(B)}, want, ref32, "CNNGradStep", B)
    TC.assert_grads_within({k: step.grads[k].cpu().numpy() for k in NC.param_keys(B)}, want["grads"], ref32["grads"], "CNNGradStep")
    model.eval()
    before = {k: v.clone() for k, v in model.named_buffers()}
    losses2 = step.step(rs, 0, n)
    torch.cuda.synchronize()
    for k, v in model.named_buffers():
        assert torch.equal(v, before[k]), k
    assert losses2.cpu().numpy().tobytes() == out["losses"].tobytes()  # the weights did not move: the same batch statistics


# ---- 7. refusals: an exception, and nothing written -----------------------------------------------------------------------------
def test_refusals(sets):
    from alpharat_amd import _lib
    from alpharat_amd.shards import RowSet, _cnn_slots, cnn_param_keys
    from alpharat_amd.train import CNNGradStep

    case = TC.shape_case(*TC.SHAPES[1])
    rs = sets(case["board"])
    dims, n = TC.dims_of(case), len(case["order"])
    params, grads, running, _ = _device_tensors(case["sd"], 1)

    def untouched(g):
        torch.cuda.synchronize()
        for k, t in g.items():
            if t.is_cuda:
                assert torch.isnan(t).all(), k

    def refused(rowset, first, rows, d=dims, p=params, g=grads, r=running, match=None):
        with pytest.raises(ValueError, match=match):
            rowset.grad_cnn_into(first, rows, d, p, g, r, 1.0, 0.5, _out(rows))
        untouched(g)

    # what CNNGradStep finds in the model, before a row set is touched
    for kw, match in ((dict(n_blocks=2, gpool=True), "GPoolResBlock"), (dict(pooled_value=True), "PooledValueHead"),
                      (dict(dropout=0.1), "dropout"), (dict(katago=True), "KataGoCNN")):
        with pytest.raises(ValueError, match=match):
            CNNGradStep(CT.CNN(5, 5, **kw).to(DEV))
    with pytest.raises(ValueError, match="dropout"):
        CNNGradStep(CT.CNN(5, 5, dropout=0.1).to(DEV), dropout_seed=1)
    missing = CT.CNN(5, 5)
    del missing.stem_bn
    with pytest.raises(ValueError, match="stem_bn.weight"):
        CNNGradStep(missing.to(DEV))
    with pytest.raises(ValueError, match="float32|dtype"):
        CNNGradStep(CT.CNN(5, 5).double().to(DEV))
    strided = CT.CNN(5, 5)
    strided.combiner[0].weight = torch.nn.Parameter(torch.zeros(64, 64).T)
    with pytest.raises(ValueError, match="contiguous"):
        CNNGradStep(strided.to(DEV))
    with pytest.raises(ValueError, match="7x5"):  # a board that does not match
        CNNGradStep(CT.CNN(7, 5, sd=None).to(DEV)).step(rs, 0, n)
    # what the library refuses
    games, plain = TC.board(case["board"])
    with RowSet(5, 5, len(plain["value_p1"])) as fresh:  # no order
        fresh.add_games(games)
        refused(fresh, 0, 2, match="order")
    with RowSet(1, 1, 4) as tiny:  # a board of one cell: the stem's input would have fewer elements than the side vectors
        refused(tiny, 0, 2, match="2 to 256 cells")
    rs.set_order(np.asarray(case["order"], np.uint64), case["swap"])
    refused(rs, n - 1, 2)            # a window beyond the order
    refused(rs, 0, 1, match="two rows")  # a training BatchNorm over one row
    p48, g48, r48, _ = _device_tensors(NC.random_cnn(5, 5, 48, 32, 64, 1, 1), 1)
    refused(rs, 0, n, d=(48, 32, 64, 1), p=p48, g=g48, r=r48, match="channels")  # not a multiple of 32
    p40, g40, r40, _ = _device_tensors(NC.random_cnn(5, 5, 32, 32, 40, 1, 1), 1)
    refused(rs, 0, n, d=(32, 32, 40, 1), p=p40, g=g40, r=r40, match="hidden_dim")
    p9, g9, r9, _ = _device_tensors(NC.random_cnn(5, 5, 32, 32, 64, 9, 1), 9)
    refused(rs, 0, n, d=(32, 32, 64, 9), p=p9, g=g9, r=r9, match="blocks")  # nine blocks: the wrapper's refusal
    refused(rs, 0, n, g=dict(grads, **{"stem.weight": torch.full((32, 5, 3, 3), float("nan"))}))  # a CPU tensor among the grads
    # n * hw above 2^22: 16385 rows of 16x16
    big = sets("16x16")
    stored = big.count()[1]
    big.set_order(np.arange(16385, dtype=np.uint64) % stored, None)
    refused(big, 0, 16385, match="2\\^22")
    # nine blocks, and a null pointer among the tensors: at the C interface, where the wrapper's checks are not
    keys = cnn_param_keys(1)
    slots = _cnn_slots(keys, 1, 3, 6)

    def struct(d, skip=None):
        s = _lib.ArCnnTensors()
        for slot, k in zip(slots, keys):
            if k != skip:
                setattr(s, _lib.CNN_TENSORS[slot], d[k].data_ptr())
        return s

    p_c, g_c = struct(params), struct(grads)
    call = lambda d, g: _lib.load().ar_rows_grad_cnn(rs._handle(), 0, n, C.byref(_lib.ArCnnDims(*d)), C.byref(p_c), C.byref(g),  # noqa: E731
                                                     None, 1.0, 0.5, None, None)
    assert call((32, 32, 64, 9), g_c) == _lib.AR_E_INVALID and "at most 8" in _lib.last_error()
    untouched(grads)
    assert call((32, 0, 64, 1), g_c) == _lib.AR_E_INVALID and "player_dim" in _lib.last_error()
    assert call(dims, struct(grads, skip="blocks.0.conv1.weight")) == _lib.AR_E_INVALID and "null tensor" in _lib.last_error()
    untouched(grads)
    assert _lib.load().ar_rows_grad_cnn(rs._handle(), 0, n, None, C.byref(p_c), C.byref(g_c), None, 1.0, 0.5, None, None) == _lib.AR_E_INVALID
    grads_after, _, out = _run(rs, case)  # and the set still works
    assert np.isfinite(out["losses"]).all() and all(np.isfinite(v).all() for v in grads_after.values())


# ---- 8. guard rows: every _run above checks the floats around each tensor it hands over; here with every output asked for ------
def test_guards_around_every_output(sets):
    case = TC.shape_case(*TC.SHAPES[7])  # PD = 24: widths that are no multiple of a tile
    rs = sets(case["board"])
    dims, n = TC.dims_of(case), len(case["order"])
    rs.set_order(np.asarray(case["order"], np.uint64), case["swap"])
    params, grads, running, bufs = _device_tensors(case["sd"], dims[3])
    before = {k: v.clone() for k, v in params.items()}
    out = _out(n, bufs)
    rs.grad_cnn_into(0, n, dims, params, grads, running, 1.0, 0.5, out)
    assert _guards_intact(bufs)
    for k, v in params.items():  # the parameters are read only
        assert torch.equal(v, before[k]), k
    for d in (grads, out):
        for k, v in d.items():
            assert torch.isfinite(v).all(), k


# ---- 9. two steps of AdamW through grad_iter -------------------------------------------------------------------------------------
def test_two_adamw_steps(sets):
    from alpharat_amd.dataset import RowDataset
    from alpharat_amd.train import CNNGradStep

    Ch, PD, HD, B = TC.TRAJ_DIMS
    TC.use_layer_weights(B)
    w, h = TC.BOARDS[TC.TRAJ_BOARD][1], TC.BOARDS[TC.TRAJ_BOARD][2]
    sd0 = NC.random_cnn(w, h, Ch, PD, HD, B, TC.TRAJ_SEED)
    rs = sets(TC.TRAJ_BOARD)
    ds = RowDataset(rs)
    # the library: grad_iter + AdamW (the model's forward is never run: no convolution of torch's on the device)
    model = CT.CNN(w, h, Ch, PD, HD, B, sd=sd0).to(DEV).train()
    step = CNNGradStep(model, TC.WEIGHTS["policy_weight"], TC.WEIGHTS["value_weight"])
    opt = torch.optim.AdamW(model.parameters(), lr=TC.TRAJ_LR)
    lib_losses, epoch = [], 0
    while len(lib_losses) < TC.TRAJ_STEPS:
        for n, losses in ds.grad_iter(step, TC.TRAJ_BATCH, epoch=epoch, seed=TC.TRAJ_PLAN_SEED, augment=False):
            opt.step()
            lib_losses.append(losses)
            if len(lib_losses) == TC.TRAJ_STEPS:
                break
        epoch += 1
    lib_losses = [float(l.cpu()[5]) for l in lib_losses]
    lib = {k: v.detach().cpu().numpy() for k, v in model.named_parameters()}
    buffers = dict(model.named_buffers())
    assert [int(buffers[f"{bn}.num_batches_tracked"]) for bn in NC.bn_modules(B)] == [TC.TRAJ_STEPS] * (1 + 2 * B)
    # the restatement with autograd and AdamW on the CPU, in float64 and in float32, over the same batches
    epochs, steps = TC.trajectory_plan()
    plans = {e: (o, m) for e, o, m in epochs}

    def reference(dtype):
        p = {k: torch.tensor(np.asarray(sd0[k]), dtype=dtype, requires_grad=True) for k in NC.param_keys(B)}
        running = {k: torch.tensor(np.asarray(sd0[k]), dtype=dtype) for k in NC.running_keys(B)}
        opt = torch.optim.AdamW(list(p.values()), lr=TC.TRAJ_LR)
        out = []
        for e, first in steps:
            order, mask = plans[e]
            idx = order[first:first + TC.TRAJ_BATCH]
            case = TC.make_case(TC.TRAJ_BOARD, sd0, idx, mask[idx])
            t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)  # noqa: E731
            opt.zero_grad()
            ls = CT.losses(CT.forward(p, t(case["observation"]), w, h, running), t(case["policy_p1"]), t(case["policy_p2"]),
                           t(case["value_p1"]), t(case["value_p2"]), TC.WEIGHTS["policy_weight"], TC.WEIGHTS["value_weight"])
            ls["loss"].backward()
            opt.step()
            out.append(float(ls["loss"].detach()))
        return {k: v.detach().numpy() for k, v in p.items()}, out

    p64, loss64 = reference(torch.float64)
    p32, loss32 = reference(torch.float32)
    TC.assert_grads_within(lib, p64, p32, "after two AdamW steps")
    for i in range(TC.TRAJ_STEPS):
        bound = 8.0 * max(abs(loss32[i] - loss64[i]), 2.0 ** -23 * abs(loss64[i]))
        print(f"step {i}: loss {lib_losses[i]!r} f64 {loss64[i]!r} ref32 {loss32[i]!r} bound {bound:.3e}")
        assert abs(lib_losses[i] - loss64[i]) <= bound, i
