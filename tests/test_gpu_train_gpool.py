"""The training step of PyRatCNN with GPoolResBlocks and dropout on the device: ar_rows_grad_cnn_gpool
(alpharat_amd/csrc/train_gpool.h), RowSet.grad_cnn_gpool_into, alpharat_amd/train.py GPoolCNNGradStep and
RowDataset.grad_iter, against the reference's own step (tests/golden/train_gpool) and the float64 restatement
(tests/_train_gpool_np.py) over rows of tests/_rows.py boards. Section by section tests/test_gpu_train_cnn.py.

Every tolerance is that file's measured rule, unchanged: with a64 the float64 array and a_ref32 the reference's own float32
evaluation (the golden's f32 arrays; elsewhere tests/_gpool_train_torch.py with autograd in float32 ON THE CPU, tied to the
reference by tests/test_train_gpool_np.py), the library must satisfy
    max|a_lib - a64| <= 8 * max(max|a_ref32 - a64|, 2^-23 * floor),
floor = max|g64 of the same layer's weight gradient| for a gradient and max|a64| for an output, a loss or a running
statistic. Error and bound of every array are printed. No test runs a torch convolution on the device. Every fixture passes
its ReLU guard and its maximum guard (tests/test_train_gpool_np.py); the tie cases tie exactly on purpose.

Measured on an MI355X, the largest err / bound over this file: 0.73 for a gradient (value_head.linear.weight on the 2x1
board), 0.87 for an output (value_p1 of the same case), 0.23 for a loss (loss_value_p1 of the golden
gpool_5x5_c32_r_g16_n12_p10) and 0.76 for a running statistic (blocks.0.bn2.running_var at C = G = 256); after two AdamW
steps with dropout 0.13 for a parameter."""
import ctypes as C

import numpy as np
import pytest
import torch  # before anything loads libalpharat_hip: a process brings up one HIP runtime, and torch ships its own

import _cnn_train_torch as CT
import _dropout_np as D
import _gpool_train_torch as GT
import _train_cnn as TC
import _train_cnn_np as NC
import _train_gpool as TG
import _train_gpool_np as NG

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD, SENTINEL = 64, 12345.0


@pytest.fixture(scope="module")
def sets():
    """one uploaded row set per board, made when first asked for; row i of the board's stacked rows is stored position i.
    "player cells" is the 5x5 set of tests/_train_cnn.py player_cell_games, "2x1" that of tests/_train_gpool.py."""
    from alpharat_amd.shards import RowSet

    made = {}

    def get(board):
        if board not in made:
            if board == "player cells":
                games, plain, _ = TC.player_cell_games()
                w, h = 5, 5
            else:
                games, plain, w, h = TG.board_rows(board)
            rs = RowSet(w, h, len(plain["value_p1"]))
            rs.add_games(games)
            assert rs.count()[1] == len(plain["value_p1"])
            made[board] = rs
        return made[board]

    yield get
    for rs in made.values():
        rs.close()


def _guarded(shape, fill):
    count = int(np.prod(shape)) if len(shape) else 1
    buf = torch.full((count + 2 * GUARD,), SENTINEL, device=DEV)
    t = buf[GUARD:GUARD + count].view(*shape)
    t.fill_(fill)
    return t, buf


def _device_tensors(sd, blocks):
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

    params = {k: put(sd[k]) for k in NG.param_keys(blocks)}
    running = {k: put(sd[k]) for k in NG.running_keys(blocks)}
    grads = {k: put(sd[k], float("nan")) for k in NG.param_keys(blocks)}
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


def _dropout_of(case):
    return (case["p"], case["dropout_seed"], case["dropout_step"]) if case.get("masks") is not None else None


def _run(rs, case, first=0, n=None, set_order=True, with_running=True, dropout="case"):
    """the step over rows first .. first + n of the case's order: numpy grads (NaN-filled before), running, out; the guard
    floats around every tensor it was given are checked"""
    dims, blocks = TG.dims_of(case), NG.blocks_of(case["sd"])
    if set_order:
        rs.set_order(np.asarray(case["order"], np.uint64), case["swap"])
    n = len(case["order"]) - first if n is None else n
    params, grads, running, bufs = _device_tensors(case["sd"], blocks)
    out = _out(n, bufs)
    rs.grad_cnn_gpool_into(first, n, dims, blocks, params, grads, running if with_running else None, case["policy_weight"],
                           case["value_weight"], out, dropout=_dropout_of(case) if dropout == "case" else dropout)
    assert _guards_intact(bufs)
    return _numpy(grads), _numpy(running), _numpy(out)


def _check_forward(out, running, want, ref32, what, blocks):
    TC.assert_values_within(out, want, ref32, NC.OUT_KEYS, what)
    TC.assert_values_within(dict(zip(NC.LOSS_KEYS, out["losses"])), want["losses"], ref32["losses"], NC.LOSS_KEYS, what)
    TC.assert_values_within(running, want["running"], ref32["running"], NG.running_keys(blocks), what)


def _check_case(rs, case, what, **kw):
    """a step against the float64 restatement, with the float32 autograd restatement on the CPU as the reference error"""
    blocks = NG.blocks_of(case["sd"])
    TG.use_layer_weights(blocks)
    want = NG.step(case)
    ref32 = GT.step(case, torch.float32, "cpu")
    grads, running, out = _run(rs, case, **kw)
    _check_forward(out, running, want, ref32, what, blocks)
    TG.assert_grads_within(grads, want["grads"], ref32["grads"], what)
    return grads, out


# ---- 1. the reference's own step -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TG.GOLDEN)
def test_goldens(sets, name):
    case = TG.golden_case(name)
    blocks = NG.blocks_of(case["sd"])
    TG.use_layer_weights(blocks)
    grads, running, out = _run(sets(case["board"]), case)
    _check_forward(out, running, case["f64"], case["f32"], name, blocks)
    TG.assert_grads_within(grads, case["f64"]["grads"], case["f32"]["grads"], name)


# ---- 2. shapes, with decided networks: each the smallest that reaches one thing (tests/_train_gpool.py SHAPES) ----------------
@pytest.mark.parametrize("shape", TG.SHAPES, ids=TG.SHAPE_IDS)
def test_shapes(sets, shape):
    _check_case(sets(shape[0]), TG.shape_case(*shape), TG.SHAPE_IDS[TG.SHAPES.index(shape)])


# ---- 3. ties: exact in every precision, the maximum's gradient shared evenly ------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["every cell", "some channels"])
def test_ties(sets, which):
    from _train import grad_bounds

    case = TG.tie_cases()[which]
    grads, _ = _check_case(sets(case["board"]), case, f"ties {which}")
    if which == 1:
        return
    # Every cell ties, so dpz is (dmean + dmax) / hw at each cell, and with ap = relu(0 * xhat + 4) passing everything
    # pool_bn.weight.grad[c] = sum over rows and cells of dap * xhat has a closed form: dap is the same at a row's cells. A
    # first-index rule puts dmax on cell 0 alone; the sums over the cells (pool_conv.weight.grad, pool_bn.bias.grad) cannot
    # tell the two apart, this gradient can.
    want = NG.step(case)
    back, = want["pool_back"]
    key = f"blocks.{back['block']}.pool_bn.weight"
    n, hw, Ch = back["xhat"].shape
    G = back["wc"].shape[0]
    dmean, dmax = back["dcat"][:, :G], back["dcat"][:, G:]
    even = ((((dmean + dmax) / hw) @ back["wc"])[:, None, :] * back["xhat"]).sum(axis=(0, 1))
    dpz_first = np.repeat((dmean / hw)[:, None, :], hw, axis=1)
    dpz_first[:, 0, :] += dmax
    first = ((dpz_first @ back["wc"]) * back["xhat"]).sum(axis=(0, 1))
    bound = grad_bounds(want["grads"], GT.step(case, torch.float32, "cpu")["grads"])[key]
    err_even, err_first = np.abs(grads[key] - even).max(), np.abs(grads[key] - first).max()
    print(f"{key}: from the even split {err_even:.3e}, from a first-index rule {err_first:.3e}, bound {bound:.3e}")
    assert np.abs(want["grads"][key] - even).max() <= 1e-12 * max(1.0, np.abs(even).max())  # the closed form is the restatement's
    assert np.abs(even - first).max() > 100 * bound  # the two rules are far apart here
    assert err_even <= bound < err_first


# ---- 4. windows of one order, swapped rows, both players on one cell (the fixtures of tests/_train_cnn.py, this trunk) ----------
def test_windows_of_one_order(sets):
    whole, windows = TC.window_cases()
    whole = TG.with_trunk(whole)
    blocks = NG.blocks_of(whole["sd"])
    TG.use_layer_weights(blocks)
    rs = sets(TC.WINDOW_BOARD)
    rs.set_order(np.asarray(whole["order"], np.uint64), whole["swap"])
    for (first, n), case in zip(TC.WINDOWS, windows):
        case = dict(case, sd=whole["sd"])
        want = NG.step(case)
        ref32 = GT.step(case, torch.float32, "cpu")
        grads, running, out = _run(rs, whole, first=first, n=n, set_order=False)
        _check_forward(out, running, want, ref32, f"window {first}+{n}", blocks)
        TG.assert_grads_within(grads, want["grads"], ref32["grads"], f"window {first}+{n}")


def test_swapped_rows_and_player_cells(sets):
    plain, swapped = (TG.with_trunk(c) for c in TC.swap_cases())
    _, oa = _check_case(sets(plain["board"]), plain, "unswapped")
    _, ob = _check_case(sets(swapped["board"]), swapped, "all swapped")
    assert np.abs(oa["logits_p1"] - oa["logits_p2"]).max() > 1e-3
    assert np.abs(ob["logits_p1"] - oa["logits_p2"]).max() < 1e-3  # the players exchanged
    _check_case(sets("player cells"), TG.with_trunk(TC.player_cell_case()), "player cells")


# ---- 5. determinism, and overwriting rather than accumulating --------------------------------------------------------------
def test_same_request_same_bytes(sets):
    case = NG.with_masks(TG.shape_case(*TG.SHAPES[8]), TG.DROPOUT_SEED, 3, TG.DROPOUT_P)  # several parts, several splits
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
    from alpharat_amd.train import GPoolCNNGradStep

    case = TG.shape_case(*TG.SHAPES[5])  # the shipped trunk
    dims, blocks = TG.dims_of(case), NG.blocks_of(case["sd"])
    TG.use_layer_weights(blocks)
    rs = sets(case["board"])
    n = len(case["order"])
    _, running, _ = _run(rs, case, with_running=False)  # running=None: nothing is written to them
    for k in NG.running_keys(blocks):
        assert running[k].tobytes() == np.asarray(case["sd"][k], np.float32).tobytes(), k
    model = GT.GPoolCNN(case["width"], case["height"], dims[0], dims[1], dims[2], blocks, sd=case["sd"]).to(DEV).train()
    step = GPoolCNNGradStep(model, case["policy_weight"], case["value_weight"])
    losses, l1, l2, v1, v2 = step.step(rs, 0, n, outputs=True)
    torch.cuda.synchronize()
    named, buffers = dict(model.named_parameters()), dict(model.named_buffers())
    for k in NG.param_keys(blocks):
        assert named[k].grad is step.grads[k], k
    assert [int(buffers[f"{bn}.num_batches_tracked"]) for bn in NG.bn_modules(blocks)] == [1] * (2 + 2 * len(blocks))
    assert "blocks.2.pool_bn" in NG.bn_modules(blocks)
    assert not torch.equal(buffers["blocks.2.pool_bn.running_mean"].cpu(), torch.as_tensor(case["sd"]["blocks.2.pool_bn.running_mean"]))
    want = NG.step(case)
    ref32 = GT.step(case, torch.float32, "cpu")
    out = dict(losses=losses.cpu().numpy(), logits_p1=l1.cpu().numpy(), logits_p2=l2.cpu().numpy(), value_p1=v1.cpu().numpy(),
               value_p2=v2.cpu().numpy())
    _check_forward(out, {k: buffers[k].cpu().numpy() for k in NG.running_keys(blocks)}, want, ref32, "GPoolCNNGradStep", blocks)
    TG.assert_grads_within({k: step.grads[k].cpu().numpy() for k in NG.param_keys(blocks)}, want["grads"], ref32["grads"], "GPoolCNNGradStep")
    model.eval()
    before = {k: v.clone() for k, v in model.named_buffers()}
    losses2 = step.step(rs, 0, n)
    torch.cuda.synchronize()
    for k, v in model.named_buffers():
        assert torch.equal(v, before[k]), k
    assert losses2.cpu().numpy().tobytes() == out["losses"].tobytes()


# ---- 7. dropout ------------------------------------------------------------------------------------------------------------------
def test_dropout_masks_are_the_restatements():
    """the device's generator under the CNN's call numbering, at the widths ar_train_dropout_mask takes"""
    from alpharat_amd.train import dropout_mask

    for call, H in ((0, 32), (1, 32), (2, 64), (3, 64)):
        got = dropout_mask(TG.DROPOUT_SEED, 1, call, 9, H, TG.DROPOUT_P).cpu().numpy()
        assert np.array_equal(got, D.mask(TG.DROPOUT_SEED, 1, call, 9, H, TG.DROPOUT_P)), call


def test_dropout(sets):
    from alpharat_amd.train import GPoolCNNGradStep

    plain = TG.shape_case(*TG.SHAPES[5])
    dims, blocks = TG.dims_of(plain), NG.blocks_of(plain["sd"])
    TG.use_layer_weights(blocks)
    rs = sets(plain["board"])
    n = len(plain["order"])
    # p = 0 with a seed: the bytes of the run without one
    a, ra, oa = _run(rs, plain)
    b, rb, ob = _run(rs, plain, set_order=False, dropout=(0.0, TG.DROPOUT_SEED, 0))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in oa:
        assert oa[k].tobytes() == ob[k].tobytes(), k
    # training mode: two consecutive steps, each under its own step's masks
    model = GT.GPoolCNN(plain["width"], plain["height"], dims[0], dims[1], dims[2], blocks, dropout=TG.DROPOUT_P, sd=plain["sd"]).to(DEV).train()
    step = GPoolCNNGradStep(model, plain["policy_weight"], plain["value_weight"], dropout_seed=TG.DROPOUT_SEED)
    sd_now = plain["sd"]
    seen = []
    for s in (0, 1):
        assert step.dropout_step == s
        out = step.step(rs, 0, n, outputs=True)
        torch.cuda.synchronize()
        case = NG.with_masks(dict(plain, sd=sd_now), TG.DROPOUT_SEED, s, TG.DROPOUT_P)
        want = NG.step(case)
        ref32 = GT.step(case, torch.float32, "cpu")
        got = dict(zip(("losses",) + NC.OUT_KEYS, (t.cpu().numpy() for t in out)))
        buffers = dict(model.named_buffers())
        _check_forward(got, {k: buffers[k].cpu().numpy() for k in NG.running_keys(blocks)}, want, ref32, f"dropout step {s}", blocks)
        TG.assert_grads_within({k: step.grads[k].cpu().numpy() for k in NG.param_keys(blocks)}, want["grads"], ref32["grads"],
                               f"dropout step {s}")
        seen.append(got["losses"].copy())
        # the second step starts from the running statistics the first one left (the weights do not move: no optimiser)
        sd_now = dict(plain["sd"], **{k: buffers[k].cpu().numpy() for k in NG.running_keys(blocks)})
    assert step.dropout_step == 2 and seen[0].tobytes() != seen[1].tobytes()  # other masks
    assert seen[0].tobytes() != oa["losses"].tobytes()  # and a mask was applied at all
    # eval mode: no mask, the counter stays
    model.eval()
    losses = step.step(rs, 0, n)
    torch.cuda.synchronize()
    assert step.dropout_step == 2 and losses.cpu().numpy().tobytes() == oa["losses"].tobytes()


# ---- 8. a trunk of ResBlocks: CNNGradStep's bytes ------------------------------------------------------------------------------
def test_resblock_model_gives_cnn_grad_steps_bytes(sets):
    from alpharat_amd.train import CNNGradStep, GPoolCNNGradStep

    case = TC.shape_case(*TC.SHAPES[2])  # 7x5, C = 64, two blocks, n = 33
    dims = TC.dims_of(case)
    rs = sets(case["board"])
    rs.set_order(np.asarray(case["order"], np.uint64), case["swap"])
    n = len(case["order"])
    results = []
    for cls in (CNNGradStep, GPoolCNNGradStep):
        model = CT.CNN(case["width"], case["height"], dims[0], dims[1], dims[2], dims[3], sd=case["sd"]).to(DEV).train()
        step = cls(model, case["policy_weight"], case["value_weight"])
        out = step.step(rs, 0, n, outputs=True)
        torch.cuda.synchronize()
        results.append(([t.cpu().numpy().tobytes() for t in out], {k: v.cpu().numpy().tobytes() for k, v in step.grads.items()},
                        {k: v.cpu().numpy().tobytes() for k, v in model.named_buffers()}))
    assert results[1][1].keys() == results[0][1].keys()
    assert results[0] == results[1]


# ---- 9. refusals: an exception, and nothing written -----------------------------------------------------------------------------
def test_refusals(sets):
    from alpharat_amd import _lib
    from alpharat_amd.shards import _cnn_gpool_structs
    from alpharat_amd.train import GPoolCNNGradStep

    case = TG.shape_case(*TG.SHAPES[0])
    rs = sets(case["board"])
    dims, blocks, n = TG.dims_of(case), NG.blocks_of(case["sd"]), len(case["order"])
    params, grads, running, _ = _device_tensors(case["sd"], blocks)

    def untouched():
        torch.cuda.synchronize()
        for k, t in grads.items():
            assert torch.isnan(t).all(), k

    # what GPoolCNNGradStep finds in the model, with CNNGradStep's messages
    for kw, match in ((dict(pooled_value=True), "PooledValueHead"), (dict(katago=True), "KataGoCNN")):
        with pytest.raises(ValueError, match=match):
            GPoolCNNGradStep(CT.CNN(5, 5, **kw).to(DEV))
    with pytest.raises(ValueError, match="dropout_seed"):
        GPoolCNNGradStep(GT.GPoolCNN(5, 5, blocks=blocks, dropout=0.1).to(DEV))
    # what grad_cnn_gpool_into refuses: the tensors of such models do not fit its keys
    rs.set_order(np.asarray(case["order"], np.uint64), case["swap"])
    pooled = dict(params, **{"value_head.mlp.0.weight": torch.zeros(8, 192, device=DEV)})
    del pooled["value_head.linear.weight"]
    with pytest.raises(ValueError, match="value_head.linear.weight"):  # a PooledValueHead has no value_head.linear
        rs.grad_cnn_gpool_into(0, n, dims, blocks, pooled, grads, running, 1.0, 0.5, _out(n))
    katago = {k: v for k, v in params.items() if not k.startswith("player_encoder.")}  # a KataGoCNN has a scalar_encoder instead
    with pytest.raises(ValueError, match="player_encoder"):
        rs.grad_cnn_gpool_into(0, n, dims, blocks, katago, grads, running, 1.0, 0.5, _out(n))
    with pytest.raises(ValueError, match="blocks"):
        rs.grad_cnn_gpool_into(0, n, dims, (0,), params, grads, running, 1.0, 0.5, _out(n))
    with pytest.raises(ValueError, match="256"):
        rs.grad_cnn_gpool_into(0, n, dims, (0, 257), params, grads, running, 1.0, 0.5, _out(n))
    with pytest.raises(ValueError, match=r"\[0, 1\)"):  # p = 1: the library's refusal, the wrapper passes it on
        rs.grad_cnn_gpool_into(0, n, dims, blocks, params, grads, running, 1.0, 0.5, _out(n), dropout=(1.0, 1, 0))
    untouched()
    # at the C interface, where the wrapper's checks are not
    p, g, pp, pg, r, pr = _cnn_gpool_structs(dims, blocks, params, grads, running)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(pool_dims, pp_=pp, pg_=pg, dropout=None):
        pd = _lib.ArCnnPoolDims((C.c_uint32 * 8)(*pool_dims))
        return _lib.load().ar_rows_grad_cnn_gpool(rs._handle(), 0, n, C.byref(_lib.ArCnnDims(*dims)), C.byref(pd), C.byref(p), C.byref(pp_),
                                                  C.byref(g), C.byref(pg_), C.byref(r), C.byref(pr), 1.0, 0.5, None,
                                                  C.byref(dropout) if dropout is not None else None, stream)

    assert call((0, 257)) == _lib.AR_E_INVALID and "at most 256" in _lib.last_error()
    untouched()
    holed = _lib.ArCnnPoolTensors.from_buffer_copy(pp)
    holed.b1_pool_conv_w = None
    assert call(blocks, pp_=holed) == _lib.AR_E_INVALID and "null tensor" in _lib.last_error() and "pool_conv_w" in _lib.last_error()
    untouched()
    assert call(blocks, dropout=_lib.ArTrainDropout(1.0, 1, 0)) == _lib.AR_E_INVALID and "[0, 1)" in _lib.last_error()
    assert call(blocks, dropout=_lib.ArTrainDropout(float("nan"), 1, 0)) == _lib.AR_E_INVALID
    assert call(blocks, dropout=_lib.ArTrainDropout(-0.5, 1, 0)) == _lib.AR_E_INVALID
    untouched()
    assert call((1, 0)) == _lib.AR_E_INVALID and "null tensor" in _lib.last_error()  # block 0 called a gpool block: it has no pool tensors
    untouched()
    grads_after, _, out = _run(rs, case)  # and the set still works
    assert np.isfinite(out["losses"]).all() and all(np.isfinite(v).all() for v in grads_after.values())


# ---- 10. two steps of AdamW through grad_iter, with dropout ------------------------------------------------------------------------
def test_two_adamw_steps(sets):
    from alpharat_amd.dataset import RowDataset
    from alpharat_amd.train import GPoolCNNGradStep

    (Ch, PD, HD), blocks = TG.TRAJ_DIMS, TG.TRAJ_BLOCKS
    TG.use_layer_weights(blocks)
    w, h = TG.BOARDS[TG.TRAJ_BOARD][1], TG.BOARDS[TG.TRAJ_BOARD][2]
    sd0 = NG.random_gpool_cnn(w, h, Ch, PD, HD, blocks, TG.TRAJ_SEED)
    rs = sets(TG.TRAJ_BOARD)
    ds = RowDataset(rs)
    model = GT.GPoolCNN(w, h, Ch, PD, HD, blocks, dropout=TG.DROPOUT_P, sd=sd0).to(DEV).train()
    step = GPoolCNNGradStep(model, TG.WEIGHTS["policy_weight"], TG.WEIGHTS["value_weight"], dropout_seed=TG.DROPOUT_SEED)
    opt = torch.optim.AdamW(model.parameters(), lr=TG.TRAJ_LR)
    lib_losses, epoch = [], 0
    while len(lib_losses) < TG.TRAJ_STEPS:
        for n, losses in ds.grad_iter(step, TG.TRAJ_BATCH, epoch=epoch, seed=TG.TRAJ_PLAN_SEED, augment=False):
            opt.step()
            lib_losses.append(losses)
            if len(lib_losses) == TG.TRAJ_STEPS:
                break
        epoch += 1
    lib_losses = [float(l.cpu()[5]) for l in lib_losses]
    lib = {k: v.detach().cpu().numpy() for k, v in model.named_parameters()}
    buffers = dict(model.named_buffers())
    assert [int(buffers[f"{bn}.num_batches_tracked"]) for bn in NG.bn_modules(blocks)] == [TG.TRAJ_STEPS] * len(NG.bn_modules(blocks))
    assert step.dropout_step == TG.TRAJ_STEPS
    epochs, steps = TG.trajectory_plan()
    plans = {e: (o, m) for e, o, m in epochs}

    def reference(dtype):
        p = {k: torch.tensor(np.asarray(sd0[k]), dtype=dtype, requires_grad=True) for k in NG.param_keys(blocks)}
        running = {k: torch.tensor(np.asarray(sd0[k]), dtype=dtype) for k in NG.running_keys(blocks)}
        opt = torch.optim.AdamW(list(p.values()), lr=TG.TRAJ_LR)
        out = []
        for s, (e, first) in enumerate(steps):
            order, mask = plans[e]
            idx = order[first:first + TG.TRAJ_BATCH]
            case = NG.with_masks(TG.make_case(TG.TRAJ_BOARD, sd0, idx, mask[idx]), TG.DROPOUT_SEED, s, TG.DROPOUT_P)
            t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)  # noqa: E731
            opt.zero_grad()
            ls = GT.losses(GT.forward(p, t(case["observation"]), w, h, running, case["masks"], case["scale"]), t(case["policy_p1"]),
                           t(case["policy_p2"]), t(case["value_p1"]), t(case["value_p2"]), TG.WEIGHTS["policy_weight"],
                           TG.WEIGHTS["value_weight"])
            ls["loss"].backward()
            opt.step()
            out.append(float(ls["loss"].detach()))
        return {k: v.detach().numpy() for k, v in p.items()}, out

    p64, loss64 = reference(torch.float64)
    p32, loss32 = reference(torch.float32)
    TG.assert_grads_within(lib, p64, p32, "after two AdamW steps")
    for i in range(TG.TRAJ_STEPS):
        bound = 8.0 * max(abs(loss32[i] - loss64[i]), 2.0 ** -23 * abs(loss64[i]))
        print(f"step {i}: loss {lib_losses[i]!r} f64 {loss64[i]!r} ref32 {loss32[i]!r} bound {bound:.3e}")
        assert abs(lib_losses[i] - loss64[i]) <= bound, i
