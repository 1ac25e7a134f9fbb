"""Dropout in the three training steps on the device: ar_rows_grad_mlp_dropout, ar_rows_grad_symmetric_dropout,
ar_rows_grad_local_value_dropout and ar_train_dropout_mask (alpharat_amd/csrc/dev_dropout.h and the DROP forms of the column
kernels in train_mlp.h and train_sym.h), RowSet.grad_*_into(dropout=...), the step classes' ``dropout_seed`` and
``train.dropout_mask``; against the reference's own models with the masks hooked onto their ``nn.Dropout`` modules
(tests/golden/train_dropout) and the float64 restatement with masks (tests/_train_dropout_np.py).

No tolerance is new. The gradients are held under tests/_train.py ``grad_bounds`` -- eight times the reference's own float32
error against float64 (the golden's f32 arrays; tests/_train_dropout_torch.py with autograd in float32 on the device
elsewhere), with the floor for the tensors whose true gradient is zero -- and the forward, the losses and the running
statistics under each architecture's own ``_check_forward``: tests/test_gpu_train.py's fixed ones for PyRatMLP,
``assert_values_within`` for the other two. Every fixture passes the ReLU guard with its masks applied
(tests/test_train_dropout_np.py). Error and bound of every array are printed.

Measured on an MI355X, the largest err / bound over this file: 0.25 for a gradient (value_head.bias, PyRatMLP through
grad_iter), 0.22 for an output (value_p2, the n = 33 SymmetricMLP golden), 0.22 for a loss and 0.21 for a running statistic
(both SymmetricMLP at 5x5)."""
import numpy as np
import pytest
import torch  # before anything loads libalpharat_hip: a process brings up one HIP runtime, and torch ships its own

import _dropout_np as D
import _train_dropout as TD
import _train_dropout_np as ND
import _train_dropout_torch as DT

pytestmark = pytest.mark.gpu

DEV = "cuda"
METHOD = dict(mlp="grad_mlp_into", symmetric="grad_symmetric_into", local_value="grad_local_value_into")


@pytest.fixture(scope="module")
def sets():
    """one uploaded row set per board, made when first asked for; row i of the board's stacked rows is stored position i"""
    from alpharat_amd.shards import RowSet

    made = {}

    def get(board):
        if board not in made:
            games, plain = TD.TR.board(board)
            rs = RowSet(TD.TR.BOARDS[board][1], TD.TR.BOARDS[board][2], len(plain["value_p1"]))
            rs.add_games(games)
            assert rs.count()[1] == len(plain["value_p1"])
            made[board] = rs
        return made[board]

    yield get
    for rs in made.values():
        rs.close()


def _device_tensors(arch, sd):
    K = TD.KEYS[arch]
    params = {k: torch.tensor(np.asarray(sd[k], np.float32), device=DEV) for k in K.PARAM_KEYS}
    running = {k: torch.tensor(np.asarray(sd[k], np.float32), device=DEV) for k in K.RUNNING_KEYS}
    grads = {k: torch.full_like(v, float("nan")) for k, v in params.items()}
    return params, grads, running


def _out(arch, n, case):
    out = dict(losses=torch.full((7 if arch == "local_value" else 6,), float("nan"), device=DEV),
               logits_p1=torch.empty((n, 5), device=DEV), logits_p2=torch.empty((n, 5), device=DEV),
               value_p1=torch.empty(n, device=DEV), value_p2=torch.empty(n, device=DEV))
    if arch == "local_value":
        out["ownership_logits"] = torch.full((n, case["height"], case["width"], 4), float("nan"), device=DEV)
    return out


def _numpy(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _dropout_of(case):
    return (case["p"], case["dropout_seed"], case["dropout_step"])


def _launch(arch, rs, case, first, n, tensors, out, dropout):
    params, grads, running = tensors
    H = case["sd"]["trunk.4.weight"].shape[0]
    weights = (case["policy_weight"], case["value_weight"]) + ((case["ownership_weight"],) if arch == "local_value" else ())
    more = {} if dropout is None else dict(dropout=dropout)
    getattr(rs, METHOD[arch])(first, n, H, params, grads, running, *weights, out, **more)


def _run(arch, rs, case, dropout="case", first=0, n=None, set_order=True):
    """the step over rows first .. first + n of the case's order: numpy grads (NaN-filled before), running, out"""
    if set_order:
        rs.set_order(np.asarray(case["order"], np.uint64), case["swap"])
    n = len(case["order"]) - first if n is None else n
    tensors = _device_tensors(arch, case["sd"])
    out = _out(arch, n, case)
    _launch(arch, rs, case, first, n, tensors, out, _dropout_of(case) if dropout == "case" else dropout)
    return _numpy(tensors[1]), _numpy(tensors[2]), _numpy(out)


def _check_forward(arch, out, running, want, ref32, what):
    K = TD.KEYS[arch]
    if arch == "mlp":  # tests/test_gpu_train.py _check_forward
        for k in K.OUT_KEYS:
            np.testing.assert_allclose(out[k], want[k], rtol=1e-5, atol=1e-5, err_msg=f"{what} {k}")
        losses = np.array([float(want["losses"][k]) for k in K.LOSS_KEYS])
        print(what, "losses", out["losses"], "err", np.abs(out["losses"] - losses).max())
        np.testing.assert_allclose(out["losses"], losses, rtol=1e-6, atol=1e-6, err_msg=f"{what} losses")
        for k in K.RUNNING_KEYS:
            np.testing.assert_allclose(running[k], want["running"][k], rtol=1e-6, atol=1e-6, err_msg=f"{what} {k}")
        return
    fx = TD.FIXTURES[arch]  # tests/test_gpu_train_sym.py and tests/test_gpu_train_lv.py _check_forward
    fx.assert_values_within(out, want, ref32, K.OUT_KEYS, what)
    fx.assert_values_within(dict(zip(K.LOSS_KEYS, out["losses"])), want["losses"], ref32["losses"], K.LOSS_KEYS, what)
    fx.assert_values_within(running, want["running"], ref32["running"], K.RUNNING_KEYS, what)


def _check_case(arch, rs, case, what, **kw):
    """a step against the float64 restatement with masks, the float32 autograd restatement on the device the reference error"""
    want = ND.STEPS[arch](case)
    ref32 = DT.step(arch, case, torch.float32, DEV)
    grads, running, out = _run(arch, rs, case, **kw)
    _check_forward(arch, out, running, want, ref32, what)
    TD.TR.assert_grads_within(grads, want["grads"], ref32["grads"], what)
    return grads, running, out


# ---- 4. the mask ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 32), (33, 32), (300, 256)], ids=["2x32", "33x32", "300x256"])
def test_mask_equals_numpy_bit_for_bit(shape):
    from alpharat_amd.train import dropout_mask

    n, H = shape
    for seed, step, call in ((0, 0, 0), (1, 1, 1), (2 ** 63 + 5, 2 ** 32 + 1, 6), (1, 0, 2), (0, 1, 3), (7, 2 ** 32 + 1, 4),
                             (2 ** 63 + 5, 1, 5)):
        for p in (0.1, 0.5):
            got = dropout_mask(seed, step, call, n, H, p)
            assert got.dtype == torch.bool and tuple(got.shape) == (n, H)
            assert got.cpu().numpy().tobytes() == D.mask(seed, step, call, n, H, p).tobytes(), (seed, step, call, p)
    assert bool(dropout_mask(3, 4, 5, n, H, 0.0).all())


# ---- 5. the reference's own step, its Dropout modules hooked ------------------------------------------------------------------------
@pytest.mark.parametrize("name", TD.GOLDEN)
def test_goldens(sets, name):
    case = TD.golden_case(name)
    arch = case["arch"]
    grads, running, out = _run(arch, sets(case["board"]), case)
    _check_forward(arch, out, running, case["f64"], case["f32"], name)
    TD.TR.assert_grads_within(grads, case["f64"]["grads"], case["f32"]["grads"], name)


# ---- 6. shapes: a batch of two, tails of rows, several row blocks and batch partitions, the full width ---------------------------
@pytest.mark.parametrize("shape", TD.SHAPES, ids=TD.SHAPE_IDS)
def test_shapes(sets, shape):
    arch, index, seed = shape
    case = TD.shape_case(arch, index, seed)
    _check_case(arch, sets(case["board"]), case, TD.SHAPE_IDS[TD.SHAPES.index(shape)])


# ---- 7. exact zeros and exact equalities ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", TD.ARCHS)
def test_dropped_elements_are_exactly_zero(sets, arch):
    """the first policy head as a window onto the trunk output: with one-hot rows and no bias, logit k of player i is element
    (row, column_k) of the activation behind the last dropout, bit for bit. Five columns a step show the whole array: 0
    wherever the mask drops, positive wherever it keeps and the ReLU passes (the guard: no pre-ReLU value within 1e-4 of 0).
    Only the last site is read back: BatchNorm call 1, or calls 5 and 6 of SymmetricMLP. The earlier sites (call 0; calls
    0 .. 4) have no such window; a wrong mask there moves the outputs and gradients that the goldens and shapes bound."""
    case = TD.shape_case(arch, 1, TD.SHAPE_DROPOUT_SEED[arch][1])
    rs = sets(case["board"])
    n, H = len(case["order"]), case["sd"]["trunk.4.weight"].shape[0]
    head = "policy_head" if arch == "symmetric" else "policy_p1_head"
    seen = [np.full((n, H), np.nan, np.float32) for _ in range(2)]
    for c0 in range(0, H, 5):
        cols = [min(c0 + k, H - 1) for k in range(5)]
        sd = dict(case["sd"])
        w = np.zeros_like(sd[f"{head}.weight"])
        w[np.arange(5), cols] = 1.0
        sd[f"{head}.weight"], sd[f"{head}.bias"] = w, np.zeros_like(sd[f"{head}.bias"])
        _, _, out = _run(arch, rs, dict(case, sd=sd), set_order=c0 == 0)
        seen[0][:, cols] = out["logits_p1"]
        if arch == "symmetric":
            seen[1][:, cols] = out["logits_p2"]
    res = ND.STEPS[arch](case)
    last = [(res["bn_out"][5], case["masks"][5]), (res["bn_out"][6], case["masks"][6])] if arch == "symmetric" else [(res["y2"], case["masks"][1])]
    for got, (y, m) in zip(seen, last):
        assert not np.isnan(got).any() and (~m).any() and (m & (y > 0)).any()
        assert (got[~m] == 0).all()
        assert (got[m & (y < 0)] == 0).all()
        assert (got[m & (y > 0)] > 0).all()
        np.testing.assert_allclose(got, np.maximum(y, 0.0) * m * case["scale"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("arch", TD.ARCHS)
def test_p_zero_is_the_step_without_dropout_byte_for_byte(sets, arch):
    case = TD.shape_case(arch, 2, 0)
    rs = sets(case["board"])
    a = _run(arch, rs, case, dropout=None)
    b = _run(arch, rs, case, dropout=(0.0, 5, 3), set_order=False)
    for x, y in zip(a, b):
        for k in x:
            assert not np.isnan(x[k]).any() and x[k].tobytes() == y[k].tobytes(), k


def _model(arch, case, dropout):
    import _lv_torch as LT
    import _mlp_torch as MT
    import _sym_torch as ST

    w, h, H = case["width"], case["height"], case["sd"]["trunk.4.weight"].shape[0]
    if arch == "mlp":
        return MT.MLP(case["observation"].shape[1], H, dropout, sd=case["sd"]).to(DEV)
    if arch == "symmetric":
        return ST.Symmetric(w, h, H, dropout, sd=case["sd"]).to(DEV)
    return LT.LocalValue(w, h, H, dropout, sd=case["sd"]).to(DEV)


def _step_of(arch, model, case, **kw):
    from alpharat_amd.train import LocalValueGradStep, MLPGradStep, SymmetricGradStep

    weights = (case["policy_weight"], case["value_weight"]) + ((case["ownership_weight"],) if arch == "local_value" else ())
    return dict(mlp=MLPGradStep, symmetric=SymmetricGradStep, local_value=LocalValueGradStep)[arch](model, *weights, **kw)


def _step_bytes(step, model, rs, n):
    out = step.step(rs, 0, n, outputs=True)
    torch.cuda.synchronize()
    return ([t.cpu().numpy().tobytes() for t in out] + [step.grads[k].cpu().numpy().tobytes() for k in step.grads]
            + [v.cpu().numpy().tobytes() for _, v in sorted(model.named_buffers())])


@pytest.mark.parametrize("arch", TD.ARCHS)
def test_step_classes_p_zero_and_eval_mode(sets, arch):
    """a seed with p = 0 is a step without a seed; so is eval mode at p = 0.1, where the counter stays as well"""
    case = TD.shape_case(arch, 1, 0)
    rs = sets(case["board"])
    rs.set_order(np.asarray(case["order"], np.uint64), case["swap"])
    n = len(case["order"])
    plain_model = _model(arch, case, 0.0).train()
    want = _step_bytes(_step_of(arch, plain_model, case), plain_model, rs, n)
    seeded_model = _model(arch, case, 0.0).train()
    seeded = _step_of(arch, seeded_model, case, dropout_seed=9)
    assert _step_bytes(seeded, seeded_model, rs, n) == want and seeded.dropout_step == 1
    plain_eval = _model(arch, case, 0.0).eval()
    want_eval = _step_bytes(_step_of(arch, plain_eval, case), plain_eval, rs, n)
    drop_eval = _model(arch, case, 0.1).eval()
    step = _step_of(arch, drop_eval, case, dropout_seed=9)
    assert _step_bytes(step, drop_eval, rs, n) == want_eval and step.dropout_step == 0
    drop_eval.train()  # and in training mode the same object does drop
    assert _step_bytes(step, drop_eval, rs, n) != want and step.dropout_step == 1


# ---- 8. determinism ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", TD.ARCHS)
def test_same_seed_and_step_same_bytes(sets, arch):
    index = TD.SHAPE_INDEX[arch][3]  # several row blocks, several batch partitions
    case = TD.shape_case(arch, index, TD.SHAPE_DROPOUT_SEED[arch][3])
    rs = sets(case["board"])
    a = _run(arch, rs, case)
    b = _run(arch, rs, case, set_order=False)
    for x, y in zip(a, b):
        for k in x:
            assert not np.isnan(x[k]).any() and x[k].tobytes() == y[k].tobytes(), k
    nxt, _, _ = _run(arch, rs, case, dropout=(case["p"], case["dropout_seed"], case["dropout_step"] + 1), set_order=False)
    assert all(not np.array_equal(nxt[k], a[0][k]) for k in ("trunk.0.weight", "trunk.4.weight", "trunk.5.weight"))


@pytest.mark.parametrize("arch", TD.ARCHS)
def test_grad_iter_counts_the_steps(sets, arch):
    """two batches of one order through grad_iter: the first under step 0's masks, the second under step 1's"""
    from alpharat_amd.dataset import RowDataset

    cases = TD.iter_cases(arch)
    rs = sets(TD.ITER_BOARD)
    model = _model(arch, cases[0], TD.P).train()
    step = _step_of(arch, model, cases[0], dropout_seed=TD.ITER_DROPOUT_SEED[arch])
    got = []
    for n, losses in RowDataset(rs).grad_iter(step, TD.ITER_BATCH, epoch=0, seed=TD.ITER_PLAN_SEED):
        got.append((losses.cpu().numpy(), {k: step.grads[k].cpu().numpy().copy() for k in step.grads}))
    assert len(got) == 2 and step.dropout_step == 2
    K = TD.KEYS[arch]
    for i, (case, (losses, grads)) in enumerate(zip(cases, got)):
        # the running statistics moved with step 0; the batch's own statistics are what a training-mode step uses
        masked = ND.with_masks(case, TD.ITER_DROPOUT_SEED[arch], i, TD.P, TD.N_CALLS[arch])
        want = ND.STEPS[arch](masked)
        ref32 = DT.step(arch, masked, torch.float32, DEV)
        TD.TR.assert_grads_within(grads, want["grads"], ref32["grads"], f"{arch} step {i}")
        wl = np.array([float(want["losses"][k]) for k in K.LOSS_KEYS])
        rl = np.array([float(ref32["losses"][k]) for k in K.LOSS_KEYS])
        bound = 8.0 * np.maximum(np.abs(rl - wl), 2.0 ** -23 * np.abs(wl))
        print(arch, "step", i, "losses err", np.abs(losses - wl), "bound", bound)
        assert (np.abs(losses - wl) <= bound).all(), i
        other = ND.STEPS[arch](ND.with_masks(case, TD.ITER_DROPOUT_SEED[arch], 1 - i, TD.P, TD.N_CALLS[arch]))
        assert abs(float(other["losses"]["loss"]) - wl[5]) > 100 * bound[5], i  # the other step's masks would show


# ---- 9. refusals: an exception, and nothing written ----------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", TD.ARCHS)
def test_refusals(sets, arch):
    from alpharat_amd.train import dropout_mask

    case = TD.shape_case(arch, 1, 0)
    rs = sets(case["board"])
    rs.set_order(np.asarray(case["order"], np.uint64), case["swap"])
    n = len(case["order"])
    for p in (1.0, -0.1, float("nan"), 1.5):
        tensors = _device_tensors(arch, case["sd"])
        out = _out(arch, n, case)
        with pytest.raises(ValueError, match="dropout"):
            _launch(arch, rs, case, 0, n, tensors, out, (p, 1, 0))
        torch.cuda.synchronize()
        for k, t in tensors[1].items():
            assert torch.isnan(t).all(), (p, k)
        assert torch.isnan(out["losses"]).all(), p
    for kw in (dict(p=1.0), dict(p=-0.1), dict(p=float("nan")), dict(n=0), dict(n=65537), dict(H=40), dict(H=288)):
        a = dict(dict(n=4, H=32, p=0.1), **kw)
        with pytest.raises(ValueError):
            dropout_mask(1, 0, 0, a["n"], a["H"], a["p"])
    grads, _, out = _run(arch, rs, case, set_order=False)  # and the set still works
    assert np.isfinite(out["losses"]).all() and all(np.isfinite(v).all() for v in grads.values())
