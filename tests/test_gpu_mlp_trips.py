"""-m gpu: k_mlp_mfma's chain starts (FL = 2) at the widths and leaf counts where their loop changes path, and the heads
at the same shapes.

The starts are written for memory latency (alpharat_amd/csrc/nets.h mlp_chain_starts): a thread has exactly H / 16 items
and issues the loads of 8, 4 or 2 of them before it stores the first sum, with no bound per item and no division per
item. The heads (heads_mfma16) take K / 4 steps of four columns.

    H     starts (items per thread)        heads (k-steps = H / 4)
    32    2: one pass of 2, the minimum    8
    64    4: one pass of 4                 16
    96    6: a pass of 4 and one of 2      24: not a multiple of 16
    160   10: a pass of 8 and one of 2     40
    256   16: two passes of 8              64 (the workload's width)

Boards are 5x5, the networks tests/_random_nets.py random_mlp. Calls of 1, 63, 64, 65 and 130 leaves: a partial tile,
exact tiles, a tile with one leaf, and the lanes past the count that read leaf 0.

What is compared. tests/_mlp_np.py states the network in float64, so the device's f32 outputs cannot equal it bit for bit;
against it every output is held to the project's tolerance for network outputs (1e-5, as tests/test_gpu_boards.py holds
them against the oracle). Bit for bit (test_gpu_boards.py's _same_bits) are:
- AR_MLP_FL = 0 / 1 against the default 2: those variants run the p1 / p2 rows through the matrix cores and never enter the
  starts loop, so they pin its sums (FL = 0 needs (3 hw + 7) & ~1 <= H + 4 and falls to 1 below H = 96 on 5x5, so at
  H = 32 and 64 the two comparisons are one);
- a leaf evaluated in a call of 1, 63, 64 or 65, taken from the front and from the back of the 130, against the call of
  130: the same leaf at other rows of a tile, next to other leaves, in a partial tile;
- k_mlp_mfma with FEAT (the trunk's output stored as well) against the evaluator without it at H = 96, through
  RowSet.validate_lv and RowSet.validate on the rows of tests/_validate.py's "5x5 open" board (its entry point takes a
  seeded net of any width), at the default first-layer variant and at AR_MLP_FL = 0 and 1."""
import numpy as np
import pytest
import torch  # noqa: F401  before anything loads libalpharat_hip

import _mlp_np
import _ownership_np as ON
import _validate as V
from _random_nets import positions, pyrat, random_mlp

pytestmark = pytest.mark.gpu
KEYS = ("logits_p1", "logits_p2", "policy_p1", "policy_p2", "value_p1", "value_p2")
WIDTHS = (32, 64, 96, 160, 256)
COUNTS = (1, 63, 64, 65, 130)
N = max(COUNTS)


@pytest.fixture(scope="module")
def leaves():
    """(oracle games, device games, flat observations) of the 130 positions, made once"""
    ogs = positions(5, 5, N, seed=5005)
    return ogs, [pyrat(og) for og in ogs], np.stack([og.encode() for og in ogs])


def _same_bits(a, b, what, rows=slice(None)):
    for k in KEYS:
        assert a[k].tobytes() == b[k][rows].tobytes(), (what, k)


@pytest.mark.parametrize("H", WIDTHS)
def test_outputs_at_every_width_and_leaf_count(H, leaves, tmp_path, monkeypatch):
    from alpharat_amd.nets import Net
    from alpharat_amd.weights import write_blob

    _, games, obs = leaves
    t = random_mlp(5, 5, H, seed=1000 + H)
    net = Net(write_blob(tmp_path / f"mlp_h{H}.arnet", "mlp", 5, 5, t))
    monkeypatch.delenv("AR_MLP_FL", raising=False)
    whole = net.evaluate(games)
    want = _mlp_np.mlp_forward(t, obs)
    for k in KEYS:
        err = np.abs(whole[k] - want[k])
        print(f"H={H} {k}: max |device - float64| = {err.max():.3g}")
        np.testing.assert_allclose(whole[k], want[k], atol=1e-5, rtol=1e-5, err_msg=f"H={H} {k}")
    for cnt in COUNTS[:-1]:
        _same_bits(net.evaluate(games[:cnt]), whole, f"H={H}: the first {cnt}", slice(0, cnt))
        _same_bits(net.evaluate(games[N - cnt:]), whole, f"H={H}: the last {cnt}", slice(N - cnt, N))
    for fl in ("0", "1"):
        monkeypatch.setenv("AR_MLP_FL", fl)
        _same_bits(net.evaluate(games), whole, f"H={H}: AR_MLP_FL={fl}")
    net.close()


def test_feat_kernel_gives_the_bits_of_the_evaluator(tmp_path):
    """H = 96 (a starts pass of 4 and one of 2) with an ownership head: validate_lv runs k_mlp_mfma<.., FEAT = true>,
    validate runs the evaluator of the self-play loop"""
    from alpharat_amd.nets import Net
    from alpharat_amd.shards import RowSet
    from alpharat_amd.weights import write_blob

    H = 96
    games, rows = V.board("5x5 open")
    n = len(rows["value_p1"])
    t = random_mlp(5, 5, H, V.SEED)
    net = Net(write_blob(tmp_path / "h96.lv.arnet", "mlp", 5, 5, {**t, **ON.random_ownership(5, 5, H, 17)}))
    assert net.has_ownership
    want = _mlp_np.mlp_forward(t, rows["observation"])
    keys = ("logits_p1", "logits_p2", "value_p1", "value_p2")
    with RowSet(5, 5, n) as rs:
        rs.add_games(games)
        for cnt in COUNTS:
            idx = np.arange(cnt) % n
            sums_lv, _, out_lv = rs.validate_lv(net, idx, return_rows=True)
            sums, out = rs.validate(net, idx, return_rows=True)
            assert sums == sums_lv, cnt
            for k in keys:
                assert out[k].tobytes() == out_lv[k].tobytes(), (cnt, k)
                np.testing.assert_allclose(out_lv[k], want[k][idx], atol=1e-5, rtol=1e-5, err_msg=f"{cnt} rows {k}")
    net.close()


def test_feat_kernel_at_every_first_layer_variant(tmp_path, monkeypatch):
    """k_mlp_mfma<.., FEAT = true> with FL = 0 and FL = 1, which no other test launches: 5x5 and H = 96, so that
    K1e = 82 <= H + 4 and AR_MLP_FL=0 really is variant 0; 65 rows, a full tile and a tile of one. Under either setting
    validate_lv (FEAT) and validate (no FEAT) give the same sums and the same bytes of logits and values, and those are
    the bytes of the default run (FL = 2)."""
    from alpharat_amd.nets import Net
    from alpharat_amd.shards import RowSet
    from alpharat_amd.weights import write_blob

    H, cnt = 96, 65
    games, rows = V.board("5x5 open")
    t = random_mlp(5, 5, H, V.SEED)
    net = Net(write_blob(tmp_path / "h96.lv.arnet", "mlp", 5, 5, {**t, **ON.random_ownership(5, 5, H, 17)}))
    assert net.has_ownership
    idx = np.arange(cnt) % len(rows["value_p1"])
    keys = ("logits_p1", "logits_p2", "value_p1", "value_p2")
    with RowSet(5, 5, len(rows["value_p1"])) as rs:
        rs.add_games(games)
        monkeypatch.delenv("AR_MLP_FL", raising=False)
        sums_ref, _, out_ref = rs.validate_lv(net, idx, return_rows=True)
        for fl in ("0", "1"):
            monkeypatch.setenv("AR_MLP_FL", fl)
            sums_lv, _, out_lv = rs.validate_lv(net, idx, return_rows=True)
            sums, out = rs.validate(net, idx, return_rows=True)
            assert sums == sums_lv == sums_ref, fl
            for k in keys:
                assert out_lv[k].tobytes() == out[k].tobytes(), (fl, k)
                assert out_lv[k].tobytes() == out_ref[k].tobytes(), (fl, k)
    net.close()
