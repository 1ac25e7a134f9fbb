"""-m gpu: k_mlp_mfma_halves, the MLP evaluator's default path with both hidden layers split at column Ha of the hidden
dimension (alpharat_amd/csrc/nets.h), at the shapes the other suites do not reach.

The kernel keeps half a layer's activations in LDS, act[64][Ha + 4] with Ha = 32 ceil(H / 64) and Hb = H - Ha, and gives
every output the sum k_mlp_mfma gives it, in the same order. tests/test_gpu_mlp_trips.py (5x5, H = 32 .. 256) and
tests/test_gpu_boards.py already pass through it wherever net_launch's rule selects it; here are the workload's board
and the widths whose halves load the wavefronts differently:

    H     Ha / Hb     first layer (a 32-column tile of each half per wavefront)      second layer, heads
    256   128 / 128   four wavefronts, a tile in both halves (the workload)         k = 128 + 128
    192    96 / 96    three wavefronts, a tile in both halves; the fourth has none   k = 96 + 96; wavefront 1's two
                                                                                     column tiles fall in different halves
    224   128 / 96    wavefront 3 has a tile in half A only                          k = 128 + 96

What is compared. tests/_mlp_np.py states the network in float64; against it every output is held to the project's
tolerance for network outputs (1e-5). Bit for bit are: AR_MLP_FL = 1 and 0 (whole-tile kernels, k_mlp_mfma: another code
path; 0 falls to 1 where the whole observation does not fit a row of its tile) against the default; and the same leaf in
a call of 130 (or 70), at the front and at the back of a shorter call, and alone."""
import numpy as np
import pytest
import torch  # noqa: F401  before anything loads libalpharat_hip

import _mlp_np
import _ownership_np as ON
import _validate as V
from _random_nets import positions, pyrat, random_mlp

pytestmark = pytest.mark.gpu
KEYS = ("logits_p1", "logits_p2", "policy_p1", "policy_p2", "value_p1", "value_p2")
COUNTS = (1, 63, 64, 65, 130)
N = max(COUNTS)


@pytest.fixture(scope="module")
def leaves_7x7():
    """(device games, flat observations) of 130 positions on the workload's board, made once"""
    ogs = positions(7, 7, N, seed=7007)
    return [pyrat(og) for og in ogs], np.stack([og.encode() for og in ogs])


def _same_bits(a, b, what, rows=slice(None)):
    for k in KEYS:
        assert a[k].tobytes() == b[k][rows].tobytes(), (what, k)


def _check(net, t, games, obs, counts, monkeypatch, what):
    """the call of all `games` against float64 and against AR_MLP_FL = 1 / 0; calls of the first and the last `cnt`
    against their rows of it"""
    n = len(games)
    monkeypatch.delenv("AR_MLP_FL", raising=False)
    whole = net.evaluate(games)
    want = _mlp_np.mlp_forward(t, obs)
    for k in KEYS:
        err = np.abs(whole[k] - want[k])
        print(f"{what} {k}: max |device - float64| = {err.max():.3g}")
        np.testing.assert_allclose(whole[k], want[k], atol=1e-5, rtol=1e-5, err_msg=f"{what} {k}")
    for cnt in counts:
        _same_bits(net.evaluate(games[:cnt]), whole, f"{what}: the first {cnt}", slice(0, cnt))
        _same_bits(net.evaluate(games[n - cnt:]), whole, f"{what}: the last {cnt}", slice(n - cnt, n))
    for fl in ("1", "0"):
        monkeypatch.setenv("AR_MLP_FL", fl)
        _same_bits(net.evaluate(games), whole, f"{what}: AR_MLP_FL={fl}")
    monkeypatch.delenv("AR_MLP_FL", raising=False)


@pytest.mark.parametrize("H", (256, 192, 224))
def test_halves_on_the_workload_board(H, leaves_7x7, tmp_path, monkeypatch):
    """7x7 (K2e = 56 staged floats a leaf), calls of 1, 63, 64, 65 and 130 leaves"""
    from alpharat_amd.nets import Net
    from alpharat_amd.weights import write_blob

    games, obs = leaves_7x7
    t = random_mlp(7, 7, H, seed=2000 + H)
    net = Net(write_blob(tmp_path / f"mlp7_h{H}.arnet", "mlp", 7, 7, t))
    _check(net, t, games, obs, COUNTS[:-1], monkeypatch, f"7x7 H={H}")
    net.close()


@pytest.mark.parametrize("w,h,kernel", [(14, 9, "halves"), (16, 8, "whole-tile")], ids=["14x9-halves", "16x8-whole-tile"])
def test_both_sides_of_the_host_rule(w, h, kernel, tmp_path, monkeypatch):
    """net_launch sends a network to k_mlp_mfma_halves when its first-layer variant would be 2, the staged operand fits a
    row of the half tile, K2e = (hw + 7) & ~1 <= Ha + 4, and three workgroups fit a CU's LDS,
    3 (64 (Ha + 4) 4 + 7,424) <= 160 KiB. At H = 256 (Ha = 128) the LDS term always holds, so the boundary is K2e <= 132:
    14x9 (126 cells, K2e = 132) is the largest board that takes the halved kernel and 16x8 (128 cells, K2e = 134) takes
    the whole-tile FL = 2 kernel. Both are four-word boards (NW = 4). 70 leaves: a full tile and a partial one."""
    from alpharat_amd.nets import Net
    from alpharat_amd.weights import write_blob

    H = 256
    ogs = positions(w, h, 70, seed=w * 1000 + h + 7)
    games, obs = [pyrat(og) for og in ogs], np.stack([og.encode() for og in ogs])
    t = random_mlp(w, h, H, seed=w * 100 + h + H + 7)
    net = Net(write_blob(tmp_path / f"mlp_{w}x{h}.arnet", "mlp", w, h, t))
    _check(net, t, games, obs, (1, 6, 64), monkeypatch, f"{w}x{h} H={H} ({kernel})")
    net.close()


def test_feat_kernel_gives_the_bits_of_the_halved_evaluator(tmp_path):
    """H = 256 with an ownership head on 5x5, 65 rows: validate_lv runs k_mlp_mfma with FEAT (a whole tile in
    LDS), validate runs k_mlp_mfma_halves"""
    from alpharat_amd.nets import Net
    from alpharat_amd.shards import RowSet
    from alpharat_amd.weights import write_blob

    H, cnt = 256, 65
    games, rows = V.board("5x5 open")
    n = len(rows["value_p1"])
    t = random_mlp(5, 5, H, V.SEED)
    net = Net(write_blob(tmp_path / "h256.lv.arnet", "mlp", 5, 5, {**t, **ON.random_ownership(5, 5, H, 17)}))
    assert net.has_ownership
    want = _mlp_np.mlp_forward(t, rows["observation"])
    with RowSet(5, 5, n) as rs:
        rs.add_games(games)
        idx = np.arange(cnt) % n
        sums_lv, _, out_lv = rs.validate_lv(net, idx, return_rows=True)
        sums, out = rs.validate(net, idx, return_rows=True)
        assert sums == sums_lv
        for k in ("logits_p1", "logits_p2", "value_p1", "value_p2"):
            assert out[k].tobytes() == out_lv[k].tobytes(), k
            np.testing.assert_allclose(out[k], want[k][idx], atol=1e-5, rtol=1e-5, err_msg=k)
    net.close()
