"""What alpharat_amd/dataset.py and RowSet.build_into decide on the host, without a device: the plan of an epoch, the
windows of its batches, the membership of a split, and the refusals of output tensors."""
import numpy as np
import pytest

import _rows_np as R


def test_epoch_plan_is_a_permutation_and_a_function_of_seed_and_epoch():
    from alpharat_amd.dataset import epoch_plan

    n = 1000
    order, mask = epoch_plan(n, 7, 0)
    assert order.dtype == np.int64 and mask.dtype == bool and order.shape == mask.shape == (n,)
    assert np.array_equal(np.sort(order), np.arange(n)) and not np.array_equal(order, np.arange(n))
    assert 400 < mask.sum() < 600
    again = epoch_plan(n, 7, 0)
    assert np.array_equal(again[0], order) and np.array_equal(again[1], mask)
    for other in (epoch_plan(n, 7, 1), epoch_plan(n, 8, 0)):
        assert not np.array_equal(other[0], order) and not np.array_equal(other[1], mask)
    # the draws, in their order: the mask first, the permutation second
    rng = np.random.default_rng([7, 0])
    assert np.array_equal(mask, rng.random(n) < 0.5) and np.array_equal(order, rng.permutation(n))


def test_epoch_plan_switches():
    from alpharat_amd.dataset import epoch_plan

    n = 257
    assert not epoch_plan(n, 1, 2, p_swap=0.0)[1].any() and epoch_plan(n, 1, 2, p_swap=1.0)[1].all()
    order, mask = epoch_plan(n, 1, 2, shuffle=False, augment=False)
    assert np.array_equal(order, np.arange(n)) and not mask.any()
    assert np.array_equal(epoch_plan(n, 1, 2, shuffle=False)[1], np.random.default_rng([1, 2]).random(n) < 0.5)
    # without augmentation no mask is drawn: the permutation is the stream's first draw
    assert np.array_equal(epoch_plan(n, 1, 2, augment=False)[0], np.random.default_rng([1, 2]).permutation(n))
    assert epoch_plan(0, 0, 0)[0].shape == (0,)


def test_batch_windows_and_drop_last():
    from alpharat_amd.dataset import batch_windows

    assert batch_windows(10, 4) == [(0, 4), (4, 4)]
    assert batch_windows(10, 4, drop_last=False) == [(0, 4), (4, 4), (8, 2)]
    assert batch_windows(8, 4) == batch_windows(8, 4, drop_last=False) == [(0, 4), (4, 4)]
    assert batch_windows(3, 4) == [] and batch_windows(3, 4, drop_last=False) == [(0, 3)]
    assert batch_windows(0, 4, drop_last=False) == []
    with pytest.raises(ValueError, match="batch_size"):
        batch_windows(10, 0)


@pytest.mark.parametrize("seed", [0, 42, None])
def test_split_membership_is_the_shard_writers(seed):
    from alpharat_amd.dataset import split_games

    lengths = [5, 1, 9, 3, 3, 7, 2, 8, 4, 6, 1]
    # an attached set lists its games as they finished; the split goes by game index
    stored_index = np.random.default_rng(1).permutation(len(lengths)).astype(np.uint32)
    if seed is None:
        train, val = split_games(stored_index, 0.3, None)
        assert len(val) == 3 and sorted(np.concatenate([train, val])) == list(range(len(lengths)))
        return
    want_train, want_val, _, _ = R.split_and_shuffle(lengths, 0.3, seed)
    train, val = split_games(stored_index, 0.3, seed)
    assert list(stored_index[train]) == list(want_train) and list(stored_index[val]) == list(want_val)
    assert len(val) == 3
    # games without an index (bundles read back) keep their stored order
    train, val = split_games(np.zeros(len(lengths), np.uint32), 0.3, seed)
    assert list(train) == list(want_train) and list(val) == list(want_val)
    with pytest.raises(ValueError, match="val_ratio"):
        split_games(stored_index, 1.0, seed)


def _tensors(n, w, h, **over):
    import torch

    from alpharat_amd.shards import KEYS, row_shapes

    shapes = row_shapes(w, h)
    out = {k: torch.zeros((n,) + shapes[k], dtype=torch.int8 if k in ("action_p1", "action_p2", "cheese_outcomes")
                          else torch.float32) for k in KEYS}
    out.update(over)
    return out


def test_build_into_refuses_tensors_before_the_library_is_touched():
    import torch

    from alpharat_amd import _lib
    from alpharat_amd.shards import RowSet, check_out_tensors

    loaded = _lib._lib
    rs = RowSet.__new__(RowSet)  # no handle: whatever got past the checks would raise RuntimeError("row set is closed")
    rs.width, rs.height, rs.device_index, rs._h, rs._session = 7, 5, 0, None, None
    n, w, h = 6, 7, 5
    with pytest.raises(ValueError, match="observation is on cpu"):               # a CPU tensor
        rs.build_into(0, n, _tensors(n, w, h))
    with pytest.raises(ValueError, match="policy_p2 has dtype torch.float64"):   # a wrong dtype
        rs.build_into(0, n, _tensors(n, w, h, policy_p2=torch.zeros((n, 5), dtype=torch.float64)))
    with pytest.raises(ValueError, match="action_p1 has dtype torch.uint8"):
        rs.build_into(0, n, _tensors(n, w, h, action_p1=torch.zeros(n, dtype=torch.uint8)))
    with pytest.raises(ValueError, match="observation is not contiguous"):      # a view with a stride
        rs.build_into(0, n, _tensors(n, w, h, observation=torch.zeros((n, 2 * (w * h * 7 + 6)))[:, ::2]))
    with pytest.raises(ValueError, match="value_p1 has 5 rows, 6 are asked for"):  # too few rows
        rs.build_into(0, n, _tensors(n, w, h, value_p1=torch.zeros(n - 1)))
    with pytest.raises(ValueError, match="cheese_outcomes has shape"):           # (w, h) is not (h, w)
        rs.build_into(0, n, _tensors(n, w, h, cheese_outcomes=torch.zeros((n, w, h), dtype=torch.int8)))
    with pytest.raises(ValueError, match="no 'action_p2'"):
        rs.build_into(0, n, {k: v for k, v in _tensors(n, w, h).items() if k != "action_p2"})
    with pytest.raises(ValueError, match="negative"):
        rs.build_into(-1, n, _tensors(n, w, h))
    # what passes: more rows than asked for, values and actions as (rows, 1)
    ok = _tensors(n + 2, w, h, value_p2=torch.zeros((n + 2, 1)), action_p2=torch.zeros((n + 2, 1), dtype=torch.int8))
    check_out_tensors(ok, n, w, h, torch.device("cpu"))
    assert _lib._lib is loaded  # nothing above loaded the library
