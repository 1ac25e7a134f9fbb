"""CPU: checkpoint_to_blob(keep_ownership=True) keeps LocalValueMLP's ownership head in an mlp blob of its own name; the
default call writes what it always wrote; the flag on another architecture raises."""
import shutil
from pathlib import Path

import numpy as np
import pytest

GOLD = Path(__file__).resolve().parent / "golden"
OWN = ("ownership_head.0.weight", "ownership_head.0.bias", "ownership_head.2.weight", "ownership_head.2.bias")


@pytest.fixture()
def lv_pt(tmp_path):
    return Path(shutil.copy(GOLD / "ckpt_katago" / "local_value_5x5_h32.pt", tmp_path / "lv.pt"))


def test_keep_ownership_writes_the_head_under_an_mlp_header(lv_pt):
    import torch

    from alpharat_amd.weights import checkpoint_to_blob, read_blob

    blob = checkpoint_to_blob(lv_pt, keep_ownership=True)
    assert blob == lv_pt.with_name("lv.lv.arnet") and blob.exists()
    arch, w, h, t = read_blob(blob)
    assert (arch, w, h) == ("mlp", 5, 5)
    sd = torch.load(lv_pt, map_location="cpu", weights_only=True)["model_state_dict"]
    H = sd["trunk.0.weight"].shape[0]
    assert [t[k].shape for k in OWN] == [(H, H), (H,), (100, H), (100,)]
    for k in OWN:
        assert np.array_equal(t[k], sd[k].numpy()), k
    assert "outcome_values" not in t
    plain = checkpoint_to_blob(lv_pt)
    assert plain == lv_pt.with_suffix(".arnet") and plain != blob  # two caches, two names
    _, _, _, tp = read_blob(plain)
    assert set(t) == set(tp) | set(OWN)
    for k in tp:
        assert np.array_equal(t[k], tp[k]), k
    assert checkpoint_to_blob(lv_pt, keep_ownership=True) == blob  # cached


def test_default_output_is_unchanged(lv_pt):
    """the default call's blob is the committed conversion of the same checkpoint, byte for byte"""
    from alpharat_amd.weights import checkpoint_to_blob, read_blob, write_blob

    plain = checkpoint_to_blob(lv_pt)
    arch, w, h, t = read_blob(plain)
    assert arch == "mlp" and not any(k.startswith("ownership_head.") or k == "outcome_values" for k in t)
    # what the function wrote before it knew the flag: the state dict without the head, in state-dict order
    import torch

    sd = torch.load(lv_pt, map_location="cpu", weights_only=True)["model_state_dict"]
    want = {k: v.numpy() for k, v in sd.items() if not k.startswith("ownership_head.") and k != "outcome_values"}
    ref = write_blob(lv_pt.with_name("ref.arnet"), "mlp", 5, 5, want)
    assert plain.read_bytes() == ref.read_bytes()


@pytest.mark.parametrize("pt", ["ckpt/mlp_5x5_h32.pt", "ckpt/symmetric_5x5_h32.pt", "ckpt_katago/katago_7x5_c32.pt"])
def test_flag_on_another_architecture_raises(pt, tmp_path):
    from alpharat_amd.weights import checkpoint_to_blob

    p = Path(shutil.copy(GOLD / pt, tmp_path / "other.pt"))
    with pytest.raises(ValueError, match="keep_ownership"):
        checkpoint_to_blob(p, keep_ownership=True)
    assert not p.with_suffix(".lv.arnet").exists()
    assert checkpoint_to_blob(p).exists()  # the default call still converts it
