#!/usr/bin/env python3
"""Generate the player-swap fixtures under tests/golden/augment/ by running the reference's own
`swap_player_perspective_batch` (build container only -- /root/reference does not travel to the GPU box; the files are
committed).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_augment_golden.py

Each file holds the eight arrays of some games' rows (`in_*`, from tests/_rows_np.py stack_rows, value_* and action_* as
(n, 1) as the reference's trainer holds them), a mask, and what the reference makes of them (`out_*`), with `width` and
`height`. The reference's function is decorated with torch.compile; TORCHDYNAMO_DISABLE=1 runs it eagerly, on the CPU.
The import shims are those of tools/gen_net_golden.py.
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

os.environ["TORCHDYNAMO_DISABLE"] = "1"
sys.dont_write_bytecode = True
ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference")
OUT = ROOT / "tests" / "golden" / "augment"
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main() -> None:
    import numpy as np
    import torch

    from tools.gen_net_golden import _install_shims

    _install_shims()
    sys.path.insert(0, str(REF))
    from alpharat.nn.augmentation import swap_player_perspective_batch

    import _batches as B
    import _rows_np as R

    open_game, mud_game, capture_game = B.open_game(), B.mud_game(), B.capture_game()
    assert open_game["p1_score"][0] == open_game["p2_score"][0] == 0
    assert (np.asarray(mud_game["p1_mud"]) != np.asarray(mud_game["p2_mud"])).any() and (mud_game["maze"] >= 2).any()
    cases = {"open_5x5": [open_game], "mud_7x5": [mud_game], "capture_5x5": [capture_game]}
    OUT.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(2024)
    for name, games in cases.items():
        w, h = games[0]["width"], games[0]["height"]
        rows = R.stack_rows(games)
        n = len(rows["value_p1"])
        for k in ("value_p1", "value_p2", "action_p1", "action_p2"):
            rows[k] = rows[k].reshape(n, 1)
        mask = rng.random(n) < 0.5
        mask[0] = True   # the first position (score difference 0) is swapped
        mask[1] = False  # and some row is not
        if name == "capture_5x5":
            mask[:] = [True, True, False, True]
            assert set(np.unique(rows["cheese_outcomes"][mask])) == {-1, 0, 1, 2, 3}
        batch = {k: torch.from_numpy(rows[k].copy()) for k in R.KEYS}
        got = swap_player_perspective_batch(batch, torch.from_numpy(mask), w, h)
        out = {k: got[k].numpy() for k in R.KEYS}
        for k in R.KEYS:
            assert out[k].dtype == rows[k].dtype and out[k].shape == rows[k].shape, k
        np.savez_compressed(OUT / f"{name}.npz", width=np.int32(w), height=np.int32(h), mask=mask,
                            **{f"in_{k}": rows[k] for k in R.KEYS}, **{f"out_{k}": out[k] for k in R.KEYS})
        print(name, n, "rows,", int(mask.sum()), "swapped,", (OUT / f"{name}.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
