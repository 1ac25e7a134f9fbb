"""CPU: the sixteen-lane backup's collision cancel (alpharat_amd/csrc/dev_backup16.h: bk16_fold gives a record's count to
the lane whose entry has the record's node as its leaf, bk16_settle subtracts the lane's total from every ancestor while
the node is in registers, bk16_cancel_left walks what no lane took) against the entry-by-entry backup followed by the
plain cancel walk, restated in tests/hostsim_backup/collide_sim.cpp. Random trees of depth 1 to 24, batches of 1, 2, 15,
16, 17 and 33 entries, lists of 0, 1, 16, 17, 40 and 530 records: several on one leaf, leaves in another chunk than the
record's index, a terminal leaf claimed twice, the root as a leaf, records with node NIL or on no leaf, an entry dropped
with error 6; lanes in ascending and in descending order. Bar: every node record equal byte for byte, equal update
counts, every record folded or walked exactly once and folded whenever its node is a noted leaf. The program has its own
main and runs once plain and once under AddressSanitizer and UBSan."""
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent / "hostsim_backup"


@pytest.mark.parametrize("program", ["collide_sim", "collide_sim_san"])
def test_folded_cancel_equals_the_plain_walk(program):
    subprocess.run(["make", "-s", "-f", "collide.mk", "-C", str(HERE), program], check=True)
    r = subprocess.run([str(HERE / program)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: ") and r.stderr == "", r.stdout + r.stderr
