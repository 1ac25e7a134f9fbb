"""CPU: the sixteen-lane backup's per-lane logic (alpharat_amd/csrc/dev_backup16.h bk16_walk / bk16_apply: every touched
node read once, given all its entries' updates in batch order, written once) against the entry-by-entry walk of
backup_round, restated in tests/hostsim_backup/backup_sim.cpp. Random trees of depth 1 to 24 (paths past PATH_LDS_STEPS),
batches of 1, 2, 15, 16, 17 and 33 entries with shared prefixes of every length, a terminal leaf claimed twice and an entry
whose leaf is the root; lanes in ascending and in descending order. Bar: every node record equal byte for byte, equal
update counts. The program has its own main and runs once plain and once under AddressSanitizer and UBSan."""
import subprocess
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent / "hostsim_backup"


@pytest.mark.parametrize("program", ["backup_sim", "backup_sim_san"])
def test_merged_backup_equals_the_entry_by_entry_walk(program):
    subprocess.run(["make", "-s", "-C", str(HERE), program], check=True)
    r = subprocess.run([str(HERE / program)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: ") and r.stderr == "", r.stdout + r.stderr
