"""Where a k_backup16 wavefront's time goes, and what its collision records look like, from the instrumented build
(hipcc ... -DAR_STATS -o alpharat_amd/libalpharat_hip_stats.so; AR_STATS_LIB names another such build). Bench workload,
steady state. The instrumented build is never the one that is timed.
Usage: python tools/bk16_stats.py [resident] [warm batch steps] [window batch steps]"""
import ctypes as C
import os
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from alpharat_amd import _lib  # noqa: E402

_lib.LIB_PATH = Path(os.environ.get("AR_STATS_LIB") or _lib.PKG / "libalpharat_hip_stats.so")
import bench  # noqa: E402
from alpharat_amd.sampling import UNBOUNDED, SelfPlaySession  # noqa: E402

L = _lib.load()
resident = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
warm = int(sys.argv[2]) if len(sys.argv) > 2 else 3072
window = int(sys.argv[3]) if len(sys.argv) > 3 else 256
blob = bench.make_mlp_blob(Path(tempfile.mkdtemp()) / "bench_mlp_7x7_h256.arnet")
search, sims, batch, _ = bench.WORKLOADS["mlp"]
L.ar_debug_backup16_clk.argtypes = [C.c_void_p]
clk = (C.c_ulonglong * 32)()
with SelfPlaySession(**bench.GAME, num_games=UNBOUNDED, simulations=sims, batch_size=batch, output_dir=None,
                     weights_path=str(blob), seed=0, concurrent_games=resident, **search) as s:
    s.step(warm)
    L.ar_debug_backup16_clk(clk)  # (reading resets the counters)
    st = s.step(window)
    L.ar_debug_backup16_clk(clk)
c = list(clk)
waves, games, recs = max(c[0], 1), max(c[6], 1), max(c[7], 1)
print(f"{_lib.LIB_PATH.name}: {window} batch steps of {resident} games, batch {batch}, step {st.device_secs / max(st.steps, 1) * 1e3:.3f} ms")
print(f"wavefronts {c[0]} ({c[0] / window:.0f} per step), lifetime in backup16() {c[5] / waves / 100:.1f} us each")
total = max(sum(c[1:5]), 1)
for name, v in zip(("entries and sort", "walk", "claim + apply", "collisions"), c[1:5]):
    print(f"  {name:<18} {v / waves / 100:8.2f} us per wavefront  {100.0 * v / total:5.1f} %")
print(f"batches {c[6]} ({c[6] / window:.0f} per step), chunks per batch {c[8] / games:.3f}")
print(f"collision records {c[7]}: {c[7] / games:.2f} per batch; node is the leaf of an entry of a chunk: {100.0 * c[9] / recs:.3f} %; "
      f"node NIL: {c[10]}")
print(f"atomic walk: {c[11]} (record, level) steps = {3 * c[11]} atomics, {3 * c[11] / window / 1e6:.2f} M per step; "
      f"{c[11] / recs:.2f} levels per record; wavefronts that walked {100.0 * c[15] / waves:.1f} %; "
      f"trips in sequence per wavefront {c[12] / waves:.2f}")
print(f"deepest path of a wavefront's chunk: {c[13] / max(c[14], 1):.2f} levels")
