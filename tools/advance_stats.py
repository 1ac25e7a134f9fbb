"""Wall clock of the tree-reuse compaction's phases (dev_advance.h, g_adv_clk) from the instrumented build
(hipcc ... -DAR_STATS -o alpharat_amd/libalpharat_hip_stats.so). Bench workload, steady state.
Usage: python tools/advance_stats.py [resident] [warm batch steps] [window batch steps]"""
import ctypes as C
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from alpharat_amd import _lib  # noqa: E402

_lib.LIB_PATH = _lib.PKG / "libalpharat_hip_stats.so"
import bench  # noqa: E402
from alpharat_amd.sampling import UNBOUNDED, SelfPlaySession  # noqa: E402

L = _lib.load()
resident = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
warm = int(sys.argv[2]) if len(sys.argv) > 2 else 3072
window = int(sys.argv[3]) if len(sys.argv) > 3 else 256
blob = bench.make_mlp_blob(Path(tempfile.mkdtemp()) / "bench_mlp_7x7_h256.arnet")
search, sims, batch, _ = bench.WORKLOADS["mlp"]
L.ar_debug_advance_clk.argtypes = [C.c_void_p]
clk = (C.c_ulonglong * 32)()
with SelfPlaySession(**bench.GAME, num_games=UNBOUNDED, simulations=sims, batch_size=batch, output_dir=None,
                     weights_path=str(blob), seed=0, concurrent_games=resident, **search) as s:
    s.step(warm)
    L.ar_debug_advance_clk(clk)  # (reading resets the counters)
    st = s.step(window)
    L.ar_debug_advance_clk(clk)
c = list(clk)
print(f"{window} batch steps, step {st.device_secs / max(st.steps, 1) * 1e3:.3f} ms")
for name, o in (("all trees", 0), ("trees that took more than 300 us", 16)):
    n = max(c[o], 1)
    print(f"{name}: {c[o]} ({c[o] / window:.0f} per launch), slow path {c[o + 6]}; mean hi - keep_root {c[o + 4] / n:.0f}, kept {c[o + 5] / n:.0f}; "
          f"mark {c[o + 1] / n / 100:.1f} us, pick {c[o + 2] / n / 100:.1f} us, move {c[o + 3] / n / 100:.1f} us")
print("trees by total time, 100 us a bucket (last: 700+):", c[8:16])
