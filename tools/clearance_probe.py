"""What the mesh clearance query and the contact monitor cost next to what a host needs today before it can check
anything (a get_state() download) and next to the physics they follow:

    python tools/clearance_probe.py            -> profiles/clearance_probe.json

The parent never opens the GPU: every configuration (ensemble size x search radius) runs in a child of its own under
`timeout -k 10`, and the first one that fails ends the probe.  Per configuration, medians over alternating repetitions
after a warm-up, fp32 engine over bench.py's config-3 orchard (vehicles moved 12 m east, among the trees):
  (a) afe_clearance_query_engine with device outputs      (b) afe_contact_monitor_update
  (c) get_state() of the same ensemble                    (d) ten physics steps, default stepping mode
and the traversal's counters (tree nodes, triangle box tests, fp64 evaluations per point) from the counting build.
"""
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (65536, 1048576)
RADII = (2.0, float("inf"))
REPS = 31
UNBOUNDED_SEARCH = 1.0e3      # a monitor wants a finite search radius: one that covers the whole orchard


def child(n, max_dist):
    import numpy as np
    import torch  # noqa: F401  (first: see INTEGRATION.md section 5)
    sys.path.insert(0, ROOT)
    afa = importlib.import_module("agri-fly_amd")
    sc = afa.scenarios
    rows, cols, altitude = 6, 10, 1.2
    tris = sc.orchard_mesh(rows=rows, cols=cols, seed=0)
    cmap = afa.ClearanceMap(tris)
    rng = np.random.default_rng(0)
    lane = rng.integers(0, rows - 1, n)
    on_row = rng.random(n) < 0.5
    y0 = np.where(on_row, lane * 4.0 + rng.uniform(-0.3, 0.3, n), lane * 4.0 + 2.0 + rng.uniform(-0.8, 0.8, n))
    pos0 = np.stack([np.full(n, 8.0) + rng.uniform(-1, 0, n), y0, np.full(n, altitude)])
    att0 = np.tile(np.array([[1.0], [0.0], [0.0], [0.0]]), (1, n))
    params = afa.params_from_type(5)
    e = afa.Ensemble(n, precision=afa.AFE_F32)
    e.set_type_table([params])
    e.set_imu_noise(True, 0.1, 0.2, afa.AFE_SEED_DECORRELATED)
    e.set_rates_logic([afa.rates_logic_params_from_type(5)])
    e.set_state(pos0, np.zeros((3, n)), att0, np.zeros((3, n)), np.full((4, n), sc.hover_speed(params)))
    e.set_rates_commands(np.full(n, 9.81, np.float32), np.zeros((3, n), np.float32))
    search = max_dist if np.isfinite(max_dist) else UNBOUNDED_SEARCH
    mon = afa.ContactMonitor(e, cmap, 0.116, search)
    bufs = (afa.DeviceBuffer(n * 8), afa.DeviceBuffer(n * 4), afa.DeviceBuffer(n * 24))
    wall = {k: [] for k in "abcd"}
    kernel_ms = []
    for rep in range(REPS + 3):
        t0 = time.perf_counter()
        ms = cmap.query_engine(e, max_dist, out=bufs)
        t1 = time.perf_counter()
        counts = mon.update()
        t2 = time.perf_counter()
        st = e.get_state()
        t3 = time.perf_counter()
        e.step(1000, 10)
        e.sync()
        t4 = time.perf_counter()
        if rep >= 3:                                   # warm-up
            for k, dt in zip("abcd", (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                wall[k].append(dt * 1e3)
            kernel_ms.append(ms)
    m = min(n, 65536)
    stats, _ = cmap.query_stats(st["pos"][:, :m], max_dist)
    d2 = bufs[0].download(np.float64, (n,))
    med = {k: float(np.median(v)) for k, v in wall.items()}
    out = dict(n=n, max_dist=("inf" if not np.isfinite(max_dist) else max_dist), reps=REPS, n_tri=int(len(tris)),
               query_engine_ms=med["a"], query_kernel_ms=float(np.median(kernel_ms)), monitor_update_ms=med["b"],
               get_state_ms=med["c"], ten_steps_ms=med["d"], update_over_get_state=med["b"] / med["c"],
               update_over_ten_steps=med["b"] / med["d"], share_within=float(np.isfinite(d2).mean()),
               in_contact_now=counts[0], ever_in_contact=counts[1],
               per_point=dict(nodes=stats["nodes"] / stats["points"], tri_box_tests=stats["tri_box_tests"] / stats["points"],
                              tri_fp64_evals=stats["tri_fp64_evals"] / stats["points"]))
    mon.close()
    for b in bufs:
        b.close()
    e.close()
    cmap.close()
    print("RESULT " + json.dumps(out))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]), float(sys.argv[3]))
    sys.path.insert(0, ROOT)
    provenance = importlib.import_module("agri-fly_amd.provenance")
    rows = []
    for n in SIZES:
        for r in RADII:
            limit = 120 if n <= 65536 else 240
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", str(n), repr(r)]
            run = subprocess.run(cmd, capture_output=True, text=True)
            line = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
            if run.returncode != 0 or not line:
                print("clearance_probe: n=%d max_dist=%r ended with status %d; stopping here\n%s" % (n, r, run.returncode, run.stderr[-2000:]))
                return 1
            rows.append(json.loads(line[0][7:]))
            print(json.dumps(rows[-1]), flush=True)
    out = dict(kernel_sources=provenance.kernel_source_hashes(("afe_clearance.hip",)), rows=rows,
               done=all(r["monitor_update_ms"] < r["get_state_ms"] for r in rows))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "clearance_probe.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
