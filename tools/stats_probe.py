"""What one afe_stats_update costs next to what a host needs today to learn what an ensemble did (a get_state() download and
numpy on it) and next to the physics between two 100 Hz samples:

    python tools/stats_probe.py            -> profiles/stats_probe.json

The parent never opens the GPU: every ensemble size runs in a child of its own under `timeout -k 10`, and the first one that
fails ends the probe.  fp32 engine, bench.py's config 4 (4 m lattice, gust process, rates logic), 8 equal groups and a 16-edge
histogram.  Per size, medians of the wall time of the call over 31 alternating repetitions after a warm-up:
  (a) afe_stats_update (records + histogram on the host)      (b) get_state() alone
  (c) get_state() + the numpy arithmetic of bench.py's disturbance_sweep bins      (d) ten physics steps
and the bytes per second (a) achieves on the 188 B per vehicle-update the kernel's accesses add up to (52 B state, 16 B
anchors, 24 B reference, 96 B latches read and written: derived, not measured).
"""
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (65536, 1048576)
REPS = 31
N_GROUPS = 8
HIST_EDGES_M = [0.001 * 2.0 ** k for k in range(16)]     # 1 mm .. 32.8 m
BYTES_PER_VEHICLE = 52 + 16 + 24 + 96


def child(n):
    import numpy as np
    import torch  # noqa: F401  (first: see INTEGRATION.md section 5)
    sys.path.insert(0, ROOT)
    afa = importlib.import_module("agri-fly_amd")
    p = afa.params_from_type(5)
    d = afa.scenarios.hover_ensemble(n, p)
    idx = np.arange(n)
    d.pos[0], d.pos[1] = (idx % 1024) * 4.0, (idx // 1024) * 4.0
    e = afa.Ensemble(n, precision=afa.AFE_F32)
    e.set_type_table([p])
    e.set_logic_period(1 / 500)
    e.set_imu_noise(True, 0.1, 0.2, afa.AFE_SEED_COUNTER)
    e.set_noise_seed(5)
    e.set_state(d.pos, d.vel, d.att, d.ang_vel, d.motor_speed)
    e.set_motor_cmds(d.motor_cmd)
    e.set_gust_process(True, seed=4, sigma_max=0.5, period_us=100000, n_global=n)
    e.set_rates_logic([afa.rates_logic_params_from_type(5)])
    e.set_rates_commands(np.full(n, 9.81, np.float32), np.zeros((3, n), np.float32))
    e.set_step_mode(afa.AFE_STEP_AUTO)
    edges = np.linspace(0, n, N_GROUPS + 1).astype(int)
    mon = afa.StatsMonitor(e, edges)
    mon.set_histogram(HIST_EDGES_M)
    p0 = e.get_state()["pos"]
    wall = {k: [] for k in "abcd"}
    for rep in range(REPS + 3):
        t0 = time.perf_counter()
        rec, hist = mon.update()
        t1 = time.perf_counter()
        st = e.get_state()
        t2 = time.perf_counter()
        st = e.get_state()
        dev2 = (st["pos"][0] - p0[0]) ** 2 + (st["pos"][1] - p0[1]) ** 2
        bins = [(float(np.sqrt(dev2[a:b].mean())), float((st["pos"][2, a:b] <= 0).mean())) for a, b in zip(edges[:-1], edges[1:])]
        t3 = time.perf_counter()
        e.step(1000, 10)
        e.sync()
        t4 = time.perf_counter()
        if rep >= 3:                                   # warm-up
            for k, dt in zip("abcd", (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                wall[k].append(dt * 1e3)
    med = {k: float(np.median(v)) for k, v in wall.items()}
    lo = {k: float(np.min(v)) for k, v in wall.items()}
    out = dict(n=n, reps=REPS, n_groups=N_GROUPS, n_hist_edges=len(HIST_EDGES_M), stats_update_ms=med["a"], get_state_ms=med["b"],
               get_state_numpy_ms=med["c"], ten_steps_ms=med["d"], min_ms=dict(stats_update=lo["a"], get_state=lo["b"], ten_steps=lo["d"]),
               update_over_get_state=med["a"] / med["b"], update_over_ten_steps=med["a"] / med["d"],
               bytes_per_vehicle_update=BYTES_PER_VEHICLE, achieved_GBps=n * BYTES_PER_VEHICLE / (med["a"] * 1e-3) / 1e9,
               bytes_over_the_bus=int(rec.nbytes + hist.nbytes), rms_xy_last_bin_m=bins[-1][0],
               rms_xy_last_bin_from_update_m=float(np.sqrt(rec["sum_h2"][-1] / (rec["count"][-1] - rec["n_invalid"][-1]))))
    mon.close()
    e.close()
    print("RESULT " + json.dumps(out))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]))
    sys.path.insert(0, ROOT)
    provenance = importlib.import_module("agri-fly_amd.provenance")
    rows = []
    for n in SIZES:
        limit = 120 if n <= 65536 else 240
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", str(n)]
        run = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
        if run.returncode != 0 or not line:
            print("stats_probe: n=%d ended with status %d; stopping here\n%s" % (n, run.returncode, run.stderr[-2000:]))
            return 1
        rows.append(json.loads(line[0][7:]))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(kernel_sources=provenance.kernel_source_hashes(("afe_stats.hip",)), rows=rows,
               device_path_faster_than_download=all(r["stats_update_ms"] < r["get_state_ms"] for r in rows))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "stats_probe.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
