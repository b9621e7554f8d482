"""What the range sensor, the explicit ray query and the line-of-sight query cost next to what a host needs today before
it can range anything (a get_state() download) and next to the physics they follow:

    python tools/raycast_probe.py            -> profiles/raycast_probe.json

The parent never opens the GPU: every ensemble size runs in a child of its own under `timeout -k 10`, and the first one
that fails ends the probe.  Per size, medians over alternating repetitions after a warm-up, fp32 engine over bench.py's
config-3 orchard (vehicles moved 12 m east, standing among the trees, yawed at random):
  (a) afe_range_sensor_update, the six-beam set, device outputs    (b) get_state() of the same ensemble
  (c) ten physics steps, default stepping mode
  (d) afe_raycast on the same 6 n rays given explicitly (kernel time, and the call with its uploads and downloads)
  (e) afe_line_of_sight between n pairs of vehicles (any-hit kernel) and (f) afe_raycast with t_max = 1 on the same pairs
      (first-hit kernel): kernel times
and the traversal's counters (tree nodes, triangle box tests, fp64 tests per ray) from the counting build.
"""
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (65536, 1048576)
REPS = 15
REPS_EXPLICIT = 5


def pose_matrix(q):
    """the pose function's matrix (afe_pose.h) for attitudes q [4, n] and the identity mount, in its operation order"""
    c0, c1, c2, c3 = q
    r0, r1, r2, r3 = c0 * c0, c1 * c1, c2 * c2, c3 * c3
    return [r0 + r1 - r2 - r3, 2 * c1 * c2 - 2 * c0 * c3, 2 * c1 * c3 + 2 * c0 * c2,
            2 * c1 * c2 + 2 * c0 * c3, r0 - r1 + r2 - r3, 2 * c2 * c3 - 2 * c0 * c1,
            2 * c1 * c3 - 2 * c0 * c2, 2 * c2 * c3 + 2 * c0 * c1, r0 - r1 - r2 + r3]


def child(n):
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
    pos0 = np.stack([np.full(n, 8.0) + rng.uniform(-1, 0, n) + rng.integers(0, cols - 1, n) * 3.0, y0, np.full(n, altitude)])
    yaw = rng.uniform(-np.pi, np.pi, n)
    att0 = np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)])
    params = afa.params_from_type(5)
    e = afa.Ensemble(n, precision=afa.AFE_F32)
    e.set_type_table([params])
    e.set_imu_noise(True, 0.1, 0.2, afa.AFE_SEED_DECORRELATED)
    e.set_rates_logic([afa.rates_logic_params_from_type(5)])
    e.set_state(pos0, np.zeros((3, n)), att0, np.zeros((3, n)), np.full((4, n), sc.hover_speed(params)))
    e.set_rates_commands(np.full(n, 9.81, np.float32), np.zeros((3, n), np.float32))
    beams = afa.crazyflie_range_beams()
    sensor = afa.RangeSensor(e, cmap, beams)
    bufs = (afa.DeviceBuffer(6 * n * 8), afa.DeviceBuffer(6 * n * 4))
    wall = {k: [] for k in "abc"}
    kernel_ms = []
    for rep in range(REPS + 3):
        t0 = time.perf_counter()
        ms = sensor.update(out=bufs)
        t1 = time.perf_counter()
        st = e.get_state()
        t2 = time.perf_counter()
        e.step(1000, 10)
        e.sync()
        t3 = time.perf_counter()
        if rep >= 3:                                   # warm-up
            for k, dt in zip("abc", (t1 - t0, t2 - t1, t3 - t2)):
                wall[k].append(dt * 1e3)
            kernel_ms.append(ms)
    # the same rays, explicitly: formed on the host from the downloaded state by the definition's arithmetic
    st = e.get_state()
    sensor.update(out=bufs)
    t_dev = bufs[0].download(np.float64, (6, n))
    R = pose_matrix(st["att"])
    origin = np.ascontiguousarray(np.tile(st["pos"], (1, 6)))
    dirs = np.empty((3, 6 * n))
    for b in range(6):
        dr = beams["dir"][b]
        for r in range(3):
            dirs[r, b * n:(b + 1) * n] = (R[3 * r] * dr[0] + R[3 * r + 1] * dr[1]) + R[3 * r + 2] * dr[2]
    t_max = np.repeat(beams["t_max"], n)
    ray_kernel, ray_wall = [], []
    for rep in range(REPS_EXPLICIT + 1):
        t0 = time.perf_counter()
        t_exp, _, ms = cmap.raycast(origin, dirs, t_max, want_ms=True)
        t1 = time.perf_counter()
        if rep >= 1:
            ray_kernel.append(ms)
            ray_wall.append((t1 - t0) * 1e3)
    same = bool(np.array_equal(t_exp.view(np.uint64), t_dev.reshape(-1).view(np.uint64)))
    m = min(6 * n, 6 * 65536)
    stats, _ = cmap.raycast_stats(origin[:, :m], dirs[:, :m], t_max[:m])
    # line of sight between pairs of vehicles: any-hit against first-hit on the same pairs, alternating
    partner = rng.permutation(n)
    p0, p1 = np.ascontiguousarray(st["pos"]), np.ascontiguousarray(st["pos"][:, partner])
    d01 = p1 - p0
    any_ms, first_ms = [], []
    for rep in range(REPS_EXPLICIT + 1):
        blocked, ms_any = cmap.line_of_sight(p0, p1, want_ms=True)
        t_first, _, ms_first = cmap.raycast(p0, d01, 1.0, want_ms=True)
        if rep >= 1:
            any_ms.append(ms_any)
            first_ms.append(ms_first)
    los_same = bool(np.array_equal(blocked, (t_first <= 1.0).astype(np.uint8)))
    los_stats, _ = cmap.raycast_stats(p0[:, :65536], d01[:, :65536], 1.0)
    med = {k: float(np.median(v)) for k, v in wall.items()}
    out = dict(n=n, n_rays=6 * n, reps=REPS, reps_explicit=REPS_EXPLICIT, n_tri=int(len(tris)),
               sensor_update_ms=med["a"], sensor_kernel_ms=float(np.median(kernel_ms)), get_state_ms=med["b"], ten_steps_ms=med["c"],
               update_over_get_state=med["a"] / med["b"], update_over_ten_steps=med["a"] / med["c"],
               share_of_beams_hitting=float(np.isfinite(t_dev).mean()),
               raycast_kernel_ms=float(np.median(ray_kernel)), raycast_call_ms=float(np.median(ray_wall)),
               explicit_rays_equal_sensor_bits=same,
               per_ray=dict(nodes=stats["nodes"] / stats["rays"], tri_box_tests=stats["tri_box_tests"] / stats["rays"],
                            tri_fp64_tests=stats["tri_fp64_tests"] / stats["rays"]),
               los_pairs=n, los_share_blocked=float(blocked.mean()), los_any_hit_kernel_ms=float(np.median(any_ms)),
               los_first_hit_kernel_ms=float(np.median(first_ms)), los_any_equals_first=los_same,
               los_first_hit_per_ray=dict(nodes=los_stats["nodes"] / los_stats["rays"], tri_box_tests=los_stats["tri_box_tests"] / los_stats["rays"],
                                          tri_fp64_tests=los_stats["tri_fp64_tests"] / los_stats["rays"]))
    sensor.close()
    for b in bufs:
        b.close()
    e.close()
    cmap.close()
    print("RESULT " + json.dumps(out))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]))
    sys.path.insert(0, ROOT)
    provenance = importlib.import_module("agri-fly_amd.provenance")
    rows = []
    for n in SIZES:
        limit = 150 if n <= 65536 else 400
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", str(n)]
        run = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
        if run.returncode != 0 or not line:
            print("raycast_probe: n=%d ended with status %d; stopping here\n%s" % (n, run.returncode, run.stderr[-2000:]))
            return 1
        rows.append(json.loads(line[0][7:]))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(kernel_sources=provenance.kernel_source_hashes(("afe_raycast.hip", "afe_clearance_map.h")), rows=rows,
               any_hit_faster=all(r["los_any_hit_kernel_ms"] < r["los_first_hit_kernel_ms"] for r in rows))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "raycast_probe.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
