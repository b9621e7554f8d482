"""What the swept clearance entries cost next to their point and sampled siblings on the same inputs in the same run:

    python tools/sweep_probe.py            -> profiles/sweep_probe.json

The parent never opens the GPU: every configuration runs in a child of its own under `timeout -k 10`, and the first one
that fails ends the probe.  fp32 engine over bench.py's config-3 orchard, vehicles among the trees (moved 12 m east, as
tools/clearance_probe.py places them).  Medians over alternating repetitions after a warm-up.
  monitor, 65 536 and 2^20 vehicles flying east at 3 m/s, ten 1 ms steps between two updates (3 cm of flight):
      (a) the swept monitor's update     (b) the point monitor's update, on the same positions
      and the counting builds' figures per vehicle for the last tick's segments and for its end points
  plans, 65 536 vehicles, real plans from one render -> plan round with config 3's planner settings, K = 64:
      (c) afe_clearance_plans_engine_swept     (d) afe_clearance_plans_engine
      the counting builds' figures per chord / per sample on the first 4 096 found plans, how many accepted plans only the
      chords find within the vehicle radius, and the largest afe_path_chord_deviation bound among the found plans
No time is fixed in advance: the yardstick is the sibling.
"""
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (65536, 1048576)
N_PLANS = 65536
K = 64
REPS = 31
N_COUNTED = 4096
SEARCH = 2.0
ROWS, COLS, ALTITUDE = 6, 10, 1.2


def _afa():
    import torch  # noqa: F401  (first: see INTEGRATION.md section 5)
    sys.path.insert(0, ROOT)
    return importlib.import_module("agri-fly_amd")


def _start(n):
    rng = np.random.default_rng(0)
    lane = rng.integers(0, ROWS - 1, n)
    on_row = rng.random(n) < 0.5
    y0 = np.where(on_row, lane * 4.0 + rng.uniform(-0.3, 0.3, n), lane * 4.0 + 2.0 + rng.uniform(-0.8, 0.8, n))
    pos0 = np.stack([np.full(n, 8.0) + rng.uniform(-1, 0, n), y0, np.full(n, ALTITUDE)])
    att0 = np.tile(np.array([[1.0], [0.0], [0.0], [0.0]]), (1, n))
    return pos0, y0, att0


def _per(d, total):
    return {k: d[k] / total for k in ("nodes", "tri_box_tests", "tri_fp64_evals")}


def child_monitor(n):
    afa = _afa()
    sc = afa.scenarios
    tris = sc.orchard_mesh(rows=ROWS, cols=COLS, seed=0)
    cmap = afa.ClearanceMap(tris)
    pos0, _, att0 = _start(n)
    params = afa.params_from_type(5)
    e = afa.Ensemble(n, precision=afa.AFE_F32)
    e.set_type_table([params])
    e.set_imu_noise(True, 0.1, 0.2, afa.AFE_SEED_DECORRELATED)
    e.set_rates_logic([afa.rates_logic_params_from_type(5)])
    vel0 = np.stack([np.full(n, 3.0), np.zeros(n), np.zeros(n)])
    e.set_state(pos0, vel0, att0, np.zeros((3, n)), np.full((4, n), sc.hover_speed(params)))
    e.set_rates_commands(np.full(n, 9.81, np.float32), np.zeros((3, n), np.float32))
    swept = afa.ContactMonitor(e, cmap, 0.116, SEARCH, swept=True)
    point = afa.ContactMonitor(e, cmap, 0.116, SEARCH)
    wall = {"swept": [], "point": [], "steps": []}
    prev = cur = None
    for rep in range(REPS + 3):
        t0 = time.perf_counter()
        e.step(1000, 10)
        e.sync()
        t1 = time.perf_counter()
        first = ("swept", "point") if rep % 2 == 0 else ("point", "swept")     # alternate who goes first
        took, counts = {}, {}
        for name in first:
            ta = time.perf_counter()
            counts[name] = (swept if name == "swept" else point).update()
            took[name] = time.perf_counter() - ta
        if rep >= 3:                                   # warm-up
            wall["steps"].append((t1 - t0) * 1e3)
            for name in first:
                wall[name].append(took[name] * 1e3)
        if rep >= REPS + 1:
            prev, cur = cur, e.get_state()["pos"]
    m = min(n, 65536)
    st_seg, _ = cmap.segments_stats(prev[:, :m], cur[:, :m], SEARCH)
    st_pt, _ = cmap.query_stats(cur[:, :m], SEARCH)
    ls, lp = swept.get(), point.get()
    med = {k: float(np.median(v)) for k, v in wall.items()}
    out = dict(what="monitor", n=n, reps=REPS, n_tri=int(len(tris)), search_radius=SEARCH, metres_per_update=float(np.linalg.norm(cur - prev, axis=0).mean()),
               swept_update_ms=med["swept"], point_update_ms=med["point"], ten_steps_ms=med["steps"],
               swept_over_point=med["swept"] / med["point"], swept_over_ten_steps=med["swept"] / med["steps"],
               ever_in_contact_swept=counts["swept"][1], ever_in_contact_point=counts["point"][1],
               closer_than_point_saw=int((ls["min_dist2"] < lp["min_dist2"]).sum()),
               per_segment=_per(st_seg, st_seg["segments"]), per_point=_per(st_pt, st_pt["points"]))
    swept.close()
    point.close()
    e.close()
    cmap.close()
    print("RESULT " + json.dumps(out))


def child_plans():
    afa = _afa()
    sc = afa.scenarios
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from path_clearance_probe import _poses
    n = N_PLANS
    tris = sc.orchard_mesh(rows=ROWS, cols=COLS, seed=0)
    cmap = afa.ClearanceMap(tris)
    scene = afa.Scene(tris)
    cam = afa.camera_default(320, 240)
    mount = afa.camera_default_mount()
    params = afa.params_from_type(5)
    pos0, y0, att0 = _start(n)
    goal = np.stack([np.full(n, (COLS - 1) * 3.0 + 8.0), y0, np.full(n, ALTITUDE)])
    e = afa.Ensemble(n, precision=afa.AFE_F32)
    e.set_type_table([params])
    e.set_state(pos0, np.zeros((3, n)), att0, np.zeros((3, n)), np.full((4, n), sc.hover_speed(params)))
    buf = afa.DeviceBuffer(n * 240 * 320 * 2)
    cfg = afa.planner_default_config(320, 240, cam.depth_scale, cam.focal_length, 2 * params.arm_length, 3 * params.arm_length, 0.5)
    cfg.cost_type = 1
    radius = float(cfg.true_vehicle_radius)
    samples = afa.planner_samples(0, 320, 240, 192)
    st = e.get_state()
    origin, R = _poses(st["pos"], st["att"], mount)
    inv = lambda v: np.stack([R[0] * v[0] + R[3] * v[1] + R[6] * v[2], R[1] * v[0] + R[4] * v[1] + R[7] * v[2],    # noqa: E731
                              R[2] * v[0] + R[5] * v[1] + R[8] * v[2]])
    scene.render_engine(e, cam, mount, out=buf)
    out, _, _ = afa.rappids_plan(cfg, buf, inv(st["vel"]), np.zeros((3, n)), inv(np.tile(np.array([[0.0], [0.0], [-9.81]]), (1, n))), samples,
                                 cost_vec=inv(goal - st["pos"]))
    plans = afa.plans_as_array(out).copy()
    found = plans["found"] != 0
    buf.close()
    afa.planner_release_scratch()
    wall = {"swept": [], "sampled": []}
    kernel = {"swept": [], "sampled": []}
    for rep in range(REPS + 2):
        order = ("swept", "sampled") if rep % 2 == 0 else ("sampled", "swept")
        for name in order:
            t0 = time.perf_counter()
            if name == "swept":
                rec_w, col_w, ms = cmap.plans_engine_swept(e, plans, mount, n_samples=K, radius=radius)
            else:
                rec_s, col_s, ms = cmap.plans_engine(e, plans, mount, n_samples=K, radius=radius)
            if rep >= 2:
                wall[name].append((time.perf_counter() - t0) * 1e3)
                kernel[name].append(ms)
    pick = np.nonzero(found)[0][:N_COUNTED]
    tr = np.stack([np.zeros(pick.size), plans["tf"][pick]])
    st_w, _ = cmap.paths_swept_stats(plans["coeffs"][pick], tr, origin[:, pick], R[:, pick], n_samples=K, radius=radius)
    st_s, _ = cmap.paths_stats(plans["coeffs"][pick], tr, origin[:, pick], R[:, pick], n_samples=K, radius=radius)
    bounds = [afa.path_chord_deviation(plans["coeffs"][i], 0.0, plans["tf"][i], R[:, i], K) for i in pick]
    med = lambda v: float(np.median(v))                                                                # noqa: E731
    hit_w, hit_s = rec_w["n_hit"][found] > 0, rec_s["n_hit"][found] > 0
    res = dict(what="plans", n=n, n_samples=K, reps=REPS, n_tri=int(len(tris)), radius=radius,
               plans_engine_swept_ms=med(wall["swept"]), plans_engine_swept_kernel_ms=med(kernel["swept"]),
               plans_engine_ms=med(wall["sampled"]), plans_engine_kernel_ms=med(kernel["sampled"]),
               swept_over_sampled_kernel=med(kernel["swept"]) / med(kernel["sampled"]),
               plans_found=int(found.sum()), colliding_swept=int(col_w), colliding_sampled=int(col_s),
               found_only_by_chords=int((hit_w & ~hit_s).sum()), sampled_hit_missed_by_chords=int((hit_s & ~hit_w).sum()),
               never_farther=bool((rec_w["min_dist2"] <= rec_s["min_dist2"]).all()),
               strictly_closer=int((rec_w["min_dist2"][found] < rec_s["min_dist2"][found]).sum()),
               chord_deviation_bound_max_m=float(np.max(bounds)), chord_deviation_bound_median_m=float(np.median(bounds)),
               per_chord=_per(st_w, st_w["chords"]), per_sample=_per(st_s, st_s["samples"]), counted_paths=int(pick.size))
    e.close()
    scene.close()
    cmap.close()
    print("RESULT " + json.dumps(res))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        return child_plans() if sys.argv[2] == "plans" else child_monitor(int(sys.argv[2]))
    sys.path.insert(0, ROOT)
    provenance = importlib.import_module("agri-fly_amd.provenance")
    rows = []
    for what, limit in [(str(n), 120 if n <= 65536 else 300) for n in SIZES] + [("plans", 300)]:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", what]
        run = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
        if run.returncode != 0 or not line:
            print("sweep_probe: %s ended with status %d; stopping here\n%s" % (what, run.returncode, run.stderr[-2000:]))
            return 1
        rows.append(json.loads(line[0][7:]))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(kernel_sources=provenance.kernel_source_hashes(("afe_clearance.hip",)), rows=rows)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sweep_probe.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
