"""What auditing every accepted plan against the mesh costs on the device, next to the route a host had before
(evaluate the sample points on the host, afe_clearance_query on them, reduce in numpy) and next to the render -> plan
round that produced the plans:

    python tools/path_clearance_probe.py            -> profiles/path_clearance_probe.json

The parent never opens the GPU: every configuration (samples per path) runs in a child of its own under `timeout -k 10`,
and the first one that fails ends the probe.  Per configuration, medians over alternating repetitions after a warm-up,
fp32 engine over bench.py's config-3 orchard, 65 536 vehicles standing among the trees (moved 12 m east, as
tools/clearance_probe.py places them), real plans from one render -> plan round with config 3's planner settings:
  (a) afe_clearance_plans_engine: wall and kernel time
  (b) the host route: get_state() for the poses, sample points in numpy by the definition's expressions,
      afe_clearance_query on them (unbounded, as the definition asks), numpy reduction: wall time in total and per
      component (the state download is reported on its own), and the kernel time of the query alone
  (c) one render -> plan round
  (d) the traversal's counters per sample (tree nodes, triangle box tests, fp64 evaluations), path kernel and point
      query on the same samples, from the counting builds, on the first 4 096 found plans
and the study's first ground-truth figure: of the plans the planner accepted, how many have a sample within the true
vehicle radius of the mesh.  That is a finding about camera + planner, recorded, not judged.
"""
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 65536
SAMPLES = (64, 256)
REPS = 31
N_COUNTED = 4096


def _poses(pos, att, mount):
    """origin [3, n] and row-major camera-to-world matrix [9, n] of att * mount: afe_camera_pose_kernel's arithmetic"""
    q, m = att, mount
    c0 = m[0] * q[0] - m[1] * q[1] - m[2] * q[2] - m[3] * q[3]
    c1 = m[1] * q[0] + m[0] * q[1] + m[3] * q[2] - m[2] * q[3]
    c2 = m[2] * q[0] - m[3] * q[1] + m[0] * q[2] + m[1] * q[3]
    c3 = m[3] * q[0] + m[2] * q[1] - m[1] * q[2] + m[0] * q[3]
    r0, r1, r2, r3 = c0 * c0, c1 * c1, c2 * c2, c3 * c3
    R = np.stack([r0 + r1 - r2 - r3, 2 * c1 * c2 - 2 * c0 * c3, 2 * c1 * c3 + 2 * c0 * c2,
                  2 * c1 * c2 + 2 * c0 * c3, r0 - r1 + r2 - r3, 2 * c2 * c3 - 2 * c0 * c1,
                  2 * c1 * c3 - 2 * c0 * c2, 2 * c2 * c3 + 2 * c0 * c1, r0 - r1 - r2 + r3])
    return pos, R


def _sample_points(coeffs, tf, origin, R, K):
    """the definition's sample times [n, K] and world points [3, n, K], vectorised over the paths"""
    k = np.arange(K, dtype=np.float64)
    t = 0.0 + (tf[:, None] - 0.0) * (k / np.float64(K - 1))[None, :]
    t[:, K - 1] = tf
    p = []
    for axis in range(3):
        v = np.broadcast_to(coeffs[:, 0, axis][:, None], t.shape)
        for j in range(1, 6):
            v = v * t + coeffs[:, j, axis][:, None]
        p.append(v)
    w = np.stack([origin[r][:, None] + ((R[3 * r][:, None] * p[0] + R[3 * r + 1][:, None] * p[1]) + R[3 * r + 2][:, None] * p[2])
                  for r in range(3)])
    return t, w


def child(K):
    import torch  # noqa: F401  (first: see INTEGRATION.md section 5)
    sys.path.insert(0, ROOT)
    afa = importlib.import_module("agri-fly_amd")
    sc = afa.scenarios
    n = N
    rows, cols, altitude = 6, 10, 1.2
    tris = sc.orchard_mesh(rows=rows, cols=cols, seed=0)
    cmap = afa.ClearanceMap(tris)
    scene = afa.Scene(tris)
    cam = afa.camera_default(320, 240)
    mount = afa.camera_default_mount()
    params = afa.params_from_type(5)
    rng = np.random.default_rng(0)
    lane = rng.integers(0, rows - 1, n)
    on_row = rng.random(n) < 0.5
    y0 = np.where(on_row, lane * 4.0 + rng.uniform(-0.3, 0.3, n), lane * 4.0 + 2.0 + rng.uniform(-0.8, 0.8, n))
    pos0 = np.stack([np.full(n, 8.0) + rng.uniform(-1, 0, n), y0, np.full(n, altitude)])
    goal = np.stack([np.full(n, (cols - 1) * 3.0 + 8.0), y0, np.full(n, altitude)])
    att0 = np.tile(np.array([[1.0], [0.0], [0.0], [0.0]]), (1, n))
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
    vel_c = inv(st["vel"])
    grav_c = inv(np.tile(np.array([[0.0], [0.0], [-9.81]]), (1, n)))
    goal_c = inv(goal - st["pos"])
    round_ms = []
    for rep in range(3):                                  # (c); the first round allocates the planner's scratch
        t0 = time.perf_counter()
        ms_r = scene.render_engine(e, cam, mount, out=buf)
        out, _, ms_p = afa.rappids_plan(cfg, buf, vel_c, np.zeros((3, n)), grav_c, samples, cost_vec=goal_c)
        round_ms.append(((time.perf_counter() - t0) * 1e3, ms_r, ms_p))
    plans = afa.plans_as_array(out).copy()
    found = plans["found"] != 0
    buf.close()
    afa.planner_release_scratch()

    wall = {"a": [], "b": [], "b_state": [], "b_points": [], "b_query": [], "b_reduce": []}
    kernel = {"a": [], "b": []}
    radius2 = np.float64(radius) * np.float64(radius)
    for rep in range(REPS + 2):
        t0 = time.perf_counter()
        rec, n_col, ms_a = cmap.plans_engine(e, plans, mount, n_samples=K, radius=radius)
        t1 = time.perf_counter()
        # the route of the parent commit: state download, points on the host, point query, numpy reduction
        s = e.get_state()
        t1b = time.perf_counter()
        o_h, R_h = _poses(s["pos"], s["att"], mount)
        t, w = _sample_points(plans["coeffs"], plans["tf"], o_h, R_h, K)
        t2 = time.perf_counter()
        d2, tri, _, ms_b = cmap.query(w.reshape(3, n * K), want_closest=False)
        t3 = time.perf_counter()
        d2 = d2.reshape(n, K)
        hit = (d2 <= radius2) & found[:, None]
        n_hit_b = hit.sum(axis=1)
        k_min_b = np.argmin(d2, axis=1)
        min_b = np.where(found, d2[np.arange(n), k_min_b], np.inf)
        t4 = time.perf_counter()
        if rep >= 2:                                   # warm-up
            wall["a"].append((t1 - t0) * 1e3)
            wall["b"].append((t4 - t1) * 1e3)
            wall["b_state"].append((t1b - t1) * 1e3)
            wall["b_points"].append((t2 - t1b) * 1e3)
            wall["b_query"].append((t3 - t2) * 1e3)
            wall["b_reduce"].append((t4 - t3) * 1e3)
            kernel["a"].append(ms_a)
            kernel["b"].append(ms_b)
    agree = bool(np.array_equal(rec["n_hit"], n_hit_b) and np.array_equal(rec["min_dist2"], min_b) and
                 np.array_equal(rec["k_min"][found], k_min_b[found]) and n_col == int((n_hit_b > 0).sum()))
    # (d) on the first found plans
    pick = np.nonzero(found)[0][:N_COUNTED]
    tr = np.stack([np.zeros(pick.size), plans["tf"][pick]])
    st_path, _ = cmap.paths_stats(plans["coeffs"][pick], tr, o_h[:, pick], R_h[:, pick], n_samples=K, radius=radius)
    st_point, _ = cmap.query_stats(w[:, pick].reshape(3, pick.size * K))
    per = lambda d, total: {k: d[k] / total for k in ("nodes", "tri_box_tests", "tri_fp64_evals")}    # noqa: E731
    med = lambda v: float(np.median(v))                                                                # noqa: E731
    fin = rec["min_dist2"][found]
    out = dict(n=n, n_samples=K, reps=REPS, n_tri=int(len(tris)), radius=radius, max_dist="inf",
               plans_engine_ms=med(wall["a"]), plans_engine_kernel_ms=med(kernel["a"]),
               host_route_ms=med(wall["b"]), host_route_get_state_ms=med(wall["b_state"]), host_route_points_ms=med(wall["b_points"]), host_route_query_ms=med(wall["b_query"]),
               host_route_reduce_ms=med(wall["b_reduce"]), host_route_query_kernel_ms=med(kernel["b"]),
               routes_agree=agree,
               render_plan_round_ms=med([r[0] for r in round_ms[1:]]), render_kernel_ms=med([r[1] for r in round_ms[1:]]),
               plan_kernel_ms=med([r[2] for r in round_ms[1:]]),
               plans_found=int(found.sum()), plans_found_colliding=int((rec["n_hit"][found] > 0).sum()), n_colliding=int(n_col),
               smallest_min_dist2=float(fin.min()) if fin.size else None,
               start_inside_radius=int((rec["k_first_hit"][found] == 0).sum()),
               per_sample_path_kernel=per(st_path, st_path["samples"]), per_sample_point_query=per(st_point, st_point["points"]),
               counted_paths=int(pick.size))
    e.close()
    scene.close()
    cmap.close()
    print("RESULT " + json.dumps(out))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]))
    sys.path.insert(0, ROOT)
    provenance = importlib.import_module("agri-fly_amd.provenance")
    rows = []
    for K in SAMPLES:
        cmd = ["timeout", "-k", "10", str(240 if K <= 64 else 420), sys.executable, os.path.abspath(__file__), "--child", str(K)]
        run = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
        if run.returncode != 0 or not line:
            print("path_clearance_probe: n_samples=%d ended with status %d; stopping here\n%s" % (K, run.returncode, run.stderr[-2000:]))
            return 1
        rows.append(json.loads(line[0][7:]))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(kernel_sources=provenance.kernel_source_hashes(("afe_clearance.hip",)), rows=rows)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "path_clearance_probe.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
