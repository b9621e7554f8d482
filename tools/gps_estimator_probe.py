"""What the GPS + IMU estimator costs on the device, next to the download it replaces:

    python tools/gps_estimator_probe.py            -> profiles/gps_estimator_probe.json

The parent never opens the GPU: every ensemble size runs in a child of its own under `timeout -k 10`, and the first one
that fails ends the probe.  Per size, medians over 15 alternating repetitions after a warm-up (the method of
tools/raycast_probe.py), fp32 engine with the on-device rates logic and IMU noise, a follower attached, each with a wait
for the engine's stream:
  (a) afe_gps_estimator_imu                       Predict for every vehicle: the 9x9 covariance read and written in place
  (b) afe_gps_estimator_measure                   UpdateWithMeasurement: the covariance once more
  (c) afe_follower_tick with the estimator attached: the tick on the estimate (nothing is announced)
  (d) get_state() + afe_get_imu of the ensemble: the download a host estimator per vehicle starts from, 500 times a second
  (e) the physics steps up to the logic tick, default stepping mode, for scale
Bytes per vehicle are the slab words the kernels touch (afe_gps_estimator.hip, LAYOUT); the bandwidth is those over the
median.  Nobody had measured these kernels before: no figure is promised, the numbers are what they are.
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
# Predict: cov 81 in + 81 out, est 13 + 13, corr 3 + 3, the time 1 + 1 (8 B each); own filter 12 + 12 floats, the raw acc 3,
# the engine's filtered gyro 3, the flag word, the type byte.  Update: cov 81 + 81, est 13 + 13, corr 3 out, the time out,
# the position 3 floats and 2 anchors, the flag word.
IMU_BYTES = (81 * 2 + 13 * 2 + 3 * 2 + 2) * 8 + (12 * 2 + 3 + 3 + 1) * 4 + 1
MEASURE_BYTES = (81 * 2 + 13 * 2 + 3 + 1 + 2) * 8 + (3 + 1) * 4


def child(n):
    import numpy as np
    import torch  # noqa: F401  (first: see INTEGRATION.md section 5)
    sys.path.insert(0, ROOT)
    afa = importlib.import_module("agri-fly_amd")
    sc = afa.scenarios
    rng = np.random.default_rng(0)
    params = afa.params_from_type(5)
    e = afa.Ensemble(n, precision=afa.AFE_F32)
    e.set_type_table([params])
    e.set_imu_noise(True, 0.1, 0.2, afa.AFE_SEED_DECORRELATED)
    e.set_rates_logic([afa.rates_logic_params_from_type(5)])
    pos0 = np.stack([rng.uniform(-50, 50, n), rng.uniform(-50, 50, n), rng.uniform(1, 3, n)])
    att0 = np.tile(np.array([[1.0], [0.0], [0.0], [0.0]]), (1, n))
    e.set_state(pos0, np.zeros((3, n)), att0, np.zeros((3, n)), np.full((4, n), sc.hover_speed(params)))
    e.set_rates_commands(np.full(n, 9.81, np.float32), np.zeros((3, n), np.float32))
    f = afa.Follower(e)                                    # nobody has a plan: everybody holds its place
    est = afa.GpsEstimator(e)
    f.attach_gps_estimator(est)
    wall = {k: [] for k in "abcde"}
    for rep in range(REPS + 4):                            # (warm-up: the NaN start of the covariance is behind the first update)
        for k in range(5):
            t0 = time.perf_counter()
            e.step(1000, e.steps_until_tick(1000))
            e.sync()
            t1 = time.perf_counter()
            est.imu()
            e.sync()
            t2 = time.perf_counter()
            if rep >= 4 and k == 0:
                wall["e"].append((t1 - t0) * 1e3)
                wall["a"].append((t2 - t1) * 1e3)
        t2 = time.perf_counter()
        est.measure()
        e.sync()
        t3 = time.perf_counter()
        f.tick()
        e.sync()
        t4 = time.perf_counter()
        st = e.get_state()
        imu = e.get_imu()
        t5 = time.perf_counter()
        if rep >= 4:
            for k, dt in zip("bcd", (t3 - t2, t4 - t3, t5 - t4)):
                wall[k].append(dt * 1e3)
    n_singular = est.measure(count_reinitialised=True)
    state, info = est.state(0, min(n, 65536)), est.info()
    med = {k: float(np.median(v)) for k, v in wall.items()}
    out = dict(n=n, reps=REPS, imu_ms=med["a"], measure_ms=med["b"], attached_tick_ms=med["c"], download_ms=med["d"],
               steps_to_tick_ms=med["e"], bytes_down=int(n * (17 * 8 + 6 * 4)), imu_bytes_per_vehicle=IMU_BYTES,
               measure_bytes_per_vehicle=MEASURE_BYTES, imu_gb_per_s=n * IMU_BYTES / (med["a"] * 1e-3) / 1e9,
               measure_gb_per_s=n * MEASURE_BYTES / (med["b"] * 1e-3) / 1e9, n_singular=int(n_singular), n_imu=info["n_imu"],
               n_measures=info["n_measures"], symmetrise="pairs, one pass: each word read once and written once",
               finite=bool(np.isfinite(state["est"]).all() and np.isfinite(state["cov"]).all() and np.isfinite(st["pos"]).all()
                           and np.isfinite(imu[0]).all()))
    f.close()
    est.close()
    e.close()
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
            print("gps_estimator_probe: n=%d ended with status %d; stopping here\n%s" % (n, run.returncode, run.stderr[-2000:]))
            return 1
        rows.append(json.loads(line[0][7:]))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(kernel_sources=provenance.kernel_source_hashes(("afe_gps_estimator.hip", "afe_follower.hip")), rows=rows)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "gps_estimator_probe.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
