"""What the mocap estimator costs on the device, next to the download it replaces:

    python tools/estimator_probe.py            -> profiles/estimator_probe.json

The parent never opens the GPU: every ensemble size runs in a child of its own under `timeout -k 10`, and the first one
that fails ends the probe.  Per size, medians over 15 alternating repetitions after a warm-up, fp32 engine with the
on-device rates logic, a follower attached, commands in flight (the ring is full), each with a wait for the engine's stream:
  (a) afe_estimator_measure                       UpdateWithMeasurement for every vehicle
  (b) afe_estimator_predict(0.03)                 GetPrediction: three or four trips through the ring
  (c) afe_follower_tick with the estimator attached: the tick on the prediction, and its announce
  (d) get_state() of the ensemble: the download a host estimator per vehicle starts from (its arithmetic comes on top)
  (e) five physics steps, default stepping mode, for scale (the mocap period)
Nobody had measured these kernels before: no figure is promised, the numbers are what they are.
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
    est = afa.Estimator(e)
    f.attach_estimator(est)
    wall = {k: [] for k in "abcde"}
    for rep in range(REPS + 8):                            # (eight periods of warm-up: the ring is full from then on)
        t0 = time.perf_counter()
        e.step(1000, 5)
        e.sync()
        t1 = time.perf_counter()
        est.measure()
        e.sync()
        t2 = time.perf_counter()
        e.step(1000, 5)
        est.measure()
        e.sync()
        t3 = time.perf_counter()
        est.predict(0.03)
        e.sync()
        t4 = time.perf_counter()
        f.tick()
        e.sync()
        t5 = time.perf_counter()
        st = e.get_state()
        t6 = time.perf_counter()
        if rep >= 8:
            for k, dt in zip("eabcd", (t1 - t0, t2 - t1, t4 - t3, t5 - t4, t6 - t5)):
                wall[k].append(dt * 1e3)
    n_rejected = est.measure(count_rejected=True)
    state, info = est.state(), est.info()
    med = {k: float(np.median(v)) for k, v in wall.items()}
    out = dict(n=n, reps=REPS, measure_ms=med["a"], predict_ms=med["b"], attached_tick_ms=med["c"], get_state_ms=med["d"],
               five_steps_ms=med["e"], bytes_down=int(n * 17 * 8), measure_bytes_per_vehicle=7 * 4 + 2 * 8 + 2 * (20 * 8 + 8) + 2 * 8 + 6 * 8,
               n_rejected=int(n_rejected), slots=info["slots"], n_messages=info["n_messages"], error=info["error"],
               finite=bool(np.isfinite(state["est"]).all() and np.isfinite(st["pos"]).all()))
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
            print("estimator_probe: n=%d ended with status %d; stopping here\n%s" % (n, run.returncode, run.stderr[-2000:]))
            return 1
        rows.append(json.loads(line[0][7:]))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(kernel_sources=provenance.kernel_source_hashes(("afe_estimator.hip", "afe_follower.hip")), rows=rows)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "estimator_probe.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
