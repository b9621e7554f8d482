"""What one offboard period costs with the follower next to the round trip it replaces:

    python tools/follower_probe.py            -> profiles/follower_probe.json

The parent never opens the GPU: every ensemble size runs in a child of its own under `timeout -k 10`, and the first one
that fails ends the probe.  Per size, medians over 15 alternating repetitions after a warm-up, fp32 engine with the
on-device rates logic, every vehicle on a running plan:
  (a) afe_follower_tick and a wait for the engine's stream: reference, controller, codec and delay line on the device
  (b) the bus traffic of the host path alone: get_state() of the ensemble and set_rates_commands() of four floats per
      vehicle -- WITHOUT the numpy controller in between (tests/orchard_flight.py), which only adds to it
  (c) ten physics steps, default stepping mode, for scale
Nobody had measured either side before: no ratio is promised, the numbers are what they are.
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
    f = afa.Follower(e)
    # a gentle five-second plan for everybody, planned now in the world frame: forward along the camera axis
    coeffs = np.zeros((18, n))
    coeffs[3 * 3 + 2] = rng.uniform(0.05, 0.2, n)          # t^2
    coeffs[3 * 2 + 0] = rng.uniform(-0.02, 0.02, n)        # t^3, sideways: the thrust direction turns
    mount = afa.camera_default_mount()
    grav = np.tile(np.array([[0.0], [9.81], [0.0]]), (1, n))   # gravity in the camera frame of a level vehicle
    f.set_plans(planned=np.ones(n, np.uint8), coeffs=coeffs, tf=np.full(n, 5.0), t_plan_us=np.zeros(n, np.uint64),
                traj_att=np.tile(mount[:, None], (1, n)), offset=pos0, grav=grav)
    hover, level = np.full(n, 9.81, np.float32), np.zeros((3, n), np.float32)
    wall = {k: [] for k in "abc"}
    for rep in range(REPS + 3):
        t0 = time.perf_counter()
        e.step(1000, 10)
        e.sync()
        t1 = time.perf_counter()
        f.tick()
        e.sync()
        t2 = time.perf_counter()
        st = e.get_state()
        e.set_rates_commands(hover, level)                 # (four floats per vehicle, ready made)
        t3 = time.perf_counter()
        if rep >= 3:                                       # warm-up
            for k, dt in zip("cab", (t1 - t0, t2 - t1, t3 - t2)):
                wall[k].append(dt * 1e3)
    n_tracking = f.tick(count_tracking=True)
    med = {k: float(np.median(v)) for k, v in wall.items()}
    out = dict(n=n, reps=REPS, follower_tick_ms=med["a"], host_round_trip_ms=med["b"], ten_steps_ms=med["c"],
               round_trip_over_tick=med["b"] / med["a"], tick_over_ten_steps=med["a"] / med["c"],
               bytes_down=int(n * 17 * 8), bytes_up=int(n * 16), n_tracking=int(n_tracking), finite=bool(np.isfinite(st["pos"]).all()))
    f.close()
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
            print("follower_probe: n=%d ended with status %d; stopping here\n%s" % (n, run.returncode, run.stderr[-2000:]))
            return 1
        rows.append(json.loads(line[0][7:]))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(kernel_sources=provenance.kernel_source_hashes(("afe_follower.hip",)), rows=rows)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "follower_probe.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
