"""What one period of the flight stage machine costs on the device, next to the download and upload it replaces:

    python tools/stages_probe.py            -> profiles/stages_probe.json

The parent never opens the GPU: every ensemble size runs in a child of its own under `timeout -k 10`, and the first one
that fails ends the probe.  Per size, medians over 15 alternating repetitions after a warm-up (the method of
tools/gps_estimator_probe.py), fp32 engine with the on-device rates logic and IMU noise, the vehicles in Flight (every
lane runs the controller), each timed with a wait for the engine's stream:
  (a) afe_stages_tick on the engine's true state
  (b) afe_stages_tick with the GPS + IMU estimator attached (a second machine on the same engine)
  (c) get_state() of the ensemble: the download a host-side state machine per vehicle starts from
  (d) afe_set_commands_from_radio of one rates packet per vehicle: the upload it ends with
  (e) afe_stages_tick with the eight counters downloaded
Bytes per vehicle are the slab words a Flight tick touches (afe_stages.hip); the bandwidth is those over the median.
Nobody had measured this kernel before: no figure is promised, the numbers are what they are.
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
# a Flight tick on the fp32 truth: state 10 floats + 2 anchors; 8 bytes read, 5 written; t0 in and out; desired 3, yaw 1, centre 2
# in; last pos / vel / acc 9 and the commanded yaw out; computed, sent and the ring slot 12 floats and a type byte out; the
# delivered slot 4 floats and a byte in, the rates command 4 floats and a byte out
TICK_BYTES = 10 * 4 + 2 * 8 + 8 + 5 + 2 * 8 + (3 + 1 + 2) * 8 + 10 * 8 + 12 * 4 + 1 + 4 * 4 + 1 + 4 * 4 + 1


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
    est = afa.GpsEstimator(e)
    cfg = afa.stages_default_config(5)
    cfg.spool_up_time_s, cfg.takeoff_time_s = 0.0, 0.02      # in Flight after a few ticks, and there for the whole probe
    machines = [afa.FlightStages(e, cfg=cfg), afa.FlightStages(e, cfg=cfg)]
    machines[1].attach_gps_estimator(est)
    for m in machines:
        m.set_desired_position(pos0)
        m.set_centre(pos0[0:2])
    packets = np.tile(np.frombuffer(bytes(afa.radio_create_rates_command(0, 9.81, np.zeros(3, np.float32))), np.uint8), (n, 1))
    wall = {k: [] for k in "abcde"}

    def period():
        for _ in range(10):
            e.step(1000, e.steps_until_tick(1000))
            est.imu()
        est.measure()
        e.sync()

    for rep in range(REPS + 6):
        period()
        t0 = time.perf_counter()
        machines[0].tick(True, False)
        e.sync()
        t1 = time.perf_counter()
        machines[1].tick(True, False)
        e.sync()
        t2 = time.perf_counter()
        st = e.get_state()
        t3 = time.perf_counter()
        e.set_commands_from_radio(packets)
        e.sync()
        t4 = time.perf_counter()
        if rep >= 6:
            for k, dt in zip("abcd", (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                wall[k].append(dt * 1e3)
    for rep in range(REPS):
        period()
        machines[1].tick(True, False)
        t0 = time.perf_counter()
        counts = machines[0].tick(True, False, count=True)
        t1 = time.perf_counter()
        wall["e"].append((t1 - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in wall.items()}
    out = dict(n=n, reps=REPS, tick_ms=med["a"], tick_estimator_ms=med["b"], download_ms=med["c"], upload_ms=med["d"],
               tick_counted_ms=med["e"], tick_bytes_per_vehicle=TICK_BYTES, tick_gb_per_s=n * TICK_BYTES / (med["a"] * 1e-3) / 1e9,
               in_flight=int(counts[3]), in_emergency=int(counts[6]), finite=bool(np.isfinite(st["pos"]).all()))
    for m in machines:
        m.close()
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
            print("stages_probe: n=%d ended with status %d; stopping here\n%s" % (n, run.returncode, run.stderr[-2000:]))
            return 1
        rows.append(json.loads(line[0][7:]))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(kernel_sources=provenance.kernel_source_hashes(("afe_stages.hip", "afe_offboard_math.h", "afe_gps_estimator.hip")), rows=rows)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "stages_probe.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
