"""What one tick of the onboard flight computer costs on the device, next to the round trip a host firmware needs:

    python tools/onboard_probe.py            -> profiles/onboard_probe.json

The parent never opens the GPU: every ensemble size runs in a child of its own under `timeout -k 10`, and the first one
that fails ends the probe.  Per size, medians over 15 repetitions after a warm-up in which (a), (b) and (c) alternate (the
method of tools/stages_probe.py), fp32 engine with the on-device rates logic and IMU noise, every vehicle in the rates state under a
command that is renewed every 10 ticks, each timed window ending in a wait for the engine's stream:
  (a) afe_onboard_tick
  (b) the round trip of a host firmware at the same tick: afe_get_imu (download) + afe_set_motor_cmds (upload)
  (c) afe_onboard_tick with the sixteen counters downloaded
Bytes per vehicle-tick are the slab words a rates-state tick without a new message touches, counted from
afe_onboard.hip; the bandwidth is those over the median of (a).
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
# read: six state bytes, the type byte, the mailbox arrival, the radio, main, reset, estimate and uwb timers (5 x 8), the command
# monitor's value, the battery filter and the voltage (5 floats), the raw accelerometer sample (3), its filter (12), the temperature
# filter (4), the engine's filtered gyro (3), the cycle counter, the main monitor's value, the attitude (4), the rates command (4) and
# the motor command in force (4)
READ_BYTES = 6 + 1 + 8 + 5 * 8 + 4 + 5 * 4 + 3 * 4 + 12 * 4 + 4 * 4 + 3 * 4 + 4 + 4 + 4 * 4 + 4 * 4 + 4 * 4
# written: the three filters (4 + 12 + 4 floats), the cycle counter, the main timer and its value, the estimate timer, the attitude (4),
# the angular velocity (3) and the four forces
WRITE_BYTES = (4 + 12 + 4) * 4 + 4 + 8 + 4 + 8 + 4 * 4 + 3 * 4 + 4 * 4
TICK_BYTES = READ_BYTES + WRITE_BYTES


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
    pos0 = np.stack([rng.uniform(-50, 50, n), rng.uniform(-50, 50, n), rng.uniform(10, 30, n)])
    att0 = np.tile(np.array([[1.0], [0.0], [0.0], [0.0]]), (1, n))
    e.set_state(pos0, np.zeros((3, n)), att0, np.zeros((3, n)), np.full((4, n), sc.hover_speed(params)))
    e.set_motor_cmds(np.full((4, n), sc.hover_speed(params), np.float32))   # (in free fall the first sample is noise and so is the first attitude)
    ob = afa.Onboard(e, quadcopter_type=5)
    thrust, rates = np.full(n, 9.81, np.float32), np.zeros((3, n), np.float32)
    wall = {k: [] for k in "abc"}
    state = dict(ticks=0)

    def to_tick():
        if state["ticks"] % 10 == 0:
            e.set_rates_commands(thrust, rates)
        state["ticks"] += 1
        e.step(1000, e.steps_until_tick(1000))
        e.sync()

    for rep in range(REPS + 6):
        to_tick()
        t0 = time.perf_counter()
        ob.tick()
        e.sync()
        t1 = time.perf_counter()
        gyro, acc = e.get_imu()
        e.set_motor_cmds(cmds if rep else e.get_motor_cmds())     # (what the firmware would have computed: the commands in force)
        e.sync()
        t2 = time.perf_counter()
        cmds = e.get_motor_cmds()
        to_tick()
        t3 = time.perf_counter()
        counts = ob.tick(count=True)
        e.sync()
        t4 = time.perf_counter()
        if rep >= 6:
            wall["a"].append((t1 - t0) * 1e3)
            wall["b"].append((t2 - t1) * 1e3)
            wall["c"].append((t4 - t3) * 1e3)
    med = {k: float(np.median(v)) for k, v in wall.items()}
    out = dict(n=n, reps=REPS, tick_ms=med["a"], host_round_trip_ms=med["b"], tick_counted_ms=med["c"], tick_bytes_per_vehicle=TICK_BYTES,
               tick_gb_per_s=n * TICK_BYTES / (med["a"] * 1e-3) / 1e9, in_rates=int(counts[6]), in_panic=int(counts[3]),
               finite=bool(np.isfinite(gyro).all() and np.isfinite(acc).all()))
    ob.close()
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
            print("onboard_probe: n=%d ended with status %d; stopping here\n%s" % (n, run.returncode, run.stderr[-2000:]))
            return 1
        rows.append(json.loads(line[0][7:]))
        print(json.dumps(rows[-1]), flush=True)
    out = dict(kernel_sources=provenance.kernel_source_hashes(("afe_onboard.hip", "afe_offboard_math.h")), rows=rows)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "onboard_probe.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
