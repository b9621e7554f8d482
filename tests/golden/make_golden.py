#!/usr/bin/env python3
"""Regenerates the committed fixtures under tests/golden/.

Run in the build container (needs /root/reference for the timer probe):

    python tests/golden/make_golden.py

* timer_cadence.json  <- oracle/_ref/timer_probe: the REFERENCE's own
  Timer / ManualTimer / CommunicationsDelay headers compiled from where they
  lie under /root/reference (they need no Eigen) and driven through the call
  sequence of Quadcopter_T::Run inside the Rappids_Simulator loop.
* rng_kat.json        <- oracle/_ref/rng_probe: libstdc++'s
  std::default_random_engine + std::normal_distribution<double>, the library
  code the reference's IMU noise comes from, compiled with g++.
* lpf_kat.json        <- oracle/_ref/lpf_probe: the REFERENCE's own
  LowPassFilterSecondOrder.hpp (stand-alone header) with the onboard logic's
  gyro / accelerometer settings.
* telemetry_kat.json  <- oracle/_ref/telemetry_probe: the REFERENCE's own
  TelemetryPacket.hpp (stand-alone header): packets -> 30-byte wire form -> back.
* planner_math_kat.json <- oracle/_ref/traj_probe: the REFERENCE's own RootFinder.hpp
  and SingleAxisTrajectory.{hpp,cpp} (stand-alone sources) + libstdc++ mt19937.
* uwb_kat.json        <- oracle/_ref/uwb_probe: libstdc++'s std::mt19937 +
  uniform_real_distribution + normal_distribution in the statement sequence of
  the reference's UWBNetwork::Run completion branch (UWBNetwork.cpp:4-6,19,66-71).
* motion_kat.json     <- oracle/_ref/motion_probe: the REFERENCE's own Rotation.hpp
  (Rotation<double>; Rotation<float> for the IMU mount) and Motor.{hpp,cpp} on a
  ManualTimer, compiled in place against a declaration-only <Eigen/Dense>
  (oracle/eigen_decl).  Every attitude and body rate in it is a float32 value held
  in a double, so one fixture serves the fp64 and the fp32 engine.
* oracle_regression.npz <- the oracle itself (NOT the reference): seeded
  single-step / rollout vectors that freeze the restatement so later edits of
  oracle/agrifly_oracle.c cannot drift silently.  It pins nothing against the
  reference (rigid-body parity is unpinned).
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

TIMER_CASES = [
    # (loop dt [s] as the loop writes it, onboard logic period [s], runs)
    ("1.0/500.0", "1.0/500.0", 40),   # the reference's own setting (main.cpp:140,177)
    ("1.0/1000.0", "1.0/500.0", 40),  # BASELINE.json dt = 1 ms
    ("1.0/1000.0", "1.0/1000.0", 40),
    ("1.0/2000.0", "1.0/500.0", 40),
    ("1.0/1000.0", "0.0029", 60),     # period*1e6 truncates to 2899 us
    ("1.0/250.0", "1.0/500.0", 20),   # dt > period: one tick per run, growing lag
    ("1.0/300.0", "1.0/500.0", 30),   # uint64_t(dt*1e6) truncates to 3333 us
    ("1.0/1000.0", "1.0/30.0", 120),  # the image-request cadence (main.cpp:198-200)
]


MIN_ANGLE = 4.84813681e-6   # Rotation.hpp:39


def _f32(x):
    """float32-representable doubles (the fp32 engine stores them unchanged)"""
    return [float(v) for v in np.asarray(x, np.float32).reshape(-1)]


def _unit_f32(rng):
    q = rng.standard_normal(4)
    return _f32(q / np.linalg.norm(q))


def _hex(vals):
    return " ".join(float(v).hex() for v in vals)


def _switch_rates(dt_us):
    """single-axis rates whose kernel-side fp32 theta^2 = fl(fl(fl(dt) w)^2) lands just below and just at / above 0.25,
    the fp32 increment's series / squaring switch (afe_kernels.hip rotvec_to_quat)"""
    dt = np.float32(dt_us * 1e-6)
    w = np.float32(0.5 / float(dt))
    cand = [w]
    for _ in range(12):
        cand = [np.nextafter(cand[0], np.float32(0))] + cand + [np.nextafter(cand[-1], np.float32(np.inf))]
    t = [(np.float32(dt * c) * np.float32(dt * c)) for c in cand]
    below = max(c for c, tt in zip(cand, t) if tt < np.float32(0.25))
    above = min(c for c, tt in zip(cand, t) if tt >= np.float32(0.25))
    return [float(below), float(above)]


# per-step angles |w| dt of the one-step attitude cases: the arc-second identity threshold (Rotation.hpp:39) outside and
# at the edge of its fp32 rounding band, the series range, the squarings k = 1..8 (1, 2, 3, 4, 6, 10, 30, 100 rad), both
# sign changes of the scalar part (pi, 2 pi) and two angles past the fp32 increment's accuracy range
STEP_ANGLES = [MIN_ANGLE * (1 - 1e-3), MIN_ANGLE * (1 - 1e-6), MIN_ANGLE * (1 + 1e-6), MIN_ANGLE * (1 + 1e-3),
               1e-4, 0.1, 0.5, 1.0, 2.0, 3.0, 4.0, 6.0, 10.0, 30.0, 100.0,
               np.pi - 1e-6, np.pi, np.pi + 1e-6, 2 * np.pi - 1e-6, 2 * np.pi, 2 * np.pi + 1e-6, 300.0, 1000.0]
AXES = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0), (0.0, -0.6, 0.8), (2.0, -3.0, 6.0), (-1.0, 4.0, 8.0)]


def make_motion_kat(probe):
    rng = np.random.default_rng(20261016)
    lines, kinds = [], []

    def case(kind, line):
        kinds.append(kind)
        lines.append(line)

    # FromRotationVector on doubles: both neighbouring doubles of MIN_ANGLE and MIN_ANGLE itself on one axis (theta is
    # then exactly that double), x(1 +- 1e-6), the series / squaring switch, k = 1..8, pi and 2 pi
    below, above = np.nextafter(MIN_ANGLE, 0.0), np.nextafter(MIN_ANGLE, 1.0)
    rv = [(0.0, 0.0, 0.0), (below, 0, 0), (MIN_ANGLE, 0, 0), (above, 0, 0), (0, -below, 0), (0, 0, above),
          (0, MIN_ANGLE * (1 - 1e-6), 0), (0, 0, MIN_ANGLE * (1 + 1e-6))]
    for th in (MIN_ANGLE * (1 + 1e-6), 1e-4, 0.1, 0.5, np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0),
               1.0, 2.0, 3.0, 4.0, 6.0, 10.0, 30.0, 100.0, np.pi - 1e-6, np.pi, np.pi + 1e-6,
               2 * np.pi - 1e-6, 2 * np.pi, 2 * np.pi + 1e-6):
        for ax in AXES[3:5]:
            a = np.asarray(ax) / np.linalg.norm(ax)
            rv.append(tuple(th * a))
    for r in rv:
        case("rotvec", "R " + _hex(r))

    # the step's increment composed with an attitude, att * FromRotationVector(angVel * dt) (Quadcopter_T.cpp:142)
    for dt_us in (1000, 4000):
        dt = dt_us * 1e-6
        rates = [[0.0, 0.0, 0.0]] + [[w, 0.0, 0.0] for w in _switch_rates(dt_us)]
        rates += [[0.0, 0.0, -w] for w in _switch_rates(dt_us)]
        for k, th in enumerate(STEP_ANGLES):
            for j in range(3):
                ax = np.asarray(AXES[(2 * k + j) % len(AXES)], float)
                rates.append(_f32(th / dt * ax / np.linalg.norm(ax)))
        for w in rates:
            case("step", "P " + _hex(_unit_f32(rng) + list(w) + [dt]))

    for _ in range(12):
        a, b = _unit_f32(rng), list(rng.standard_normal(4))
        case("mul", "M " + _hex(a + b))
    for _ in range(12):
        case("rotate", "V " + _hex(list(rng.standard_normal(4)) + list(rng.uniform(-20, 20, 3))))
    eul = [(0.0, np.pi / 2, 0.3), (1.0, -np.pi / 2, -2.0), (np.pi, 0.0, -np.pi)] + \
        [tuple(rng.uniform(-4, 4, 3)) for _ in range(9)]
    for e in eul:
        case("euler", "E " + _hex(e))
    # (unit quaternions: ToEulerYPR's asin is NaN past |1|, which no JSON fixture holds)
    quats = [[0.5, 0.5, 0.5, 0.5], [0.6, 0.0, 0.8, 0.0], [0.0, 0.0, 0.0, 1.0]] + \
        [list(q / np.linalg.norm(q)) for q in rng.standard_normal((9, 4))]
    for q in quats:
        case("to_euler", "Y " + _hex(q))
    # the IMU-mount matrix (Quadcopter_T.cpp:78-80): every shipped type's angles are 0 (QuadcopterConstants.hpp), so
    # tilted mounts as well
    imu = [(0.0, 0.0, 0.0)] + [tuple(_f32(rng.uniform(-0.5, 0.5, 3))) for _ in range(5)] + [(0.0, 0.0, 3.0), (-3.0, 1.5, 0.0)]
    for y in imu:
        case("imu_mount", "F " + _hex(y))

    # rotors: each shipped type (tau = J = 0) and two lagged variants (tau, J > 0; one with a nonzero minimum speed),
    # the clockwise motor 0 or the counter-clockwise motor 1; three dt schedules shared by the device test
    # (1 ms, 4 ms, and one with dt < 1 us early returns -- dt_us = 0 -- and a 1 us step)
    from oracle import oracle_py
    schedules = {"1ms": [1000] * 8, "4ms": [4000] * 6, "mixed": [1000, 0, 1000, 4000, 0, 0, 1000, 1, 1000]}
    motors = []
    for base in (1, 2, 4, 5):
        op = oracle_py.params_from_type(base)
        wmax = op.motor_max_speed
        variants = [dict(tau=0.0, J=0.0, wmin=0.0)]
        if base == 2:
            variants.append(dict(tau=0.02, J=1.5e-8, wmin=0.0))
        if base == 5:
            variants.append(dict(tau=0.005, J=4e-8, wmin=0.1 * wmax))
        for v in variants:
            for k, (sched, dts) in enumerate(sorted(schedules.items())):
                m = k % 2
                # below zero, zero, mid-range, above the maximum, below the minimum, then a changing ramp
                cmds = [-50.0, 0.0, 0.5 * wmax, 1.7 * wmax, 0.05 * wmax, 0.8 * wmax, 0.3 * wmax, 0.95 * wmax, 0.6 * wmax]
                cmds = cmds[:len(dts)][::-1] if m else cmds[:len(dts)]
                motors.append(dict(type=base, motor=m, schedule=sched, dt_us=dts, cmd=_f32(cmds),
                                   min_speed=float(v["wmin"]), max_speed=wmax, k_thrust=op.k_thrust,
                                   k_torque=op.k_torque, time_const=v["tau"], inertia=v["J"],
                                   position=list(op.motor_pos[m]), rot_axis=list(op.motor_rot_axis[m]),
                                   clockwise=int(m == 0)))
    for c in motors:
        head = [c["clockwise"], c["min_speed"], c["max_speed"], c["k_thrust"], c["k_torque"], c["time_const"],
                c["inertia"]] + c["position"] + c["rot_axis"] + [len(c["dt_us"])]
        case("motor", "S " + _hex(head) + " " + " ".join("%d %s" % (d, float(x).hex()) for d, x in zip(c["dt_us"], c["cmd"])))

    out = subprocess.check_output([probe], input=("\n".join(lines) + "\n").encode()).decode().splitlines()
    assert len(out) == len(lines), (len(out), len(lines))
    res = {k: [] for k in ("rotvec", "step", "mul", "rotate", "euler", "to_euler", "imu_mount", "motor")}
    mi = 0
    for kind, line, o in zip(kinds, lines, out):
        o = json.loads(o)
        vals = [float.fromhex(t) for t in line.split()[1:]]
        if kind == "rotvec":
            res[kind].append(dict(r=vals, q=o["q"]))
        elif kind == "step":
            res[kind].append(dict(att=vals[:4], ang_vel=vals[4:7], dt=vals[7], q=o["q"]))
        elif kind == "mul":
            res[kind].append(dict(a=vals[:4], b=vals[4:], q=o["q"]))
        elif kind == "rotate":
            res[kind].append(dict(q=vals[:4], v=vals[4:], fwd=o["fwd"], inv=o["inv"]))
        elif kind == "euler":
            res[kind].append(dict(ypr=vals, q=o["q"]))
        elif kind == "to_euler":
            res[kind].append(dict(q=vals, ypr=o["ypr"], R=o["R"]))
        elif kind == "imu_mount":
            res[kind].append(dict(ypr=vals, R=o["R"]))
        else:
            c = dict(motors[mi])
            mi += 1
            c["speed"] = [s["speed"][0] for s in o["steps"]]
            for key in ("thrust", "torque", "ang_mom"):
                c[key] = [s[key] for s in o["steps"]]
            res[kind].append(c)
    res["generator"] = ("oracle/_ref/motion_probe (reference Rotation.hpp and Motor.{hpp,cpp} + ManualTimer.hpp compiled "
                        "in place, -ffp-contract=off, declaration-only <Eigen/Dense>)")
    res["min_angle"] = MIN_ANGLE
    return res


def main():
    from oracle import oracle_py
    oracle_py.build(force=True)
    ref = os.path.join(ROOT, "oracle", "_ref")
    timer = os.path.join(ref, "timer_probe")
    rng = os.path.join(ref, "rng_probe")

    cases = []
    for dt_s, per_s, n in TIMER_CASES:
        dt, per = eval(dt_s), eval(per_s)
        out = subprocess.check_output([timer, repr(dt), repr(per), str(n)])
        rec = json.loads(out)
        rec["loop_dt_expr"], rec["period_expr"] = dt_s, per_s
        cases.append(rec)
    with open(os.path.join(HERE, "timer_cadence.json"), "w") as f:
        json.dump({"generator": "oracle/_ref/timer_probe (reference Timer.hpp, ManualTimer.hpp, "
                                "CommunicationsDelay.hpp compiled in place)",
                   "cases": cases}, f, indent=0)

    kats = []
    for args in (["600"], ["60", "2"], ["60", "12345"], ["60", "2147483646"], ["60", "4097"]):
        rec = json.loads(subprocess.check_output([rng] + args))
        rec["seed"] = int(args[1]) if len(args) > 1 else 1
        kats.append(rec)
    with open(os.path.join(HERE, "rng_kat.json"), "w") as f:
        json.dump({"generator": "oracle/_ref/rng_probe (libstdc++ <random>, g++)",
                   "gxx": subprocess.check_output(["g++", "--version"]).decode().splitlines()[0],
                   "streams": kats}, f, indent=0)

    lpf = os.path.join(ref, "lpf_probe")
    lpfs = []
    for per, cut, n in ((1 / 500.0, 200.0, 200), (1 / 500.0, 100.0, 200), (1 / 1000.0, 200.0, 200)):
        lpfs.append(json.loads(subprocess.check_output([lpf, repr(per), repr(cut), str(n)])))
    with open(os.path.join(HERE, "lpf_kat.json"), "w") as f:
        json.dump({"generator": "oracle/_ref/lpf_probe (reference LowPassFilterSecondOrder.hpp compiled in place, "
                                "LowPassFilterSecondOrder<float,float>)", "cases": lpfs}, f, indent=0)

    tel = json.loads(subprocess.check_output([os.path.join(ref, "telemetry_probe"), "48", "20261002"]))
    tel["generator"] = ("oracle/_ref/telemetry_probe (reference TelemetryPacket.hpp compiled in place; "
                        "EncodeTelemetryPacket / DecodeTelemetryPacket)")
    with open(os.path.join(HERE, "telemetry_kat.json"), "w") as f:
        json.dump(tel, f, indent=0)

    pm = json.loads(subprocess.check_output([os.path.join(ref, "traj_probe"), "64", "20261002"]))
    pm["generator"] = ("oracle/_ref/traj_probe (reference RootFinder.hpp and SingleAxisTrajectory.{hpp,cpp} compiled in "
                       "place; libstdc++ mt19937 + uniform_real_distribution in the planner's call shape)")
    with open(os.path.join(HERE, "planner_math_kat.json"), "w") as f:
        json.dump(pm, f, indent=0)

    uwb = []
    for args in (["200", "0.05", "0.1", "3.0"], ["200", "0.0", "0.0", "0.0"], ["101", "0.25", "0.5", "10.0"]):
        uwb.append(json.loads(subprocess.check_output([os.path.join(ref, "uwb_probe")] + args)))
    with open(os.path.join(HERE, "uwb_kat.json"), "w") as f:
        json.dump({"generator": "oracle/_ref/uwb_probe (libstdc++ <random>, g++; call-site shape of UWBNetwork.cpp:66-71; "
                                "true range of transaction k = 1 + k/8 m)", "cases": uwb}, f, indent=0)

    motion = make_motion_kat(os.path.join(ref, "motion_probe"))
    with open(os.path.join(HERE, "motion_kat.json"), "w") as f:
        json.dump(motion, f, indent=0)

    # --- oracle regression vectors (oracle-generated; not a reference pin) ---
    from tests.scenarios import random_ensemble
    ens = random_ensemble(n=256, seed=20261002)
    b0 = ens.to_oracle_batch()
    b0.step(1e-3, 1, ticks=[1])
    b1 = ens.to_oracle_batch()
    ticks100 = np.zeros(100, np.uint8)
    ticks100[1::2] = 1
    b1.step(1e-3, 100, ticks=ticks100)
    np.savez_compressed(
        os.path.join(HERE, "oracle_regression.npz"),
        seed=20261002,
        s1_pos=b0.pos, s1_vel=b0.vel, s1_att=b0.att, s1_ang_vel=b0.ang_vel,
        s1_motor=b0.motor_speed, s1_gyro=b0.gyro, s1_acc=b0.acc, s1_rng=b0.rng,
        s100_pos=b1.pos, s100_vel=b1.vel, s100_att=b1.att, s100_ang_vel=b1.ang_vel,
        s100_motor=b1.motor_speed, s100_gyro=b1.gyro, s100_acc=b1.acc, s100_rng=b1.rng)
    print("fixtures written to", HERE)


if __name__ == "__main__":
    main()
