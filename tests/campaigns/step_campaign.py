"""Randomised campaign of the step kernel against the CPU oracle over the CONFIGURATION space (development tool;
tests/test_gpu_parity.py::test_configuration_campaign runs a short version): random type tables (mass, inertia,
motor lag, rotor inertia, CoM error, drag, IMU mount), 1..6 types laid out at random / type by type / all on
record 0 (the three ways a parameter record reaches the kernel), random dt and logic period, wrench arrays
on or off, IMU noise on or off under either seed policy, fused or single-step launches, ragged sizes, both
precisions.   python tests/campaigns/step_campaign.py [configurations] [seed]"""
import importlib, os, sys
import numpy as np
import torch  # noqa: F401
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
afa = importlib.import_module("agri-fly_amd")
from oracle import oracle_py as ora
from tests.scenarios import FLOORS, rel_err_vec

DTS_US = (100, 250, 500, 1000, 2000, 4000)
PERIODS = (1 / 1000, 1 / 500, 1 / 250, 1 / 100, 0.0033)


def random_table(rng, n_types):
    plist, olist = [], []
    for _ in range(n_types):
        p = afa.params_from_type(int(rng.choice([1, 2, 4, 5])))
        p.mass *= float(rng.uniform(0.8, 1.25))
        if rng.random() < 0.5:
            p.motor_time_const = float(rng.uniform(0.008, 0.06))
        if rng.random() < 0.4:
            p.motor_inertia = float(rng.uniform(1e-8, 2e-6))
        if rng.random() < 0.5:
            for k in range(3):
                p.com_error[k] = float(rng.normal(0, 1.5e-3))
        for k in range(3):
            p.lin_drag_coeff_b[k] = float(rng.uniform(0, 0.3)) if rng.random() < 0.7 else 0.0
        if rng.random() < 0.5:          # a full symmetric positive-definite inertia tensor
            A = rng.normal(size=(3, 3)) * 0.15
            I = np.array(p.inertia).reshape(3, 3)
            I = I + A @ A.T * I[0, 0]
            for a in range(9):
                p.inertia[a] = float(I.reshape(9)[a])
        p.imu_yaw, p.imu_pitch, p.imu_roll = [float(x) for x in rng.uniform(-0.6, 0.6, 3)]
        ablate = os.environ.get("STEP_CAMPAIGN_ABLATE", "")     # development: which parameter family drives an error
        if "jm" in ablate: p.motor_inertia = 0.0
        if "tau" in ablate: p.motor_time_const = 0.0
        if "com" in ablate:
            for k in range(3): p.com_error[k] = 0.0
        if "mount" in ablate: p.imu_yaw = p.imu_pitch = p.imu_roll = 0.0
        if "inertia" in ablate:
            q = afa.params_from_type(5)
            for a in range(9): p.inertia[a] = q.inertia[a]
        plist.append(p)
        olist.append(ora.params_init(p.mass, list(p.inertia), p.arm_length, list(p.com_error), p.motor_min_speed,
                                     p.motor_max_speed, p.prop_thrust_from_speed_sqr, p.prop_torque_from_speed_sqr,
                                     p.motor_time_const, p.motor_inertia, list(p.lin_drag_coeff_b),
                                     (p.imu_yaw, p.imu_pitch, p.imu_roll)))
    return plist, olist


def run_campaign(n_cfg=40, seed=1, verbose=True, only=None):
    master = np.random.default_rng(seed)
    worst = {"f32": {}, "f64": {}}
    for ci in range(n_cfg):
        rng = np.random.default_rng(master.integers(1 << 31))
        if only is not None and ci != only:
            continue
        n = int(rng.choice([1, 63, 64, 65, 1000, 2049, 4096, 5000]))
        n_types = int(rng.integers(1, 7))
        layout = str(rng.choice(["random", "by_type", "record0"]))
        plist, olist = random_table(rng, n_types)
        if layout == "random":
            types = rng.integers(0, n_types, n).astype(np.uint8)
        elif layout == "by_type":
            types = (np.arange(n) // 64 % n_types).astype(np.uint8)
        else:
            types = np.zeros(n, np.uint8)
        dt_us = int(rng.choice(DTS_US))
        period = float(rng.choice(PERIODS))
        steps = int(rng.integers(1, 41))
        use_force, use_torque = bool(rng.random() < 0.6), bool(rng.random() < 0.4)
        noise = bool(rng.random() < 0.6)
        policy = int(rng.choice([afa.AFE_SEED_REFERENCE, afa.AFE_SEED_DECORRELATED]))
        sg, sa = float(rng.uniform(0, 0.3)), float(rng.uniform(0, 0.5))
        fused = int(rng.choice([1, 1, 2, 7, 64]))
        first_global = int(rng.integers(0, 1 << 20))
        d = afa.scenarios.random_ensemble(n, int(rng.integers(1 << 30)), type_ids=(5,) * n_types)
        d.pos[2] += 40                                                    # room to fall for 40 x 4 ms
        wmax = np.array([p.motor_max_speed for p in plist])[types]
        cmd = (rng.uniform(0, 1.05, (4, n)) * wmax).astype(np.float32)   # a few above the clamp
        cmd[0, rng.random(n) < 0.02] = -50.0
        speed = rng.uniform(0, 1, (4, n)) * wmax
        for o in olist:
            o.sigma_gyro, o.sigma_acc = (sg, sa) if noise else (0.0, 0.0)
        ticks = afa.plan_ticks(period, 0, dt_us, steps)[0]
        # fp32 bound: BASELINE's 1e-5 for the reference's motor model (tau_m = J_m = 0, every shipped type).  With a
        # lagged rotor the speed itself is fp32 state: its rounding (6e-8 relative per step) enters the body
        # torque through DIFFERENCES of four nearly equal thrusts, and 30 steps of that reach 3e-5 in ang_vel /
        # the IMU sample (ablation: STEP_CAMPAIGN_ABLATE=tau removes it) -- a limit of fp32 storage, stated here.
        lagged = any(p.motor_time_const > 0 or p.motor_inertia > 0 for p in plist)
        for precision, tag, tol in ((afa.AFE_F64, "f64", 2e-11), (afa.AFE_F32, "f32", 5e-5 if lagged else 1e-5)):
            with afa.Ensemble(n, precision=precision, first_global_index=first_global) as e:
                if os.environ.get("STEP_CAMPAIGN_SPLIT"):            # the same campaign with the two halves on two streams
                    e.set_split_stepping(2)
                e.set_type_table(plist)
                e.set_vehicle_types(types)
                e.set_logic_period(period)
                e.set_imu_noise(noise, sg, sa, policy)
                e.set_max_fused_steps(fused)
                e.set_state(d.pos, d.vel, d.att, d.ang_vel, speed)
                e.set_motor_cmds(cmd)
                if use_force:
                    e.set_external_force(d.ext_force)
                if use_torque:
                    e.set_external_torque(d.ext_torque)
                rng0 = e.get_rng_state()
                if fused == 1 and steps > 1 and rng.random() < 0.5:
                    for _ in range(steps):
                        e.step(dt_us, 1)
                else:
                    e.step(dt_us, steps)
                st, (gyro, acc), rs, nt = e.get_state(), e.get_imu(), e.get_rng_state(), e.logic_ticks
            b = ora.Batch(n, olist, types)
            b.pos[:], b.vel[:], b.att[:], b.ang_vel[:], b.motor_speed[:] = d.pos, d.vel, d.att, d.ang_vel, speed
            b.motor_cmd[:] = cmd
            if use_force:
                b.ext_force[:] = d.ext_force
            if use_torque:
                b.ext_torque[:] = d.ext_torque
            b.rng[:] = rng0
            b.step(dt_us * 1e-6, steps, ticks=ticks)
            # vehicles the explicit integrator has blown up (tiny inertia x 4 ms steps: |w| reaches 1e44 rad/s in
            # both) are outside any tolerance statement: compared are those turning less than 0.5 rad per step at
            # the end, well inside the range the fp32 quaternion increment is proven for (afe_kernels.hip rotvec_to_quat:
            # 1e-6 up to pi rad per step, tests/test_gpu_attitude_domain.py); not widened: past it a vehicle is mid-blow-up
            with np.errstate(all="ignore"):
                sane = np.linalg.norm(b.ang_vel, axis=0) * dt_us * 1e-6 <= 0.5
            sane &= np.isfinite(b.pos).all(axis=0)
            errs = {k: rel_err_vec(st[k][..., sane], getattr(b, k)[..., sane], FLOORS[k])
                    for k in ("pos", "vel", "att", "ang_vel", "motor_speed")} if sane.any() else {"pos": 0.0}
            if ticks.any() and sane.any():
                errs["gyro"] = rel_err_vec(gyro[:, sane], b.gyro[:, sane], FLOORS["gyro"])
                errs["acc"] = rel_err_vec(acc[:, sane], b.acc[:, sane], FLOORS["acc"])
            worst[tag]["vehicles"] = worst[tag].get("vehicles", 0) + n
            worst[tag]["vehicles_blown_up"] = worst[tag].get("vehicles_blown_up", 0) + int(n - sane.sum())
            # engine noise switched off = no draws at all (the oracle, like the reference, always draws: sigma 0 there)
            rng_ok = (not noise or bool(np.array_equal(rs, b.rng))) and nt == int(ticks.sum())
            # the IMU sample is float arithmetic on float-narrowed inputs in every build (Quadcopter_T.cpp:165-180):
            # its bound is never below a float ulp (tests/test_gpu_parity.py _cmp_state)
            bad = [k for k, v in errs.items() if not v <= (max(tol, 1e-6) if k in ("gyro", "acc") else tol)] + \
                  ([] if rng_ok else ["rng/ticks"])
            for k, v in errs.items():
                worst[tag][k] = max(worst[tag].get(k, 0.0), v)
            if bad and only is not None:      # development: the worst vehicle of the first failing field
                k = bad[0] if bad[0] in st else "att"
                a_, b_ = np.atleast_2d(st[k]).astype(float), np.atleast_2d(getattr(b, k)).astype(float)
                w_ = int(np.nanargmax(np.linalg.norm(a_ - b_, axis=0)))
                print("   worst vehicle %d (type %d): engine %s = %s\n      oracle %s\n      ang_vel engine %s oracle %s |w| dt = %.3f rad\n      pos engine %s oracle %s"
                      % (w_, types[w_], k, a_[:, w_], b_[:, w_], st["ang_vel"][:, w_], b.ang_vel[:, w_],
                         np.linalg.norm(b.ang_vel[:, w_]) * dt_us * 1e-6, st["pos"][:, w_], b.pos[:, w_]))
            if verbose or bad:
                print("cfg %3d %s n=%5d types=%d/%-7s dt=%4dus period=%.4f steps=%2d fused=%2d F=%d T=%d noise=%d/%d  worst %-11s %.2e %s"
                      % (ci, tag, n, n_types, layout, dt_us, period, steps, fused, use_force, use_torque, noise, policy,
                         max(errs, key=errs.get), max(errs.values()), ("FAIL " + ",".join(bad)) if bad else ""), flush=True)
            worst[tag]["failures"] = worst[tag].get("failures", 0) + (1 if bad else 0)
            if tag == "f32":
                key = "worst_lagged_rotor" if lagged else "worst_reference_motor_model"
                worst[tag][key] = max(worst[tag].get(key, 0.0), max(errs.values()))
    return worst


def run_logic_campaign(n_cfg=30, seed=1, verbose=True):
    """The same idea with the loop closed on the device: onboard rates logic (KalmanFilter6DOF gyro path, low-pass,
    rates controller, mixer) against the oracle's restated logic, over vehicle-type mixes and layouts, dt, onboard
    period, noise, command magnitudes up to saturation, idle -> command -> partly re-commanded flights."""
    master = np.random.default_rng(seed)
    worst = {"f32": {"failures": 0}, "f64": {"failures": 0}}
    for ci in range(n_cfg):
        rng = np.random.default_rng(master.integers(1 << 31))
        n = int(rng.choice([1, 65, 300, 513]))
        ids = [int(t) for t in rng.permutation([5, 1, 2, 4])[:int(rng.integers(1, 5))]]
        layout = str(rng.choice(["random", "by_type"]))
        types = (rng.integers(0, len(ids), n) if layout == "random" else np.arange(n) // 64 % len(ids)).astype(np.uint8)
        dt_us = int(rng.choice([250, 500, 1000, 2000]))
        period = float(rng.choice([1 / 1000, 1 / 500, 1 / 250]))
        noise = bool(rng.random() < 0.7)
        policy = int(rng.choice([afa.AFE_SEED_REFERENCE, afa.AFE_SEED_DECORRELATED]))
        fused = int(rng.choice([1, 3, 64]))
        k0, k1, k2 = int(rng.integers(0, 8)), int(rng.integers(4, 30)), int(rng.integers(0, 25))
        d = afa.scenarios.random_ensemble(n, int(rng.integers(1 << 30)), type_ids=tuple(ids), ground_fraction=0.0)
        d.types = types
        d.pos[2] += 30
        d.ang_vel *= 0.3
        hover = np.array([afa.params_from_type(t).hover_speed for t in ids])[types]
        speed = hover * (1 + 0.05 * rng.uniform(-0.5, 0.5, (4, n)))
        thrust = np.clip(9.81 + rng.normal(0, 3.0, n), 0, 25).astype(np.float32)
        wdes = rng.normal(0, 2.0, (3, n)).astype(np.float32)
        thrust_b = np.clip(9.81 + rng.normal(0, 1.0, n), 0, 25).astype(np.float32)
        wdes_b = rng.normal(0, 0.5, (3, n)).astype(np.float32)
        half = n // 2
        steps = k0 + k1 + k2
        ticks = afa.plan_ticks(period, 0, dt_us, steps)[0]
        for precision, tag, tol in ((afa.AFE_F64, "f64", 1e-9), (afa.AFE_F32, "f32", 1e-5)):
            with afa.Ensemble(n, precision=precision) as e:
                if os.environ.get("STEP_CAMPAIGN_SPLIT"):
                    e.set_split_stepping(2)
                e.set_type_table([afa.params_from_type(t) for t in ids])
                e.set_vehicle_types(types)
                e.set_logic_period(period)
                e.set_imu_noise(noise, 0.1, 0.2, policy)
                e.set_max_fused_steps(fused)
                e.set_state(d.pos, d.vel, d.att, d.ang_vel, speed)
                e.set_motor_cmds(np.zeros((4, n), np.float32))
                e.set_external_force(d.ext_force)
                e.set_rates_logic([afa.rates_logic_params_from_type(t) for t in ids])
                rng0 = e.get_rng_state()
                if k0:
                    e.step(dt_us, k0)
                e.set_rates_commands(thrust, wdes)
                e.step(dt_us, k1)
                if k2:
                    if half:
                        e.set_rates_commands(thrust_b[:half], wdes_b[:, :half], first=0, count=half)
                    e.step(dt_us, k2)
                st, cmds, rs = e.get_state(), e.get_motor_cmds(), e.get_rng_state()
            olist = [ora.params_from_type(t) for t in ids]
            for o in olist:
                if not noise:
                    o.sigma_gyro = o.sigma_acc = 0.0
                else:
                    o.sigma_gyro, o.sigma_acc = 0.1, 0.2
            b = ora.Batch(n, olist, types)
            b.pos[:], b.vel[:], b.att[:], b.ang_vel[:], b.motor_speed[:] = d.pos, d.vel, d.att, d.ang_vel, speed
            b.ext_force[:] = d.ext_force
            b.rng[:] = rng0
            cl = ora.ClosedLoopBatch(b, [ora.logic_params_from_type(t, period) for t in ids], period)
            cl.step(dt_us * 1e-6, ticks[:k0])
            cl.set_rates_cmd(thrust, wdes)
            cl.step(dt_us * 1e-6, ticks[k0:k0 + k1])
            if k2:
                if half:
                    t2, w2 = thrust.copy(), wdes.copy()
                    t2[:half], w2[:, :half] = thrust_b[:half], wdes_b[:, :half]
                    cl.set_rates_cmd(t2, w2)
                cl.step(dt_us * 1e-6, ticks[k0 + k1:])
            errs = {k: rel_err_vec(st[k], getattr(b, k), FLOORS[k]) for k in ("pos", "vel", "att", "ang_vel", "motor_speed")}
            errs["motor_cmd"] = rel_err_vec(cmds, b.motor_cmd, 1.0)
            rng_ok = not noise or bool(np.array_equal(rs, b.rng))
            bad = [k for k, v in errs.items() if not v <= (max(tol, 1e-6) if k == "motor_cmd" else tol)] + ([] if rng_ok else ["rng"])
            for k, v in errs.items():
                worst[tag][k] = max(worst[tag].get(k, 0.0), v)
            worst[tag]["failures"] += 1 if bad else 0
            if verbose or bad:
                print("logic cfg %3d %s n=%4d types=%s/%-7s dt=%4dus period=%.4f steps=%d+%d+%d fused=%2d noise=%d/%d  worst %-11s %.2e %s"
                      % (ci, tag, n, ids, layout, dt_us, period, k0, k1, k2, fused, noise, policy, max(errs, key=errs.get),
                         max(errs.values()), ("FAIL " + ",".join(bad)) if bad else ""), flush=True)
    return worst


if __name__ == "__main__":
    w = run_campaign(int(sys.argv[1]) if len(sys.argv) > 1 else 40, int(sys.argv[2]) if len(sys.argv) > 2 else 1,
                     only=int(sys.argv[3]) if len(sys.argv) > 3 else None)
    print(w)
    if len(sys.argv) <= 3:
        wl = run_logic_campaign(max(4, (int(sys.argv[1]) if len(sys.argv) > 1 else 40) // 4), int(sys.argv[2]) if len(sys.argv) > 2 else 1)
        print(wl)
        w["f32"]["failures"] += wl["f32"]["failures"] + wl["f64"]["failures"]
    sys.exit(1 if w["f32"]["failures"] or w["f64"]["failures"] else 0)
