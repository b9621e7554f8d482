"""The step kernel's attitude increment over its whole domain, and its rotor model, against the reference's own
Rotation<double> and Motor (tests/golden/motion_kat.json, printed by oracle/_ref/motion_probe; the CPU pin of the same
fixture is tests/test_motion_oracle.py).  Needs an MI355X: run with -m gpu.

The random ensembles of the parity suite turn about 0.002 rad per step, so they judge only the series branch of the
fp32 increment (afe_kernels.hip rotvec_to_quat); here every vehicle turns by a chosen angle, from below the
reference's one-arc-second identity threshold to 1000 rad per step, and the spin tests run 50 such steps.
"""
import json
import os

import numpy as np
import pytest

from tests.scenarios import FLOORS, afa, record_parity, rel_err_vec

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "motion_kat.json")
PRECISIONS = [afa.AFE_F64, afa.AFE_F32]


def _kat():
    with open(GOLDEN) as f:
        return json.load(f)


def _still_engine(precision, n, plist, types=None):
    """n vehicles high above the ground with stopped rotors, no command, no external wrench, noise-free IMU: one step
    moves the attitude by FromRotationVector(angVel * dt) of the pre-step rates alone (Quadcopter_T.cpp:142)"""
    e = afa.Ensemble(n, precision=precision)
    e.set_type_table(plist)
    e.set_vehicle_types(np.zeros(n, np.uint8) if types is None else types)
    e.set_imu_noise(False)
    e.set_motor_cmds(np.zeros((4, n), np.float32))
    e.set_external_force(np.zeros((3, n)))
    e.set_external_torque(np.zeros((3, n)))
    return e


def _state_in(e, precision, att, ang_vel):
    n = att.shape[1]
    pos = np.zeros((3, n))
    pos[2] = 1000.0
    dt = np.float64 if precision == afa.AFE_F64 else np.float32
    e.set_state(pos, np.zeros((3, n)), att, ang_vel, np.zeros((4, n)))
    back = e.get_state(dtype=dt)
    # the fixture's attitudes and rates are float32 values: both engines must hold them unchanged
    np.testing.assert_array_equal(back["att"], att.astype(dt))
    np.testing.assert_array_equal(back["ang_vel"], ang_vel.astype(dt))


# C1 bounds, max |engine - reference| per quaternion component.  fp64: the reference's formula with the device's
# sin / cos.  fp32 up to pi rad per step: the series and <= 3 squarings; to 100 rad: <= 8 squarings, each roughly
# doubling the error, inside the general 1e-5; past 100 rad the fp32 increment makes no accuracy claim (a unit
# quaternion, nothing more).
F64_BOUND = 1e-14
F32_BOUNDS = ((np.pi, 1e-6), (100.0, 1e-5))
BAND = 1e-6    # |theta / MIN_ANGLE - 1| inside which fp32 rounding of theta^2 may take either branch


def _f32_bound(theta):
    for top, b in F32_BOUNDS:
        if theta <= top:
            return b
    return None


@pytest.mark.parametrize("dt_us", [1000, 4000])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_step_increment_over_the_whole_domain(precision, dt_us):
    kat = _kat()
    min_angle = kat["min_angle"]
    cases = [c for c in kat["step"] if c["dt"] == dt_us * 1e-6]
    n = len(cases)
    assert n % 64 != 0 and n > 64   # ragged: the last wave is partly empty
    att = np.array([c["att"] for c in cases]).T
    w = np.array([c["ang_vel"] for c in cases]).T
    ref = np.array([c["q"] for c in cases]).T
    theta = np.linalg.norm(w * (dt_us * 1e-6), axis=0)
    with _still_engine(precision, n, [afa.params_from_type(5)]) as e:
        _state_in(e, precision, att, w)
        e.step(dt_us, 1)
        q = e.get_state()["att"]
    assert np.isfinite(q).all()
    err = np.max(np.abs(q - ref), axis=0)
    tag = "attitude increment dt=%dus" % dt_us
    if precision == afa.AFE_F64:
        for sel, what in ((theta <= 100, "theta<=100"), (theta > 100, "theta>100")):
            record_parity("%s %s" % (tag, what), precision, "att", q[:, sel], ref[:, sel])
        # the reference's own test on the same double theta: the identity branch is taken exactly where it takes it
        ident = theta < min_angle
        np.testing.assert_array_equal(q[:, ident], ref[:, ident])
        bad = (theta <= 100) & ~(err <= F64_BOUND)
        assert not bad.any(), list(zip(theta[bad], err[bad]))
        bad = (theta > 100) & ~(err <= 1e-12)
        assert not bad.any(), list(zip(theta[bad], err[bad]))
        return
    band = np.abs(theta / min_angle - 1) <= BAND
    below = (theta < min_angle) & ~band
    # outside the band the reference's branch: below it the exact identity increment (att, renormalised: <= 2 ulp),
    # above it the general branch, whose first 1e-6 bound is less than half of the theta/2 an identity step would miss
    assert (err[below] <= 2.4e-7).all(), list(zip(theta[below], err[below]))
    assert (err[band] <= theta[band] / 2 + 1e-7).all(), list(zip(theta[band], err[band]))
    gen = ~band & ~below
    for (lo, hi), what in (((0, np.pi), "theta<=pi"), ((np.pi, 100.0), "pi<theta<=100"), ((100.0, np.inf), "theta>100")):
        sel = gen & (theta > lo) & (theta <= hi)
        assert sel.any()
        record_parity("%s %s" % (tag, what), precision, "att", q[:, sel], ref[:, sel])
    over = np.array([_f32_bound(t) is not None and err[i] > _f32_bound(t) for i, t in enumerate(theta)]) & gen
    assert not over.any(), ["theta %.9g err %.3g bound %g" % (theta[i], err[i], _f32_bound(theta[i])) for i in np.where(over)[0]]
    far = gen & (theta > 100)
    assert (np.abs(np.linalg.norm(q[:, far], axis=0) - 1) <= 1e-6).all()


SPIN_THETAS = (0.05, 0.3, 0.6, 1.5, 3.0)
# body axes only: about a skew axis in the x-y plane w x I w is zero in exact arithmetic but not in floating point (the
# two products round differently), and the explicit integrator amplifies that seed by sqrt(1 + theta^2) per step
SPIN_AXES = ((1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0))
N_SPIN = 50


@pytest.mark.parametrize("precision", PRECISIONS)
def test_steady_spin_matches_its_closed_form(precision):
    """A body spinning about its x, y or z axis keeps its rate (every shipped type has I_xx = I_yy, so
    w x I w = 0, and stopped rotors add no momentum), so after N steps the attitude is att0 * exp(N w dt / 2), in
    closed form.  Bound: N x the one-step bound at that angle (fp64 1e-14; fp32 1e-6 up to pi rad per step), plus
    N 2^-24 for the fp32 storage of every intermediate attitude.  The fp32 kernel renormalises every step, so its
    |q| - 1 must stay within 4 ulp however large N is -- the check that catches a lost renormalisation (the attitude
    bound is too wide to); the fp64 kernel, like the reference, does not renormalise and may drift by one rounding per
    step.  The noise-free gyro is the rate itself; the accelerometer is att^-1 (acc + g) of the oracle's step."""
    from oracle import oracle_py
    rng = np.random.default_rng(50)
    dt_us, dt = 1000, 1e-3
    axes = np.array(SPIN_AXES) / np.linalg.norm(SPIN_AXES, axis=1)[:, None]
    w = np.float32(np.concatenate([th / dt * axes for th in SPIN_THETAS]).T).astype(np.float64)
    n = w.shape[1]
    att0 = rng.standard_normal((4, n))
    att0 = np.float32(att0 / np.linalg.norm(att0, axis=0)).astype(np.float64)
    # closed form: att0 * (cos(N theta / 2), sin(N theta / 2) w / |w|), Rotation.hpp:124-131's product in double
    theta = np.linalg.norm(w * dt, axis=0)
    half = N_SPIN * theta / 2
    ex = np.vstack([np.cos(half), np.sin(half) * w / np.linalg.norm(w, axis=0)])
    a, r1 = att0, ex
    ref = np.vstack([r1[0] * a[0] - r1[1] * a[1] - r1[2] * a[2] - r1[3] * a[3],
                     r1[1] * a[0] + r1[0] * a[1] + r1[3] * a[2] - r1[2] * a[3],
                     r1[2] * a[0] - r1[3] * a[1] + r1[0] * a[2] + r1[1] * a[3],
                     r1[3] * a[0] + r1[2] * a[1] - r1[1] * a[2] + r1[0] * a[3]])

    t = 2   # a drag-carrying type (CF_BIGMOTORSPROPS): the accelerometer then reads more than zero
    ticks = afa.plan_ticks(1 / 500, 0, dt_us, N_SPIN)[0]
    with _still_engine(precision, n, [afa.params_from_type(t)]) as e:
        e.set_logic_period(1 / 500)
        _state_in(e, precision, att0, w)
        e.step(dt_us, N_SPIN)
        st = e.get_state()
        gyro, acc = e.get_imu()
    p = oracle_py.params_from_type(t)
    p.sigma_acc = p.sigma_gyro = 0.0     # the engine's noise is off
    b = oracle_py.Batch(n, [p])
    b.pos[2] = 1000.0
    b.att[:], b.ang_vel[:] = att0, w
    b.step(dt, N_SPIN, ticks=ticks)

    np.testing.assert_array_equal(st["ang_vel"], w)   # w x I w == 0 exactly: the rate never changes
    q = st["att"]
    err = np.max(np.abs(q - ref), axis=0)
    f32 = precision == afa.AFE_F32
    bound = np.array([N_SPIN * (_f32_bound(x) + 2.0 ** -24) if f32 else N_SPIN * F64_BOUND for x in theta])
    for th in SPIN_THETAS:
        sel = np.abs(theta - th) < 1e-6
        record_parity("steady spin %d steps at %g rad/step" % (N_SPIN, th), precision, "att", q[:, sel], ref[:, sel])
    assert (err <= bound).all(), ["theta %.3g err %.3g bound %.3g" % v for v in zip(theta, err, bound) if v[1] > v[2]]
    norm = np.linalg.norm(q, axis=0)
    if f32:
        assert np.max(np.abs(norm - 1)) <= 4 * 2.0 ** -23, np.max(np.abs(norm - 1))
    else:
        assert np.max(np.abs(norm - np.linalg.norm(att0, axis=0))) <= N_SPIN * 2.0 ** -52

    np.testing.assert_array_equal(gyro, np.float32(w))     # identity IMU mount, no noise: the body rate itself
    np.testing.assert_array_equal(b.gyro, np.float32(w))
    # the accelerometer rotates the proper acceleration by the attitude: an attitude error e moves it by <= 2 e |a|
    acc_err = rel_err_vec(acc, b.acc, FLOORS["acc"])
    record_parity("steady spin %d steps (IMU)" % N_SPIN, precision, "acc", acc, b.acc)
    assert np.abs(b.acc).max() > 1e-2
    assert acc_err <= (2 * bound.max() + 1e-6 if f32 else 1e-6), acc_err


@pytest.mark.parametrize("precision", PRECISIONS)
def test_motor_sequences_match_the_reference_motor(precision):
    """The fixture's rotor sequences (Motor.cpp: negative, zero, mid-range and above-maximum commands, a nonzero
    minimum speed, tau = J = 0 and lagged rotors, 1 ms / 4 ms steps and dt < 1 us early returns) through the engine:
    one vehicle per case, its own type-table row, the command set before every step.  fp64 <= 1e-13 relative; fp32
    within the parity tolerance at the rotor-speed floor."""
    kat = _kat()
    tol = 1e-13 if precision == afa.AFE_F64 else 1e-5
    for sched in ("1ms", "4ms", "mixed"):
        cases = [c for c in kat["motor"] if c["schedule"] == sched]
        n = len(cases)
        plist = []
        for c in cases:
            p = afa.params_from_type(c["type"])
            p.motor_min_speed, p.motor_max_speed = c["min_speed"], c["max_speed"]
            p.prop_thrust_from_speed_sqr, p.prop_torque_from_speed_sqr = c["k_thrust"], c["k_torque"]
            p.motor_time_const, p.motor_inertia = c["time_const"], c["inertia"]
            plist.append(p)
        with _still_engine(precision, n, plist, types=np.arange(n, dtype=np.uint8)) as e:
            pos = np.zeros((3, n))
            pos[2] = 1000.0
            att = np.zeros((4, n))
            att[0] = 1.0
            e.set_state(pos, np.zeros((3, n)), att, np.zeros((3, n)), np.zeros((4, n)))
            got = []
            for k, dt_us in enumerate(cases[0]["dt_us"]):
                assert all(c["dt_us"][k] == dt_us for c in cases)
                e.set_motor_cmds(np.tile(np.float32([c["cmd"][k] for c in cases]), (4, 1)))
                e.step(dt_us, 1)
                got.append(e.get_state()["motor_speed"])
        for k in range(len(got)):
            ref = np.tile([c["speed"][k] for c in cases], (4, 1))
            # fp64: relative to the speed itself (a stopped rotor must read exactly 0); fp32: at the parity floor
            floor = FLOORS["motor_speed"] if precision == afa.AFE_F32 else 1e-300
            worst = np.max(np.abs(got[k] - ref) / np.maximum(np.abs(ref), floor))
            record_parity("reference motor sequences %s step %d" % (sched, k), precision, "motor_speed", got[k], ref)
            assert worst <= tol, (sched, k, worst, got[k][0], ref[0])
