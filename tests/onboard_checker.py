"""The onboard flight computer's specification in numpy for N vehicles: tests/onboard_reference.py (the scalar, line by line
restatement of Onboard::QuadcopterLogic::Run and the complementary branch of KalmanFilter6DOF::Predict) vectorised, bit for bit
the same; agri-fly_amd/csrc/afe_onboard.hip states the same operations for the device.  Arrays are planar: [components, n].

  math(op, x, x2)  op 0..3 = sinf, cosf, acosf, asinf; 4 = atan2f(x, x2) (float32): device_math asks the GPU
                   (afe_onboard_selftest_math), glibc_math libm through ctypes, numpy_math numpy
  BRANCHES         every branch of the definition, with the dead ones marked; Onboard.tick counts who took which in .count
                   (the scripted flight that reaches every live one is tests/onboard_flight.py's)

PINNED PARTS: the second-order low-pass is tests/gps_imu_reference.py's (held to the oracle library's ora_lpf2_* in
tests/test_onboard_cpu.py), the quaternion functions are tests/follower_checker.py's and the attitude controller is
tests/stages_checker.desired_angular_velocity (both pinned through tests/golden/offboard_reference.npz); the command of the rates
state is held to ora_logic_tick and the telemetry bytes to afe_telemetry_encode.

PINNED AS A WHOLE to the reference's own class: oracle/_ref/onboard_probe (QuadcopterLogic.cpp and KalmanFilter6DOF.cpp compiled
where they lie against oracle/eigen_trap) flies the script of tests/onboard_flight.py call for call, and under glibc_math every
field of every vehicle after every tick and every telemetry byte of this file equals it bit for bit
(tests/golden/make_onboard_reference.py asserts it, tests/test_onboard_reference.py holds this file to the recording).  Still
open: the branch behind _UWBInitialized, RunControllerFullyAutonomous, TestMotors, the calibrations (none is stated here)."""
import ctypes as _C
import ctypes.util as _Cu

import numpy as np

from tests import follower_checker as fc
from tests import gps_imu_reference as gref
from tests import stages_checker as sc
from tests.follower_checker import m_rotate, q_inv, q_matrix, q_mul, same_bits, v_cross, v_dot  # noqa: F401

D, F = np.float64, np.float32
UNINIT, IDLE, AUTONOMOUS, PANIC, KILLED, ACCELERATION, RATES = range(7)
NO_PANIC, ESTIMATE_CRAZY, UWB_TIMEOUT, UPSIDE_DOWN, RADIO_TIMEOUT, LOW_BATTERY, KILLED_INTERNALLY, KILLED_EXTERNALLY = range(8)
WARN_LOW_BATT, WARN_CMD_RATE, WARN_UWB_RESET, WARN_ONBOARD_FREQ, WARN_CMD_BATCH_DROP = 0x01, 0x02, 0x04, 0x08, 0x10
MSG_KILL, MSG_POSITION, MSG_ACCELERATION, MSG_RATES, MSG_IDLE = 2, 3, 4, 5, 6
FLAG_DISABLE_CHECKS = 0x02
PI_F = F(np.pi)

_libm = _C.CDLL(_Cu.find_library("m") or "libm.so.6")
for _n in ("sinf", "cosf", "acosf", "asinf"):
    getattr(_libm, _n).restype = _C.c_float
    getattr(_libm, _n).argtypes = [_C.c_float]
_libm.expf.restype = _C.c_float
_libm.expf.argtypes = [_C.c_float]
_libm.atan2f.restype = _C.c_float
_libm.atan2f.argtypes = [_C.c_float, _C.c_float]
_NAMES = ("sinf", "cosf", "acosf", "asinf", "atan2f")


def glibc_math(op, x, x2=None):
    x = np.asarray(x, F)
    f = getattr(_libm, _NAMES[op])
    if op == 4:
        x2 = np.broadcast_to(np.asarray(x2, F), x.shape)
        return np.array([f(float(a), float(b)) for a, b in zip(x.reshape(-1), x2.reshape(-1))], F).reshape(x.shape)
    return np.array([f(float(v)) for v in x.reshape(-1)], F).reshape(x.shape)


def numpy_math(op, x, x2=None):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        if op == 4:
            return np.arctan2(x, np.asarray(x2, F)).astype(F)
        return (np.sin, np.cos, np.arccos, np.arcsin)[op](x).astype(F)


def device_math(afa, device=-1):
    def math(op, x, x2=None):
        x = np.asarray(x, F)
        if op == 4:
            x2 = np.ascontiguousarray(np.broadcast_to(np.asarray(x2, F), x.shape))
        return afa.onboard_selftest_math(op, x, x2, device=device).reshape(x.shape)
    return math


def _fm(math):
    """tests/follower_checker.py numbers sinf, cosf, asinf, acosf from 0"""
    return lambda op, x: math((0, 1, 3, 2)[op], x)


def _stages_math(math):
    """tests/stages_checker.py numbers them from 2"""
    return lambda op, x: math((0, 1, 3, 2)[op - 2], x)


def default_config(threshold=6.0):
    """afe_onboard_default_config(5) without the library (MINIQUAD: two cells)"""
    av_xy = F(0.04)
    two_pi = F(2 * np.pi)
    return dict(accel_cutoff=F(100.0), batt_cutoff=F(0.5) * two_pi, temp_cutoff=F(0.5) * two_pi, main_cutoff=F(50.0), cmd_cutoff=F(1.0),
                tc_xy=av_xy * F(2), tc_z=(av_xy * F(5)) * F(2), threshold=F(threshold), radio_period=F(0.02))


def config_from(cfg):
    """an OnboardConfig of the package -> the dict the class below takes"""
    return dict(accel_cutoff=F(cfg.accel_lowpass_cutoff), batt_cutoff=F(cfg.batt_lowpass_cutoff), temp_cutoff=F(cfg.temp_lowpass_cutoff),
                main_cutoff=F(cfg.main_loop_monitor_cutoff), cmd_cutoff=F(cfg.cmd_rate_monitor_cutoff), tc_xy=F(cfg.att_time_const_xy),
                tc_z=F(cfg.att_time_const_z), threshold=F(cfg.low_battery_threshold), radio_period=F(cfg.radio_cmd_period))


def logic_record(p):
    """an afe_rates_logic_params (RatesLogicParams of the package) -> the constants the mixer and the rate controller use, as
    afe_params.cpp expand_logic derives them (QuadcopterMixer::SetParameters, QuadcopterMixer.hpp:36-52)"""
    max_thrust = F(p.max_thrust_per_propeller)
    return dict(mass=F(p.mass), I=np.array(list(p.inertia), F), tc_xy=F(p.ang_vel_time_const_xy), tc_z=F(p.ang_vel_time_const_z),
                d=F(p.arm_length) / np.sqrt(F(2.0)), kt=F(p.prop0_spin_dir) * F(p.prop_torque_from_thrust), kf=F(p.prop_thrust_from_speed_sqr),
                max_thrust=max_thrust, min_thrust=F(p.min_thrust_per_propeller),
                max_cmd_total=F(4) * max_thrust * F(0.8) if p.max_cmd_total_thrust < 0 else F(p.max_cmd_total_thrust),
                mount=(p.imu_yaw, p.imu_pitch, p.imu_roll), gyro_cutoff=F(p.gyro_lowpass_cutoff))


# name -> live?  (a dead branch is one no input can take; the reason stands beside it)
BRANCHES = {
    # the radio
    "msg_new": True, "msg_waits": True, "msg_ignored_panic": True, "msg_ignored_killed": True, "msg_kill": True, "msg_kill_first_reason": True,
    "msg_kill_reason_kept": False,   # a kill is ignored in PANIC, and PANIC is the only other way to a reason
    "msg_acceleration": True, "msg_rates": True, "msg_idle": True,
    "msg_position": False,           # afe_onboard_radio refuses the type: FS_FULLY_AUTONOMOUS is not built
    # Predict
    "kf_init": True, "kf_predict": True, "acos_gt_1": True, "acos_lt_m1": True, "acos_in_domain": True, "axis_small": True, "axis_normalised": True,
    "rotvec_small": True,
    # warnings
    "warn_low_batt": True, "warn_cmd_rate": True, "warn_batch_drop": True, "warn_onboard_freq": True, "warn_reset": True,
    # panic
    "motors_not_running": True, "not_critical": True, "panic_upside_down": True, "panic_radio": True, "panic_battery": True,
    "upside_down_suppressed": True, "ovr_radio_over_upside_down": True, "ovr_battery_over_radio": True, "already_panic": False,
    "panic_estimate_crazy": False,   # no UWB: the estimated z stays 0
    "panic_uwb_timeout": False,      # needs FS_FULLY_AUTONOMOUS
    # the controller
    "ctl_rates": True, "ctl_zero": True, "acc_cutoff": True, "acc_identity": True, "acc_general": True,
}
# already_panic: CheckPanicReasons runs for PANIC too but AreInSafetyCriticalFlightState() is false there


def lp2_apply(k, state, x):
    """LowPassFilterSecondOrder::Apply, :51-64; k = (a1, a2, b0, b1, b2) (scalars or [n]), state = [xm0, xm1, ym0, ym1] arrays like x"""
    a1, a2, b0, b1, b2 = k
    x = np.array(x, F)                       # (a copy: it is kept as xm1)
    out = b2 * x
    out = out + (+b0 * state[0] + b1 * state[1])
    out = out + (-a1 * state[2] - a2 * state[3])
    state[0], state[1] = state[1], x
    state[2], state[3] = state[3], out
    assert out.dtype == F
    return out


def lp1_coefficient(period, cutoff):
    """LowPassFilterFirstOrder<float, float>::Initialise, :31: exp of a float product -- the float overload in C++, libm's expf
    (the host computes it once per type record; for 0.002 x 50 and 0.02 x 1 the double exp narrowed is the same float)"""
    return F(_libm.expf(float(-F(period) * F(cutoff))))


def seconds_f(now_us, reset_us):
    """Timer::GetSeconds<float>: float(uint64 difference) * 1e-6f"""
    return (np.asarray(now_us, np.uint64) - reset_us).astype(F) * F(1e-6)


def guarded_acos(c, math, count=None):
    """errno after acosf: |c| > 1 -> c < 0 ? pi : 0; a NaN passes through"""
    c = np.asarray(c, F)
    with np.errstate(all="ignore"):
        hi, lo = c > F(1), c < F(-1)
        inner = math(2, np.where(hi | lo, F(0), c).astype(F))
    if count is not None:
        count["acos_gt_1"] += int(hi.sum())
        count["acos_lt_m1"] += int(lo.sum())
        count["acos_in_domain"] += int((~hi & ~lo).sum())
    return np.where(hi, F(0), np.where(lo, PI_F, inner)).astype(F)


def from_axis_angle(u, angle, math):
    """Rotation.hpp:92-97"""
    half = (angle * F(0.5)).astype(F)
    s, c = math(0, half), math(1, half)
    return np.stack([c, s * u[0], s * u[1], s * u[2]]).astype(F)


def from_euler_ypr(y, p, r, math):
    """Rotation.hpp:99-110"""
    h = F(0.5)
    sy, cy, sp, cp, sr, cr = math(0, h * y), math(1, h * y), math(0, h * p), math(1, h * p), math(0, h * r), math(1, h * r)
    return np.stack([cy * cp * cr + sy * sp * sr, cy * cp * sr - sy * sp * cr, cy * sp * cr + sy * cp * sr, sy * cp * cr - cy * sp * sr]).astype(F)


def to_euler_ypr(q, math):
    """Rotation.hpp:163-169"""
    two = F(2.0)
    y = math(4, two * q[1] * q[2] + two * q[0] * q[3], q[1] * q[1] + q[0] * q[0] - q[3] * q[3] - q[2] * q[2])
    p = -math(3, two * q[1] * q[3] - two * q[0] * q[2])
    r = math(4, two * q[2] * q[3] + two * q[0] * q[1], q[3] * q[3] - q[2] * q[2] - q[1] * q[1] + q[0] * q[0])
    return y.astype(F), p.astype(F), r.astype(F)


def gravity_axis_angle(att, acc, math, count=None, who=None):
    """KalmanFilter6DOF.cpp:83-103 and :121-141 -> (axis [3, n], angle [n])"""
    n = att.shape[1]
    e3 = np.zeros((3, n), F)
    e3[2] = 1
    with np.errstate(all="ignore"):
        exp_acc = m_rotate(q_matrix(q_inv(att)), e3).astype(F)
        na = np.sqrt(v_dot(acc, acc)).astype(F)
        u = (acc / na).astype(F)
        c = v_dot(exp_acc, u).astype(F)
        ax = v_cross(u, exp_acc).astype(F)
        nr = np.sqrt(v_dot(ax, ax)).astype(F)
        big = nr > F(1e-6)
        ax = np.where(big, ax / np.where(big, nr, F(1)), np.array([[1], [0], [0]], F)).astype(F)
    angle = guarded_acos(c, math)
    if count is not None:
        who = np.ones(n, bool) if who is None else who
        count["axis_small"] += int((~big & who).sum())
        count["axis_normalised"] += int((big & who).sum())
        count["acos_gt_1"] += int(((c > F(1)) & who).sum())
        count["acos_lt_m1"] += int(((c < F(-1)) & who).sum())
        count["acos_in_domain"] += int((~(c > F(1)) & ~(c < F(-1)) & who).sum())
    return ax, angle


def motors_from_rates(L, thrust_norm, wdes, w):
    """GetDesiredTorques (QuadcopterAngularVelocityController.hpp:25-38), GetMotorForces and PropellerSpeedsFromThrust
    (QuadcopterMixer.hpp:63-99) as rates_logic_tick states them -> (forces [4, n], speeds [4, n]); L: per-vehicle constants"""
    with np.errstate(all="ignore"):
        e = (wdes - w).astype(F)
        aa = np.stack([e[0] / L["tc_xy"], e[1] / L["tc_xy"], e[2] / L["tc_z"]]).astype(F)
        I = L["I"]
        mv = lambda v: np.stack([((F(0) + I[3 * i] * v[0]) + I[3 * i + 1] * v[1]) + I[3 * i + 2] * v[2] for i in range(3)]).astype(F)  # noqa: E731
        Iw, Ia = mv(w), mv(aa)
        tx = Ia[0] + (w[1] * Iw[2] - w[2] * Iw[1])
        ty = Ia[1] + (w[2] * Iw[0] - w[0] * Iw[2])
        tz = Ia[2] + (w[0] * Iw[1] - w[1] * Iw[0])
        tot = (thrust_norm * L["mass"]).astype(F)
        des = np.where(tot > L["max_cmd_total"], L["max_cmd_total"], tot).astype(F)
        d, kt = L["d"], L["kt"]
        f = np.stack([(-tx / d - ty / d - tz / kt + des) / F(4), (-tx / d + ty / d + tz / kt + des) / F(4),
                      (+tx / d + ty / d - tz / kt + des) / F(4), (+tx / d - ty / d + tz / kt + des) / F(4)]).astype(F)
        f = np.where(f < L["min_thrust"], L["min_thrust"], np.where(f > L["max_thrust"], L["max_thrust"], f)).astype(F)
        speed = np.where(f <= 0, F(0), np.sqrt(np.where(f <= 0, F(1), f) / (F(1) * L["kf"]))).astype(F)
    return f, speed


def telemetry_code(x, a, b):
    """EncodeOnesRange(MapToOnesRange(x, a, b)), TelemetryPacket.hpp:38-60 -> uint16; a NaN is code 0"""
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        t = ((x - F(a)) / (F(b) - F(a))) * F(2) - F(1)
        bad = np.isnan(t) | (t < -1) | (t > 1)
        return np.where(bad, 0, (F(32768) + F(32767) * np.where(bad, F(0), t)).astype(np.int64)).astype(np.uint16)


class Onboard:
    """n vehicles' QuadcopterLogic without UWB.  types [n] indexes logic (list of logic_record) and cfgs (list of default_config /
    config_from dicts).  The rates command and have_cmd of the engine are kept here too: deliver() is every way a command arrives."""

    def __init__(self, n, period, types, logic, cfgs, t0_us=0, math=glibc_math):
        self.n, self.math, self.period = n, math, F(period)
        ty = np.asarray(types, int)
        pick = lambda rows: np.array(rows)[ty]                        # noqa: E731
        self.L = dict(mass=pick([r["mass"] for r in logic]), I=np.stack([r["I"] for r in logic])[ty].T.copy(), tc_xy=pick([r["tc_xy"] for r in logic]),
                      tc_z=pick([r["tc_z"] for r in logic]), d=pick([r["d"] for r in logic]), kt=pick([r["kt"] for r in logic]),
                      kf=pick([r["kf"] for r in logic]), max_thrust=pick([r["max_thrust"] for r in logic]),
                      min_thrust=pick([r["min_thrust"] for r in logic]), max_cmd_total=pick([r["max_cmd_total"] for r in logic]))
        self.R = np.stack([gref.mount_matrix(*r["mount"]) for r in logic])[ty]
        coeff = lambda cut: tuple(np.array(c, F) for c in zip(*[gref.lowpass_coefficients(period, c[cut]) for c in cfgs]))   # noqa: E731
        self.k_gyro = tuple(np.array(c, F)[ty] for c in zip(*[gref.lowpass_coefficients(period, r["gyro_cutoff"]) for r in logic]))
        self.k_acc, self.k_batt, self.k_temp = (tuple(c[ty] for c in coeff(cut)) for cut in ("accel_cutoff", "batt_cutoff", "temp_cutoff"))
        self.c_main = pick([lp1_coefficient(period, c["main_cutoff"]) for c in cfgs]).astype(F)
        self.c_cmd = pick([lp1_coefficient(c["radio_period"], c["cmd_cutoff"]) for c in cfgs]).astype(F)
        self.att_tc = dict(tc_xy=pick([c["tc_xy"] for c in cfgs]).astype(F), tc_z=pick([c["tc_z"] for c in cfgs]).astype(F))
        self.v_crit = pick([c["threshold"] for c in cfgs]).astype(F)
        self.v_warn = (F(1.05) * self.v_crit).astype(F)
        self.radio_period = pick([c["radio_period"] for c in cfgs]).astype(F)
        z = lambda k: np.zeros((k, n), F)                             # noqa: E731
        self.gyro_lp = [z(3) for _ in range(4)]
        self.acc_lp = [z(3) for _ in range(4)]
        v0 = (self.v_crit * F(1.2)).astype(F)
        self.batt_lp = [v0.copy() for _ in range(4)]
        self.temp_lp = [np.full(n, 25, F) for _ in range(4)]
        self.volts = (D(1.2) * self.v_crit.astype(D)).astype(F)       # float _battVoltage = 1.2 * threshold, Quadcopter_T.cpp:72
        self.main_dt = np.full(n, self.period, F)
        self.cmd_dt = self.radio_period.copy()
        t0 = lambda: np.full(n, t0_us, np.uint64)                     # noqa: E731
        self.t_main, self.t_cmd, self.t_radio, self.t_est, self.t_reset, self.t_uwb = t0(), t0(), t0(), t0(), t0(), t0()
        self.att = z(4)
        self.att[0] = 1
        self.ang_vel = z(3)
        self.init = np.zeros(n, bool)
        self.state = np.full(n, IDLE, np.uint8)
        self.reason = np.zeros(n, np.uint8)
        self.warnings = np.zeros(n, np.uint8)
        self.flags = np.zeros(n, np.uint8)
        self.running = np.zeros(n, bool)
        self.cycle = np.zeros(n, np.uint32)
        self.packet = np.zeros(n, np.uint32)
        self.forces, self.motor_cmd = z(4), z(4)
        self.payload = z(4)
        self.rates_cmd, self.have_cmd = z(4), np.zeros(n, bool)
        self.mail_arrival = np.zeros(n, np.uint64)
        self.mail_type = np.zeros(n, np.uint8)
        self.mail_flags = np.zeros(n, np.uint8)
        self.count = {k: 0 for k in BRANCHES}

    # ---- SetCommandRadioMsg, however it arrives -------------------------------------------------------------------------------
    def deliver(self, now_us, who, mtype, flags=0, floats=None):
        """who: bool mask or indices; mtype, flags: scalars or per selected vehicle; floats [4, k] for types 4 and 5"""
        idx = np.flatnonzero(who) if np.asarray(who).dtype == bool else np.asarray(who, int)
        mtype = np.broadcast_to(np.asarray(mtype, np.uint8), idx.shape)
        self.mail_arrival[idx] = np.uint64(now_us + 1)
        self.mail_type[idx] = mtype
        self.mail_flags[idx] = np.broadcast_to(np.asarray(flags, np.uint8), idx.shape)
        fl = np.zeros((4, idx.size), F) if floats is None else np.asarray(floats, F).reshape(4, idx.size)
        rates = mtype == MSG_RATES
        self.rates_cmd[:, idx] = np.where(rates, fl, F(0))
        self.have_cmd[idx] = rates
        acc = mtype == MSG_ACCELERATION
        self.payload[:, idx[acc]] = fl[:, acc]

    def set_battery(self, volts, first=0):
        v = np.asarray(volts, F)
        self.volts[first:first + v.size] = v

    def set_state(self, first=0, est_att4=None, est_ang_vel3=None, imu_initialized=None, lowpass20=None, flight_state=None, motors_running=None,
                  last_radio_us=None):
        """afe_onboard_set_state"""
        given = [a for a in (est_att4, est_ang_vel3, imu_initialized, lowpass20, flight_state, motors_running, last_radio_us) if a is not None]
        s = slice(first, first + np.asarray(given[0]).shape[-1])
        if est_att4 is not None:
            self.att[:, s] = np.asarray(est_att4, F)
        if est_ang_vel3 is not None:
            self.ang_vel[:, s] = np.asarray(est_ang_vel3, F)
        if imu_initialized is not None:
            self.init[s] = np.asarray(imu_initialized) != 0
        if lowpass20 is not None:
            lp = np.asarray(lowpass20, F)
            for k in range(4):
                self.acc_lp[k] = self.acc_lp[k].copy()
                self.acc_lp[k][:, s] = lp[3 * k:3 * k + 3]
                self.batt_lp[k] = self.batt_lp[k].copy()
                self.batt_lp[k][s] = lp[12 + k]
                self.temp_lp[k] = self.temp_lp[k].copy()
                self.temp_lp[k][s] = lp[16 + k]
        if flight_state is not None:
            self.state[s] = np.asarray(flight_state, np.uint8)
        if motors_running is not None:
            self.running[s] = np.asarray(motors_running) != 0
        if last_radio_us is not None:
            self.t_radio[s] = np.asarray(last_radio_us, np.uint64)

    # ---- Quadcopter_T.cpp:163-185 + QuadcopterLogic::Run ------------------------------------------------------------------------
    def _monitor(self, c, now_us, reset, lp, who):
        dt = seconds_f(now_us, reset)
        new = np.where(c <= F(0), dt, c * lp + (F(1) - c) * dt).astype(F)
        adj = (dt * F(1e6)).astype(np.uint64)
        lp[who] = new[who]
        reset[who] = (reset + adj)[who]

    def tick(self, T, gyro_raw, acc_raw):
        """one tick at clock T [us] with the engine's raw IMU sample -> counts16"""
        n, math, cnt = self.n, self.math, self.count
        T = np.uint64(T)
        with np.errstate(all="ignore"):
            # 0 the radio
            have = self.mail_arrival != 0
            fresh = have & (self.mail_arrival - np.uint64(1) <= T) & have
            cnt["msg_new"] += int(fresh.sum())
            cnt["msg_waits"] += int((have & ~fresh).sum())
            ta = np.where(fresh, self.mail_arrival - np.uint64(1), T).astype(np.uint64)
            mtype = np.where(fresh, self.mail_type, 0)
            self.flags[fresh] = self.mail_flags[fresh]
            self.t_radio[fresh] = ta[fresh]
            self._monitor(self.c_cmd, ta, self.t_cmd, self.cmd_dt, fresh)
            self.mail_arrival[fresh] = 0
            # 1 battery
            vfilt = lp2_apply(self.k_batt, self.batt_lp, self.volts)
            # 2 IMU
            gyro = lp2_apply(self.k_gyro, self.gyro_lp, gref.mount_rotate(self.R, gyro_raw) - F(0))
            acc = lp2_apply(self.k_acc, self.acc_lp, gref.mount_rotate(self.R, acc_raw))
            lp2_apply(self.k_temp, self.temp_lp, np.full(n, 25, F))
            # 3
            self.cycle += np.uint32(1)
            self._monitor(self.c_main, T, self.t_main, self.main_dt, np.ones(n, bool))
            # 4 Predict
            first = ~self.init
            cnt["kf_init"] += int(first.sum())
            cnt["kf_predict"] += int((~first).sum())
            ident = np.zeros((4, n), F)
            ident[0] = 1
            ax0, an0 = gravity_axis_angle(ident, acc, math, cnt, first)
            att_first = q_mul(ident, from_axis_angle(ax0, an0, math)).astype(F)
            dt = seconds_f(T, self.t_est)
            rv = (gyro * dt).astype(F)
            theta = np.sqrt(v_dot(rv, rv)).astype(F)
            cnt["rotvec_small"] += int(((theta < fc.MIN_ANGLE) & ~first).sum())
            att1 = q_mul(self.att, fc.from_rotvec(rv, _fm(math))).astype(F)
            ax1, an1 = gravity_axis_angle(att1, acc, math, cnt, ~first)
            corr = ((dt / F(4.0)) * an1).astype(F)
            att_later = q_mul(att1, from_axis_angle(ax1, corr, math)).astype(F)
            self.att = np.where(first, att_first, att_later).astype(F)
            self.ang_vel = np.where(first, F(0), gyro).astype(F)
            self.t_reset[first] = T
            self.t_est[:] = T
            self.init[:] = True
            # 5 ParseIncomingCommunications
            st = self.state.copy()
            sticky = (st == PANIC) | (st == KILLED)
            cnt["msg_ignored_panic"] += int((fresh & (st == PANIC)).sum())
            cnt["msg_ignored_killed"] += int((fresh & (st == KILLED)).sum())
            go = fresh & ~sticky
            kill = go & (mtype == MSG_KILL)
            cnt["msg_kill"] += int(kill.sum())
            cnt["msg_kill_first_reason"] += int((kill & (self.reason == 0)).sum())
            cnt["msg_kill_reason_kept"] += int((kill & (self.reason != 0)).sum())
            self.reason[kill & (self.reason == 0)] = KILLED_EXTERNALLY
            st[kill] = KILLED
            for m, s, name in ((MSG_POSITION, AUTONOMOUS, "msg_position"), (MSG_ACCELERATION, ACCELERATION, "msg_acceleration"),
                               (MSG_RATES, RATES, "msg_rates"), (MSG_IDLE, IDLE, "msg_idle")):
                sel = go & (mtype == m)
                cnt[name] += int(sel.sum())
                st[sel] = s
            # 6 UpdateWarnings
            since_radio = seconds_f(T, self.t_radio)
            w = self.warnings.copy()
            for bit, cond, name in ((WARN_LOW_BATT, vfilt <= self.v_warn, "warn_low_batt"),
                                    (WARN_CMD_RATE, np.abs(self.cmd_dt - self.radio_period) > F(0.1) * self.radio_period, "warn_cmd_rate"),
                                    (WARN_CMD_BATCH_DROP, since_radio > F(3) * self.radio_period, "warn_batch_drop"),
                                    (WARN_ONBOARD_FREQ, np.abs(self.main_dt - self.period) > F(0.05) * self.period, "warn_onboard_freq"),
                                    (WARN_UWB_RESET, seconds_f(T, self.t_reset) < F(0.02), "warn_reset")):
                cnt[name] += int(cond.sum())
                w[cond] |= np.uint8(bit)
            self.warnings = w
            # 7 CheckPanicReasons
            run = self.running
            cnt["motors_not_running"] += int((~run).sum())
            unsafe = np.zeros(n, np.uint8)
            suppressed = (self.flags & FLAG_DISABLE_CHECKS) != 0
            est_z = np.zeros(n, F)
            crazy = run & (est_z < F(-2.0)) & ~suppressed
            unsafe[crazy] = ESTIMATE_CRAZY
            uwb = run & ((T - self.t_uwb) > np.uint64(1500000)) & (st == AUTONOMOUS)
            unsafe[uwb] = UWB_TIMEOUT
            e3 = np.zeros((3, n), F)
            e3[2] = 1
            down = m_rotate(q_matrix(self.att), e3).astype(F)[2] < 0
            cnt["upside_down_suppressed"] += int((run & down & suppressed).sum())
            ud = run & down & ~suppressed
            unsafe[ud] = UPSIDE_DOWN
            silent = run & ((T - self.t_radio) > np.uint64(1500000))
            cnt["ovr_radio_over_upside_down"] += int((silent & ud).sum())
            unsafe[silent] = RADIO_TIMEOUT
            flat = run & (vfilt <= self.v_crit)
            cnt["ovr_battery_over_radio"] += int((flat & silent).sum())
            unsafe[flat] = LOW_BATTERY
            critical = ~((st == UNINIT) | (st == IDLE) | (st == PANIC) | (st == KILLED))
            cnt["not_critical"] += int(((unsafe != 0) & ~critical).sum())
            cnt["panic_estimate_crazy"] += int((critical & (unsafe == ESTIMATE_CRAZY)).sum())
            cnt["panic_uwb_timeout"] += int((critical & (unsafe == UWB_TIMEOUT)).sum())
            cnt["panic_upside_down"] += int((critical & (unsafe == UPSIDE_DOWN)).sum())
            cnt["panic_radio"] += int((critical & (unsafe == RADIO_TIMEOUT)).sum())
            cnt["panic_battery"] += int((critical & (unsafe == LOW_BATTERY)).sum())
            panic = (unsafe != 0) & critical
            st[panic] = PANIC
            self.reason[panic] = unsafe[panic]
            self.state = st
            # 8 the controller
            zero4 = np.zeros((4, n), F)
            f_rates, cmd_rates = motors_from_rates(self.L, self.rates_cmd[0], self.rates_cmd[1:4], self.ang_vel)
            step_cmd = np.where(self.have_cmd, cmd_rates, F(0)).astype(F)        # what the step kernel wrote at this tick
            des = self.payload[0:3]
            cut = des[2] < F(-9.81) / F(2)
            proper = np.stack([des[0] + F(0), des[1] + F(0), des[2] + F(9.81)]).astype(F)
            nrm = np.sqrt(v_dot(proper, proper)).astype(F)
            dirv = (proper / nrm).astype(F)
            angle = guarded_acos(v_dot(dirv, e3).astype(F), math)
            axv = v_cross(e3, dirv).astype(F)
            na = np.sqrt(v_dot(axv, axv)).astype(F)
            tiny = na < F(1e-6)
            k = (angle / np.where(tiny, F(1), na)).astype(F)
            des_att = fc.from_rotvec((axv * k).astype(F), _fm(math))
            des_att[:, tiny] = np.array([[1], [0], [0], [0]], F)
            _, p, r = to_euler_ypr(self.att, math)
            no_yaw = from_euler_ypr(np.zeros(n, F), p, r, math)
            wdes = sc.desired_angular_velocity(des_att, no_yaw, self.att_tc, _stages_math(math))
            wdes[2] = self.payload[3]
            f_acc, cmd_acc = motors_from_rates(self.L, nrm, wdes, self.ang_vel)
            is_r, is_a = st == RATES, st == ACCELERATION
            cnt["ctl_rates"] += int(is_r.sum())
            cnt["ctl_zero"] += int((~is_r & ~is_a).sum())
            cnt["acc_cutoff"] += int((is_a & cut).sum())
            cnt["acc_identity"] += int((is_a & ~cut & tiny).sum())
            cnt["acc_general"] += int((is_a & ~cut & ~tiny).sum())
            live_a = is_a & ~cut
            self.forces = np.where(is_r, f_rates, np.where(live_a, f_acc, zero4)).astype(F)
            self.motor_cmd = np.where(is_r, step_cmd, np.where(live_a, cmd_acc, zero4)).astype(F)
            self.running = (self.motor_cmd > 0).any(0)
        return self.counters()

    def counters(self):
        c = np.zeros(16, np.int64)
        c[0:7] = np.bincount(self.state, minlength=7)[:7]
        c[7:15] = np.bincount(self.reason, minlength=8)[:8]
        c[15] = int((self.warnings != 0).sum())
        return c

    def fields(self):
        """what Onboard.get of the package reads back, and three the telemetry packets carry besides"""
        return dict(flight_state=self.state.copy(), panic_reason=self.reason.copy(), warnings=self.warnings.copy(), est_att=self.att.copy(),
                    est_ang_vel=self.ang_vel.copy(), acc_filtered=self.acc_lp[3].copy(), gyro_filtered=self.gyro_lp[3].copy(),
                    temp_filtered=self.temp_lp[3].copy(), volts=self.volts.copy(), batt_filtered=self.batt_lp[3].copy(),
                    main_loop_dt=self.main_dt.copy(), cmd_dt=self.cmd_dt.copy(), motor_forces=self.forces.copy(), cycle_counter=self.cycle.copy(),
                    last_radio_us=self.t_radio.copy(), motors_running=self.running.astype(np.uint8))

    def telemetry(self, first=0, count=None):
        """GetTelemetryDataPackets for [first, first + count) -> uint8 [count, 2, 30]; counters advance, warnings are cleared"""
        count = self.n - first if count is None else count
        s = slice(first, first + count)
        out = np.zeros((count, 2, 30), np.uint8)
        codes1 = [telemetry_code(self.acc_lp[3][k, s], -30, 30) for k in range(3)] + [telemetry_code(self.gyro_lp[3][k, s], -35, 35) for k in range(3)] + \
                 [telemetry_code(self.forces[k, s], 0, 10) for k in range(4)] + [telemetry_code(np.zeros(count, F), -30, 30)] * 3 + \
                 [telemetry_code(self.volts[s], 0, 15)]
        w = self.att[0, s] > 0
        codes2 = [telemetry_code(np.zeros(count, F), -30, 30)] * 3 + [telemetry_code(np.where(w, self.att[k, s], -self.att[k, s]), -1, 1) for k in (1, 2, 3)] + \
                 [telemetry_code(self.temp_lp[3][s], -100, 100)] + [telemetry_code(np.zeros(count, F), -100, 100)] * 5
        out[:, 0, 0], out[:, 1, 0] = 0, 1
        out[:, 0, 1] = out[:, 1, 1] = (self.packet[s] % 256).astype(np.uint8)
        for slot, c in enumerate(codes1):
            out[:, 0, 2 + 2 * slot], out[:, 0, 3 + 2 * slot] = c & 0xff, c >> 8
        for slot, c in enumerate(codes2):
            out[:, 1, 2 + 2 * slot], out[:, 1, 3 + 2 * slot] = c & 0xff, c >> 8
        out[:, 1, 26], out[:, 1, 28] = self.reason[s], self.warnings[s]
        self.packet[s] += np.uint32(1)
        self.warnings[s] = 0
        return out


def tilt_from_vertical(att):
    """angle between the body z axis and the world z axis [rad], float64"""
    q = np.asarray(att, D)
    return np.arccos(np.clip(q[0] * q[0] - q[1] * q[1] - q[2] * q[2] + q[3] * q[3], -1, 1))
