"""The field node's mission, restated line by line in scalar Python from the reference's text:

  ExampleVehicleStateMachine   AIFS_ROS/hiperlab_rostools/src/QuadGPSRatesControl/ExampleVehicleStateMachine.cpp:6-26, :106-379, :413-437
  SafetyNet                    Components/Components/Offboard/SafetyNet.hpp:17-50, :73-106
  QuadcopterController::Run    Components/Components/Offboard/QuadcopterController.cpp:5-9, :11-74
                               (QuadcopterPositionController.hpp:22-28, QuadcopterAttitudeController.hpp:35-68, Rotation.hpp, Vec3.hpp)

One vehicle, one object, one Run per period -- the shape of the reference, so that it can be read beside it.  SafetyNet and
QuadcopterController::Run are PINNED: tests/test_offboard_reference.py holds them to what the reference's own code, compiled
in place, computed (tests/golden/offboard_reference.npz).  ExampleVehicleStateMachine needs ROS headers and is compiled
nowhere in this repository: the switch is UNPINNED (nothing compares it with the reference's binary).  tests/stages_checker.py is the same arithmetic in numpy for N vehicles and must equal
this file bit for bit; agri-fly_amd/csrc/afe_stages.hip is the device's.

Number formats: D = float64 where the reference says double, F = float32 where it says float; every narrowing is where
the reference has it.  math(op, x): op 0, 1 = sin, cos (float64), 2..5 = sinf, cosf, asinf, acosf (float32), arrays in
and out (tests/stages_checker.py has glibc_math, numpy_math and device_math).

What differs from the reference, as the device library's header states: the trajectory id and the constants of the
stages are configuration (the defaults are the reference's), the circle centre's x and y are a per-vehicle pair, the
time since the last good measurement is handed in, and HaveLowBattery() is bit 0 of a warnings byte that is handed in."""
import numpy as np

from tests.offboard_stub import radio_quantise

D, F = np.float64, np.float32
MIN_ANGLE = F(4.84813681e-6)
PI_F = F(np.pi)
WAIT, SPOOLUP, TAKEOFF, FLIGHT, LANDING, COMPLETE, EMERGENCY = range(7)
MSG_NONE, MSG_KILL, MSG_RATES, MSG_IDLE = 0, 2, 5, 6          # RadioTypes.hpp:18-24


def _m(math, op, x):
    return math(op, np.array([x], D if op < 2 else F))[0]


# ---- Rotation.hpp / Vec3.hpp on tuples of one scalar type -------------------------------------------------------------------
def q_mul(a, b):
    """Rotation.hpp:124-131, this = a, r1 = b"""
    return (b[0] * a[0] - b[1] * a[1] - b[2] * a[2] - b[3] * a[3],
            b[1] * a[0] + b[0] * a[1] + b[3] * a[2] - b[2] * a[3],
            b[2] * a[0] - b[3] * a[1] + b[0] * a[2] + b[1] * a[3],
            b[3] * a[0] + b[2] * a[1] - b[1] * a[2] + b[0] * a[3])


def q_inv(q):
    return (q[0], -q[1], -q[2], -q[3])


def q_matrix(q):
    """Rotation.hpp:196-220"""
    two = type(q[0])(2)
    r0, r1, r2, r3 = q[0] * q[0], q[1] * q[1], q[2] * q[2], q[3] * q[3]
    return (r0 + r1 - r2 - r3, two * q[1] * q[2] - two * q[0] * q[3], two * q[1] * q[3] + two * q[0] * q[2],
            two * q[1] * q[2] + two * q[0] * q[3], r0 - r1 + r2 - r3, two * q[2] * q[3] - two * q[0] * q[1],
            two * q[1] * q[3] - two * q[0] * q[2], two * q[2] * q[3] + two * q[0] * q[1], r0 - r1 - r2 + r3)


def m_rotate(R, v):
    return (R[0] * v[0] + R[1] * v[1] + R[2] * v[2], R[3] * v[0] + R[4] * v[1] + R[5] * v[2], R[6] * v[0] + R[7] * v[1] + R[8] * v[2])


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def from_rotvec(r, math):
    """Rotationf::FromRotationVector, Rotation.hpp:84-97"""
    theta = np.sqrt(dot(r, r))
    if theta < MIN_ANGLE:
        return (F(1), F(0), F(0), F(0))
    ux, uy, uz = r[0] / theta, r[1] / theta, r[2] / theta
    half = theta * F(0.5)
    s, c = _m(math, 2, half), _m(math, 3, half)
    return (c, s * ux, s * uy, s * uz)


def to_rotvec(q, math):
    """Rotationf::ToRotationVector, Rotation.hpp:144-161 (the norm held at 1 for asinf)"""
    n = (q[1], q[2], q[3]) if q[0] > 0 else (-q[1], -q[2], -q[3])
    norm = np.sqrt(dot(n, n))
    angle = _m(math, 4, norm if norm < F(1) else F(1)) * F(2)
    if angle < MIN_ANGLE:
        return (F(0), F(0), F(0))
    k = angle / norm
    return (n[0] * k, n[1] * k, n[2] * k)


def tilt_angle(c, math):
    """QuadcopterController.cpp:51-59 (1 - 1e-12f is 1 in float)"""
    if c >= F(1):
        return F(0)
    if c <= F(-1):
        return PI_F
    return _m(math, 5, c)


def desired_angular_velocity(des_att, cur_att, tc_xy, tc_z, math):
    """QuadcopterAttitudeController::GetDesiredAngularVelocity, QuadcopterAttitudeController.hpp:35-68"""
    e3 = (F(0), F(0), F(1))
    err = q_mul(q_inv(des_att), cur_att)
    rot = to_rotvec(err, math)
    zb = m_rotate(q_matrix(q_inv(err)), e3)
    rax = cross(zb, e3)
    an = tilt_angle(dot(zb, e3), math)
    rn = np.sqrt(dot(rax, rax))
    rax = (F(0), F(0), F(0)) if rn < F(1e-12) else (rax[0] / rn, rax[1] / rn, rax[2] / rn)
    k3, k12 = F(1) / tc_z, F(1) / tc_xy
    nk3, kr = -k3, (k12 - k3) * an
    return (nk3 * rot[0] - kr * rax[0], nk3 * rot[1] - kr * rax[1], nk3 * rot[2] - kr * rax[2])


class QuadcopterController:
    """Offboard::QuadcopterController, Run only"""

    def __init__(self, nat_freq, damping, tc_xy, tc_z):
        self.min_vertical_proper_acc = D(0.5) * D(9.81)                  # :6
        self.max_proper_acc = D(20)                                      # :7
        self.min_proper_acc = D(-1)                                      # :8
        self.nat_freq, self.damping, self.tc_xy, self.tc_z = F(nat_freq), F(damping), F(tc_xy), F(tc_z)
        self.seen = {}

    def run(self, cur_pos, cur_vel, cur_att, des_pos, des_vel, des_acc, desired_yaw, math):
        """-> (outCmdThrust double, outCmdAngVel 3 doubles)"""
        seen = self.seen = {}
        e3 = (F(0), F(0), F(1))                                                                   # :17
        pf, vf, dp, dv, da = (tuple(F(x) for x in v) for v in (cur_pos, cur_vel, des_pos, des_vel, des_acc))
        w, z = self.nat_freq, self.damping
        # :20-22, QuadcopterPositionController.hpp:25-26
        cmd_acc = tuple(((dp[k] - pf[k]) * w) * w + (((dv[k] - vf[k]) * F(2)) * w) * z + da[k] for k in range(3))
        proper = [cmd_acc[0] + F(0), cmd_acc[1] + F(0), cmd_acc[2] + F(9.81)]                     # :24
        norm = np.sqrt(dot(proper, proper))
        seen["sat_norm"] = bool(D(norm) > self.max_proper_acc)
        if D(norm) > self.max_proper_acc:                                                         # :27-29
            f = F(self.max_proper_acc / D(np.sqrt(dot(proper, proper))))                          # Vec3f::operator*=(const float &)
            proper = [f * proper[0], f * proper[1], f * proper[2]]
        seen["z_floor"] = bool(D(proper[2]) < self.min_vertical_proper_acc)
        if D(proper[2]) < self.min_vertical_proper_acc:                                           # :32-34
            proper[2] = F(self.min_vertical_proper_acc)
        norm = np.sqrt(dot(proper, proper))                                                       # :37
        tdir = (proper[0] / norm, proper[1] / norm, proper[2] / norm)                             # :38
        qf = tuple(F(x) for x in cur_att)
        thrust = D(norm * dot(m_rotate(q_matrix(qf), e3), tdir))                                  # :41-42
        seen["thrust_floor"] = bool(thrust < self.min_proper_acc)
        if thrust < self.min_proper_acc:                                                          # :44-46
            thrust = self.min_proper_acc
        cos_angle = dot(tdir, e3)                                                                 # :51
        seen["cos_ge_1"], seen["cos_le_m1"] = bool(cos_angle >= F(1)), bool(cos_angle <= F(-1))
        angle = tilt_angle(cos_angle, math)                                                       # :52-59
        rot_ax = cross(e3, tdir)                                                                  # :60
        n = np.sqrt(dot(rot_ax, rot_ax))
        seen["n_tiny"] = bool(n < F(1e-6))
        if n < F(1e-6):                                                                           # :62-66
            cmd_att = (F(1), F(0), F(0), F(0))
        else:
            k = angle / n
            cmd_att = from_rotvec((k * rot_ax[0], k * rot_ax[1], k * rot_ax[2]), math)
        yawf = F(desired_yaw)
        seen["yaw_nonzero"] = bool(yawf != 0)
        cmd_att_yawed = q_mul(cmd_att, from_rotvec((F(0), F(0), yawf), math))                     # :69-70
        we = desired_angular_velocity(cmd_att_yawed, qf, self.tc_xy, self.tc_z, math)             # :72-73
        return thrust, (D(we[0]), D(we[1]), D(we[2]))


class SafetyNet:
    """Offboard::SafetyNet"""

    def __init__(self):
        self.vehicle_not_seen, self.unsafe_position, self.upside_down_and_low, self.user_unsafe = True, False, False, False   # :18-23
        self.min_corner, self.max_corner = (D(-2.4), D(-3.1), D(-0.5)), (D(1.8), D(3.1), D(4.5))
        self.min_normal_height, self.not_seen_timeout = D(1.0), D(0.5)
        self.faces = [False] * 6

    def set_safe_corners(self, min_corner, max_corner, min_normal_height):
        self.min_corner, self.max_corner = tuple(D(x) for x in min_corner), tuple(D(x) for x in max_corner)
        self.min_normal_height = D(min_normal_height)
        for i in range(3):
            assert self.min_corner[i] < self.max_corner[i]                                        # :68-70

    def update_with_estimator(self, pos, att, time_since_last_good_meas):
        self.vehicle_not_seen = bool(time_since_last_good_meas > self.not_seen_timeout)           # :75-79
        self.unsafe_position = False
        self.faces = [False] * 6
        for i in range(3):                                                                        # :82-89
            if pos[i] < self.min_corner[i]:
                self.unsafe_position = True
                self.faces[2 * i] = True
            if pos[i] > self.max_corner[i]:
                self.unsafe_position = True
                self.faces[2 * i + 1] = True
        self.upside_down_and_low = False
        if pos[2] < self.min_normal_height:                                                       # :92-97
            if m_rotate(q_matrix(att), (D(0), D(0), D(1)))[2] < 0:
                self.upside_down_and_low = True

    def is_safe(self):                                                                            # :25-43
        return not (self.vehicle_not_seen or self.unsafe_position or self.upside_down_and_low or self.user_unsafe)

    def set_unsafe(self):
        self.user_unsafe = True

    def bits(self):
        return 1 * self.vehicle_not_seen + 2 * self.unsafe_position + 4 * self.upside_down_and_low + 8 * self.user_unsafe


def _min(a, b):
    return b if b < a else a                                             # std::min


class ExampleVehicleStateMachine:
    """One vehicle.  cfg: the dict tests/stages_checker.py's default_config returns."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.stage, self.last_stage = WAIT, COMPLETE                                              # :10-11, :91-92
        self.ready = False
        self.init_pos = (D(0), D(0), D(0))
        self.desired_pos = (D(0), D(0), D(0))
        self.desired_yaw, self.cmd_yaw = D(0), D(0)
        self.warnings = 0
        self.last_pos, self.last_vel, self.last_acc = (D(0),) * 3, (D(0),) * 3, (D(0),) * 3
        self.centre = (D(0), D(-2.0) if cfg["traj_id"] == 1 else D(0))                            # :236, :264, :279
        self.t0_us = 0
        self.ctrl = QuadcopterController(cfg["nat_freq"], cfg["damping"], cfg["tc_xy"], cfg["tc_z"])
        self.safety = SafetyNet()
        self.safety.set_safe_corners(cfg["min_corner"], cfg["max_corner"], cfg["min_normal_height"])   # :88
        self.safety.not_seen_timeout = D(cfg["not_seen_timeout"])
        self.request = 0
        self.computed = (F(0),) * 4
        self.sent = (F(0),) * 4
        self.msg_type = MSG_NONE
        self.seen = {}

    def have_low_battery(self):
        return bool(self.warnings & 0x01)

    def _run_controller(self, pos, vel, att, des_pos, des_vel, des_acc, math):
        """RunControllerAndUpdateEstimator, :413-437"""
        thrust, w = self.ctrl.run(pos, vel, att, des_pos, des_vel, des_acc, self.cmd_yaw, math)
        self.seen.update(self.ctrl.seen)
        self.seen["ran"] = True
        return MSG_RATES, (F(thrust), F(w[0]), F(w[1]), F(w[2]))

    def run(self, should_start, should_stop, now_us, pos, vel, att, time_since_last_good_meas, math):
        """Run(shouldStart, shouldStop), :106-379, at the clock now_us; -> (type, sent 4 floats)"""
        cfg = self.cfg
        seen = self.seen = {}
        should_start = bool(should_start) or bool(self.request & 1)
        should_stop = bool(should_stop) or bool(self.request & 2)
        pos, vel, att = tuple(D(x) for x in pos), tuple(D(x) for x in vel), tuple(D(x) for x in att)
        stage_change = self.stage != self.last_stage                                              # :109-113
        self.last_stage = self.stage
        if stage_change:
            self.t0_us = int(now_us)
        seconds = D(np.uint64(now_us) - np.uint64(self.t0_us)) * D(1e-6)                          # Timer.hpp:36-38
        self.safety.update_with_estimator(pos, att, D(time_since_last_good_meas))                 # :118-119
        safe = self.safety.is_safe()
        msg_type, computed = MSG_NONE, (F(0), F(0), F(0), F(0))                                   # a default-constructed message
        stage = self.stage
        zero3 = (D(0), D(0), D(0))
        if stage == WAIT:                                                                         # :126-133
            if should_start:
                self.stage = SPOOLUP
                seen["wait_start"] = True
        elif stage == SPOOLUP:                                                                    # :135-172
            if not safe:
                self.stage = EMERGENCY
                seen["spool_unsafe"] = True
            msg_type, computed = MSG_RATES, (F(D(9.81) * D(cfg["spool_up_thrust_by_weight"])), F(0), F(0), F(0))
            if seconds > D(cfg["spool_up_time"]):
                self.stage = TAKEOFF
                seen["spool_done"] = True
                seen["ovr_spool_unsafe_to_takeoff"] = not safe
            if self.have_low_battery():
                self.stage = LANDING
                seen["spool_lowbatt"] = True
                seen["ovr_lowbatt_after_unsafe"] = not safe
        elif stage == TAKEOFF:                                                                    # :174-201
            if stage_change:
                self.init_pos = pos
                seen["takeoff_change"] = True
            if not safe:
                self.stage = EMERGENCY
                seen["takeoff_unsafe"] = True
            frac = seconds / D(cfg["takeoff_time"])
            if frac >= 1.0:
                self.stage = FLIGHT
                frac = D(1.0)
                seen["takeoff_done"] = True
                seen["ovr_takeoff_unsafe_to_flight"] = not safe
            a = D(1) - frac
            cmd_pos = tuple(a * self.init_pos[k] + frac * self.desired_pos[k] for k in range(3))
            msg_type, computed = self._run_controller(pos, vel, att, cmd_pos, zero3, zero3, math)
            if self.have_low_battery():
                self.stage = LANDING
                seen["takeoff_lowbatt"] = True
                seen["ovr_lowbatt_after_unsafe"] = not safe
        elif stage == FLIGHT:                                                                     # :203-310
            if not safe:
                self.stage = EMERGENCY
                seen["flight_unsafe"] = True
            if self.have_low_battery():
                self.stage = LANDING
                seen["flight_lowbatt"] = True
                seen["ovr_lowbatt_after_unsafe"] = not safe
            traj_id = cfg["traj_id"]
            cmd_pos, cmd_vel, cmd_acc = self.desired_pos, zero3, zero3
            t = seconds
            frac = _min(t / D(cfg["get_into_action_time"]), D(1.0))
            des = self.desired_pos
            seen["traj%d" % traj_id] = True
            if traj_id == 0:
                self.cmd_yaw = D(0)
            elif traj_id in (1, 3, 4):
                radius = D(1.0) if traj_id == 1 else D(0.5)
                ang = D(1) if traj_id == 3 else D(0.5)
                arg = ang * t
                s, c = _m(math, 0, arg), _m(math, 1, arg)
                zc, zv, za = D(0), D(0), D(0)
                if traj_id == 4:
                    arg4 = arg * D(4)
                    s4, c4 = _m(math, 0, arg4), _m(math, 1, arg4)
                    zc, zv, za = c4, -s4, -c4
                k1, k2 = radius * ang, radius * (ang * ang)                                       # pow(angSpeed, 2): exact for 0.5, 1
                cmd_pos = (self.centre[0] + radius * c, self.centre[1] + radius * s, des[2] + radius * zc)
                cmd_vel = (k1 * (-s), k1 * c, k1 * zv)
                cmd_acc = (k2 * (-c), k2 * (-s), k2 * za)
                self.cmd_yaw = self.desired_yaw + arg if traj_id == 1 else D(0) if traj_id == 3 else arg
            elif traj_id == 2:
                amplitude, ang = D(1.0), D(2.0)
                arg = ang * t
                s, c = _m(math, 0, arg), _m(math, 1, arg)
                k1, k2 = amplitude * ang, amplitude * (ang * ang)
                cmd_pos = (des[0] + amplitude * D(0), des[1] + amplitude * s, des[2] + amplitude * D(0))
                cmd_vel = (k1 * D(0), k1 * c, k1 * D(0))
                cmd_acc = (k2 * D(0), k2 * (-s), k2 * D(0))
                self.cmd_yaw = self.desired_yaw
            else:
                self.cmd_yaw = D(0.2) * t
            a = D(1) - frac
            self.last_pos = tuple(a * des[k] + frac * cmd_pos[k] for k in range(3))               # :300-302
            self.last_vel = tuple(frac * cmd_vel[k] for k in range(3))
            self.last_acc = tuple(frac * cmd_acc[k] for k in range(3))
            msg_type, computed = self._run_controller(pos, vel, att, self.last_pos, self.last_vel, self.last_acc, math)
            if should_stop:
                self.stage = LANDING
                seen["flight_stop"] = True
        elif stage == LANDING:                                                                    # :312-336
            if not safe:
                self.stage = EMERGENCY
                seen["landing_unsafe"] = True
            down = -D(cfg["landing_speed"])
            frac = _min(seconds / D(cfg["get_into_action_time"]), D(1.0))
            cmd_pos = (self.last_pos[0] + seconds * D(0), self.last_pos[1] + seconds * D(0), self.last_pos[2] + seconds * down)
            if cmd_pos[2] < 0:
                self.stage = COMPLETE
                seen["landing_done"] = True
                seen["ovr_landing_unsafe_to_complete"] = not safe
            a = D(1) - frac
            des_pos = tuple(a * self.last_pos[k] + frac * cmd_pos[k] for k in range(3))
            des_vel = (a * self.last_vel[0] + frac * D(0), a * self.last_vel[1] + frac * D(0), a * self.last_vel[2] + frac * down)
            des_acc = tuple(a * self.last_acc[k] + frac * D(0) for k in range(3))
            msg_type, computed = self._run_controller(pos, vel, att, des_pos, des_vel, des_acc, math)
        elif stage == COMPLETE:                                                                   # :338-357
            msg_type = MSG_IDLE
            if seconds > 1.0:
                self.ready = True
                seen["complete_ready"] = True
        else:                                                                                     # :359-372
            msg_type = MSG_KILL
            seen["emergency"] = True
        self.msg_type, self.computed = msg_type, computed
        self.sent = tuple(radio_quantise(np.array([c], F), 35)[0] for c in computed)
        return msg_type, self.sent


def deliver(held, msg):
    """What afe_set_commands_from_radio leaves of a delivered message; held = (four floats, have)"""
    msg_type, sent = msg
    if msg_type == MSG_RATES:
        return (tuple(sent), 1)
    if msg_type in (MSG_IDLE, MSG_KILL):
        return ((F(0),) * 4, 0)
    return held
