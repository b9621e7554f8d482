"""Onboard::QuadcopterLogic and the complementary branch of Onboard::KalmanFilter6DOF restated line by line in scalar Python,
quirks included, for ONE vehicle without UWB ranging (Components/Components/Logic/QuadcopterLogic.{hpp,cpp},
KalmanFilter6DOF.cpp:33-147, Common/Time/Timer.hpp, Common/Math/LowPassFilter{First,Second}Order.hpp, Rotation.hpp, Vec3.hpp,
Common/DataTypes/TelemetryPacket.hpp), with the part of Simulation::Quadcopter_T::Run that feeds it (Quadcopter_T.cpp:159-185).
Every value is a numpy float32 scalar, so every operation rounds as the reference's float code does; math(op, x[, x2]) is
tests/onboard_checker.py's (sinf, cosf, acosf, asinf, atan2f).

The classes keep the reference's names.  Not restated: UWB (no network exists in Rappids_Simulator), FS_FULLY_AUTONOMOUS's
controller, TestMotors, the calibrations.  tests/onboard_checker.py is the same in numpy for N vehicles; tests/test_onboard_cpu.py
holds the two to each other bit for bit.

PINNED to the reference's own class: oracle/_ref/onboard_probe compiles QuadcopterLogic.cpp and KalmanFilter6DOF.cpp where they lie
(against oracle/eigen_trap, whose Eigen arithmetic aborts by name: the path restated here executes none) and is given, call for
call, what this restatement is given on the scripted flight of tests/onboard_flight.py; tests/golden/make_onboard_reference.py
asserts every field of every vehicle after every tick and every telemetry byte equal bit for bit, and
tests/test_onboard_reference.py holds this file to what it recorded (tests/golden/onboard_reference.npz).  The feed
(Vehicle, TickGate) is pinned by the probe's vehicle mode, Quadcopter_T<Onboard::QuadcopterLogic> itself.  STILL OPEN: the
branch behind _UWBInitialized, RunControllerFullyAutonomous, TestMotors and the calibrations (they would abort the probe by
name or are not driven)."""
import numpy as np

from tests.onboard_checker import lp1_coefficient            # (libm's expf through ctypes: one spelling of a library call)

F = np.float32
U64 = (1 << 64) - 1
FS_UNINITIALIZED, FS_IDLE, FS_FULLY_AUTONOMOUS, FS_PANIC, FS_KILLED, FS_EXTERNAL_ACCELERATION_CONTROL, FS_EXTERNAL_RATES_CONTROL = range(7)
M_PI_F = F(np.pi)


def _m(math, op, x, x2=None):
    a = np.array([x], F)
    return F(math(op, a)[0]) if x2 is None else F(math(op, a, np.array([x2], F))[0])


class Clock:                                                    # ManualTimer
    def __init__(self, now_us=0):
        self.now_us = int(now_us)


class Timer:                                                    # Timer.hpp
    def __init__(self, clock):
        self.clock = clock
        self.Reset()

    def Reset(self):
        self.last = self.clock.now_us

    def GetMicroSeconds(self):
        return (self.clock.now_us - self.last) & U64

    def GetSeconds_f(self):
        return F(F(self.GetMicroSeconds()) * F(1e-6))

    def AdjustTimeBySeconds(self, s):
        s = F(s)
        if s > 0:
            self.last = (self.last - int(F(s * F(1e6)))) & U64
        else:
            self.last = (self.last + int(F(s * F(-1e6)))) & U64


class LowPassFilterSecondOrder:                                 # LowPassFilterSecondOrder.hpp, TYPE_SAMPLE a float or a list of 3
    def Initialise(self, dt, wc, init):
        dt, wc = F(dt), F(wc)
        sqrt2, two, four = F(np.sqrt(2.0)), F(2), F(4)
        den = dt * dt * wc * wc + two * sqrt2 * dt * wc + four
        self.a1 = (dt * dt * wc * wc - two * sqrt2 * dt * wc + four) / den
        self.a2 = two * (dt * dt * wc * wc - four) / den
        self.b0 = dt * dt * wc * wc / den
        self.b1 = dt * dt * wc * wc / den
        self.b2 = two * dt * dt * wc * wc / den
        self.vec = isinstance(init, (list, tuple))
        cp = (lambda: [F(v) for v in init]) if self.vec else (lambda: F(init))
        self.xm0, self.xm1, self.ym0, self.ym1 = cp(), cp(), cp(), cp()

    def _one(self, x, xm0, xm1, ym0, ym1):
        out = self.b2 * x
        out = out + (+self.b0 * xm0 + self.b1 * xm1)
        out = out + (-self.a1 * ym0 - self.a2 * ym1)
        return out

    def Apply(self, x):
        with np.errstate(all="ignore"):
            if self.vec:
                x = [F(v) for v in x]
                out = [self._one(x[k], self.xm0[k], self.xm1[k], self.ym0[k], self.ym1[k]) for k in range(3)]
            else:
                x = F(x)
                out = self._one(x, self.xm0, self.xm1, self.ym0, self.ym1)
        self.xm0, self.xm1 = self.xm1, x
        self.ym0, self.ym1 = self.ym1, out
        return out

    def GetValue(self):
        return self.ym1


class LowPassFilterFirstOrder:                                  # LowPassFilterFirstOrder.hpp
    def Initialise(self, period, wc, init):
        self.prev = F(init)
        self.c = lp1_coefficient(period, wc)                   # exp(-samplingPeriod * cutoff): the float overload

    def Apply(self, x):
        x = F(x)
        if self.c <= F(0):
            self.prev = x
            return x
        out = self.c * self.prev + (F(1) - self.c) * x
        self.prev = out
        return out


class MonitorSimplePeriod:                                      # QuadcopterLogic.hpp:387-403
    def __init__(self, clock, samplePeriod, cutoff, expected):
        self.timeSinceLast = Timer(clock)
        self.filter = LowPassFilterFirstOrder()
        self.filter.Initialise(samplePeriod, cutoff, expected)
        self.lpDt = F(expected)

    def Update(self):
        dt = self.timeSinceLast.GetSeconds_f()
        self.lpDt = self.filter.Apply(dt)
        self.timeSinceLast.AdjustTimeBySeconds(-dt)


# ---- Vec3f / Rotationf ---------------------------------------------------------------------------------------------------------
def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def norm2(a):
    return F(np.sqrt(dot(a, a)))


def q_mul(a, b):                                                # Rotation.hpp:124-131, this = a, r1 = b
    return [b[0] * a[0] - b[1] * a[1] - b[2] * a[2] - b[3] * a[3], b[1] * a[0] + b[0] * a[1] + b[3] * a[2] - b[2] * a[3],
            b[2] * a[0] - b[3] * a[1] + b[0] * a[2] + b[1] * a[3], b[3] * a[0] + b[2] * a[1] - b[1] * a[2] + b[0] * a[3]]


def q_inv(q):
    return [q[0], -q[1], -q[2], -q[3]]


def q_rotate(q, v):                                             # Rotation.hpp:196-245
    two = F(2)
    r0, r1, r2, r3 = q[0] * q[0], q[1] * q[1], q[2] * q[2], q[3] * q[3]
    R = [r0 + r1 - r2 - r3, two * q[1] * q[2] - two * q[0] * q[3], two * q[1] * q[3] + two * q[0] * q[2],
         two * q[1] * q[2] + two * q[0] * q[3], r0 - r1 + r2 - r3, two * q[2] * q[3] - two * q[0] * q[1],
         two * q[1] * q[3] - two * q[0] * q[2], two * q[2] * q[3] + two * q[0] * q[1], r0 - r1 - r2 + r3]
    return [R[0] * v[0] + R[1] * v[1] + R[2] * v[2], R[3] * v[0] + R[4] * v[1] + R[5] * v[2], R[6] * v[0] + R[7] * v[1] + R[8] * v[2]]


def from_axis_angle(u, angle, math):                            # :92-97
    h = F(angle * F(0.5))
    s, c = _m(math, 0, h), _m(math, 1, h)
    return [c, s * u[0], s * u[1], s * u[2]]


def from_rotvec(r, math):                                       # :84-89
    theta = norm2(r)
    if theta < F(4.84813681e-6):
        return [F(1), F(0), F(0), F(0)]
    return from_axis_angle([r[0] / theta, r[1] / theta, r[2] / theta], theta, math)


def to_rotvec(q, math):                                         # :144-161 (the norm held at 1 for asinf, as tests/offboard_stub.py)
    n = [q[1], q[2], q[3]] if q[0] > 0 else [-q[1], -q[2], -q[3]]
    norm = norm2(n)
    angle = F(_m(math, 3, norm if norm < F(1) else F(1)) * F(2))
    if angle < F(4.84813681e-6):
        return [F(0), F(0), F(0)]
    k = F(angle / norm)
    return [n[0] * k, n[1] * k, n[2] * k]


def from_euler_ypr(y, p, r, math):                              # :99-110
    h = F(0.5)
    sy, cy, sp, cp, sr, cr = _m(math, 0, h * y), _m(math, 1, h * y), _m(math, 0, h * p), _m(math, 1, h * p), _m(math, 0, h * r), _m(math, 1, h * r)
    return [cy * cp * cr + sy * sp * sr, cy * cp * sr - sy * sp * cr, cy * sp * cr + sy * cp * sr, sy * cp * cr - cy * sp * sr]


def to_euler_ypr(q, math):                                      # :163-169
    two = F(2.0)
    y = _m(math, 4, two * q[1] * q[2] + two * q[0] * q[3], q[1] * q[1] + q[0] * q[0] - q[3] * q[3] - q[2] * q[2])
    p = -_m(math, 3, two * q[1] * q[3] - two * q[0] * q[2])
    r = _m(math, 4, two * q[2] * q[3] + two * q[0] * q[1], q[3] * q[3] - q[2] * q[2] - q[1] * q[1] + q[0] * q[0])
    return y, p, r


def MapToOnesRange(x, a, b):                                    # TelemetryPacket.hpp:39-41 (a, b ints: b - a in int, then float)
    return ((F(x) - F(a)) / F(b - a)) * F(2) - F(1)


def EncodeOnesRange(t):                                         # :55-63; a NaN passes both tests, and its conversion to uint16 is 0 on x86-64
    with np.errstate(all="ignore"):
        if t < -1 or t > 1 or np.isnan(t):
            return 0
        return int(F(32768) + F(32767) * t) & 0xffff


def acosf_errno(c, math):
    """errno = 0; angle = acosf(c); if (errno) angle = c < 0 ? float(M_PI) : 0 -- glibc sets EDOM for |c| > 1, not for a NaN"""
    if c > F(1) or c < F(-1):
        return M_PI_F if c < 0 else F(0)
    return _m(math, 2, c)


class KalmanFilter6DOF:                                         # KalmanFilter6DOF.cpp, without UWB
    def __init__(self, clock, math):
        self.math = math
        self._estimateTimer = Timer(clock)
        self._IMUInitialized = False
        self._numResets = 0
        self._lastCheckNumResets = 0
        self._att = [F(1), F(0), F(0), F(0)]
        self._angVel = [F(0), F(0), F(0)]

    def Reset(self):                                            # :33-68
        self._numResets += 1
        self._IMUInitialized = False
        self._att = [F(1), F(0), F(0), F(0)]
        self._angVel = [F(0), F(0), F(0)]
        self._estimateTimer.Reset()

    def GetWasResetSinceLastCheck(self):
        change = self._lastCheckNumResets != self._numResets
        self._lastCheckNumResets = self._numResets
        return change

    def _axis_angle(self, measAcc):
        with np.errstate(all="ignore"):
            expAccelerometer = q_rotate(q_inv(self._att), [F(0), F(0), F(1)])
            n = norm2(measAcc)
            accUnitVec = [measAcc[0] / n, measAcc[1] / n, measAcc[2] / n]
            cosAngleError = dot(expAccelerometer, accUnitVec)
            rotAx = cross(accUnitVec, expAccelerometer)
            if norm2(rotAx) > F(1e-6):
                nr = norm2(rotAx)
                rotAx = [rotAx[0] / nr, rotAx[1] / nr, rotAx[2] / nr]
            else:
                rotAx = [F(1), F(0), F(0)]
            return rotAx, acosf_errno(cosAngleError, self.math)

    def Predict(self, measGyro, measAcc):                       # :70-147
        with np.errstate(all="ignore"):
            if not self._IMUInitialized:
                self.Reset()
                self._IMUInitialized = True
                self._estimateTimer.Reset()
                rotAx, angle = self._axis_angle(measAcc)
                self._att = q_mul(self._att, from_axis_angle(rotAx, angle, self.math))
                return
            dt = self._estimateTimer.GetSeconds_f()
            self._estimateTimer.Reset()
            self._angVel = list(measGyro)
            self._att = q_mul(self._att, from_rotvec([measGyro[0] * dt, measGyro[1] * dt, measGyro[2] * dt], self.math))
            rotAx, angle = self._axis_angle(measAcc)
            corrAngle = (dt / F(4.0)) * angle
            self._att = q_mul(self._att, from_axis_angle(rotAx, corrAngle, self.math))


class QuadcopterLogic:
    """logic: tests/onboard_checker.logic_record; cfg: tests/onboard_checker.default_config / config_from; R: the mount matrix"""

    def __init__(self, clock, period, logic, cfg, R, math):
        self.math, self.L, self.cfg = math, logic, cfg
        self._timer = clock
        self._onboardPeriod = F(period)
        self._radioCmdPeriod = F(cfg["radio_period"])
        self._kf = KalmanFilter6DOF(clock, math)
        self._timeSinceLastUwb = Timer(clock)
        self._timeSinceLastRadioMessage = Timer(clock)
        self._monitorCmdRate = MonitorSimplePeriod(clock, self._radioCmdPeriod, cfg["cmd_cutoff"], self._radioCmdPeriod)
        self._monitorMainLoopPeriod = MonitorSimplePeriod(clock, self._onboardPeriod, cfg["main_cutoff"], self._onboardPeriod)
        self._resetTimer = Timer(clock)                         # _monitorUWBEstimatorResets.timeSinceLast
        # Initialise(), :97-162
        self._R = R
        self._battThresholdCriticalVoltage = F(cfg["threshold"])
        self._battThresholdWarningVoltage = F(1.05) * self._battThresholdCriticalVoltage
        self._acc, self._gyro, self._temp, self._batt = (LowPassFilterSecondOrder() for _ in range(4))
        self._acc.Initialise(self._onboardPeriod, cfg["accel_cutoff"], [0, 0, 0])
        self._gyro.Initialise(self._onboardPeriod, logic["gyro_cutoff"], [0, 0, 0])
        self._temp.Initialise(self._onboardPeriod, cfg["temp_cutoff"], 25)
        self._batt.Initialise(self._onboardPeriod, cfg["batt_cutoff"], self._battThresholdCriticalVoltage * F(1.2))
        self._state = FS_IDLE
        self._firstPanicReason = 0
        self._kf.Reset()
        self._cycleCounter = 0
        self._desMotorSpeeds = [F(0)] * 4
        self._desMotorForcesForTelemetry = [F(0)] * 4
        self._telWarnings = 0
        self._telPacketCounter = 0
        self._msgNew, self._msgType, self._msgFlags, self._msgFloats = False, 0, 0, [F(0)] * 4
        self._voltageFiltered = F(0)
        self._voltageRaw = F(0)
        self._debug = [F(0)] * 6
        self._count = dict(batt=0, gyro=0, acc=0, temp=0)       # _battMeas.count, _imuRateGyro.count, ...

    def _rotate(self, v):                                       # _R * Vec3f, Vec3.hpp:201-210
        R = self._R
        return [((F(0) + R[i][0] * F(v[0])) + R[i][1] * F(v[1])) + R[i][2] * F(v[2]) for i in range(3)]

    def SetBatteryMeasurement(self, voltage):
        self._count["batt"] += 1
        self._voltageRaw = F(voltage)
        self._voltageFiltered = self._batt.Apply(voltage)

    def SetIMUMeasurementRateGyro(self, x, y, z):
        self._count["gyro"] += 1
        with np.errstate(all="ignore"):
            raw = self._rotate([x, y, z])
            self._gyro.Apply([raw[0] - F(0), raw[1] - F(0), raw[2] - F(0)])

    def SetIMUMeasurementAccelerometer(self, x, y, z):
        self._count["acc"] += 1
        with np.errstate(all="ignore"):
            self._acc.Apply(self._rotate([x, y, z]))

    def SetIMUMeasurementTemperature(self, t):
        self._count["temp"] += 1
        self._tempRaw = F(t)
        self._temp.Apply(t)

    def SetRadioMessage(self, mtype, flags, floats):
        self._msgNew, self._msgType, self._msgFlags, self._msgFloats = True, int(mtype), int(flags), [F(v) for v in floats]
        self._timeSinceLastRadioMessage.Reset()
        self._monitorCmdRate.Update()

    def GetAreMotorsRunning(self):
        return any(s > 0 for s in self._desMotorSpeeds)

    def GetTelemetryDataPackets(self):                          # :621-679, EncodeTelemetryPacket (TelemetryPacket.hpp:122-166) -> 2 x 30 bytes
        code = lambda x, a, b: EncodeOnesRange(MapToOnesRange(x, a, b))      # noqa: E731
        acc, gyro, q = self._acc.GetValue(), self._gyro.GetValue(), self._kf._att
        vec = [q[1], q[2], q[3]] if q[0] > 0 else [-q[1], -q[2], -q[3]]       # ToVectorPartOfQuaternion, Rotation.hpp:155-161
        with np.errstate(all="ignore"):
            d1 = [code(v, -30, 30) for v in acc] + [code(v, -35, 35) for v in gyro] + [code(v, 0, 10) for v in self._desMotorForcesForTelemetry] + \
                 [code(F(0), -30, 30)] * 3 + [code(self._voltageRaw, 0, 15)]
            d2 = [code(F(0), -30, 30)] * 3 + [code(v, -1, 1) for v in vec] + [code(v, -100, 100) for v in self._debug]
        number = self._telPacketCounter % 256
        p1 = bytes([0, number]) + b"".join(int(c).to_bytes(2, "little") for c in d1)
        p2 = bytes([1, number]) + b"".join(int(c).to_bytes(2, "little") for c in d2) + bytes([self._firstPanicReason, 0, self._telWarnings, 0])
        self._telPacketCounter += 1
        self._telWarnings = 0
        return p1, p2

    def Run(self):                                              # :164-219
        self._cycleCounter += 1
        self._monitorMainLoopPeriod.Update()
        self._kf.Predict(self._gyro.GetValue(), self._acc.GetValue())      # UpdateEstimator
        if self._msgNew:                                        # ParseIncomingCommunications
            self._msgNew = False
            if self._state != FS_PANIC and self._state != FS_KILLED:
                if self._msgType == 2:
                    self._state = FS_KILLED
                    if not self._firstPanicReason:
                        self._firstPanicReason = 7
                elif self._msgType == 3:
                    self._state = FS_FULLY_AUTONOMOUS
                elif self._msgType == 4:
                    self._state = FS_EXTERNAL_ACCELERATION_CONTROL
                elif self._msgType == 5:
                    self._state = FS_EXTERNAL_RATES_CONTROL
                elif self._msgType == 6:
                    self._state = FS_IDLE
        # UpdateWarnings
        if self._voltageFiltered <= self._battThresholdWarningVoltage:
            self._telWarnings |= 0x01
        if abs(self._monitorCmdRate.lpDt - self._radioCmdPeriod) > F(0.1) * self._radioCmdPeriod:
            self._telWarnings |= 0x02
        if self._timeSinceLastRadioMessage.GetSeconds_f() > F(3) * self._radioCmdPeriod:
            self._telWarnings |= 0x10
        if abs(self._monitorMainLoopPeriod.lpDt - self._onboardPeriod) > F(0.05) * self._onboardPeriod:
            self._telWarnings |= 0x08
        if self._kf.GetWasResetSinceLastCheck():
            self._resetTimer.Reset()
        if self._resetTimer.GetSeconds_f() < F(0.02):
            self._telWarnings |= 0x04
        # CheckPanicReasons
        unsafeReason = 0
        if self.GetAreMotorsRunning():
            suppressed = self._msgFlags & 0x02
            estPos_z = F(0)
            if estPos_z < F(-2.0) and not suppressed:
                unsafeReason = 1
            if self._timeSinceLastUwb.GetMicroSeconds() > 1500 * 1000 and self._state == FS_FULLY_AUTONOMOUS:
                unsafeReason = 2
            with np.errstate(all="ignore"):
                if q_rotate(self._kf._att, [F(0), F(0), F(1)])[2] < 0 and not suppressed:
                    unsafeReason = 3
            if self._timeSinceLastRadioMessage.GetMicroSeconds() > 1500 * 1000:
                unsafeReason = 4
            if self._voltageFiltered <= self._battThresholdCriticalVoltage:
                unsafeReason = 5
        critical = self._state not in (FS_UNINITIALIZED, FS_IDLE, FS_PANIC, FS_KILLED)
        if unsafeReason and critical:
            if self._state != FS_PANIC:
                self._state = FS_PANIC
                self._firstPanicReason = unsafeReason
        self._debug[0] = self._temp.GetValue()                  # :178
        # the controller
        with np.errstate(all="ignore"):
            if self._state == FS_EXTERNAL_ACCELERATION_CONTROL:
                return self.RunControllerExternalAcceleration()
            if self._state == FS_EXTERNAL_RATES_CONTROL:
                return self.RunControllerExternalRatesControl()
        self._desMotorSpeeds = [F(0)] * 4
        self._desMotorForcesForTelemetry = [F(0)] * 4

    def _mix(self, totalNormThrust, desAngVel):                 # GetDesiredTorques, GetMotorForces, PropellerSpeedsFromThrust
        L, w = self.L, self._kf._angVel
        e = [desAngVel[k] - w[k] for k in range(3)]
        aa = [e[0] / L["tc_xy"], e[1] / L["tc_xy"], e[2] / L["tc_z"]]
        I = L["I"]
        mv = lambda v: [((F(0) + I[3 * i] * v[0]) + I[3 * i + 1] * v[1]) + I[3 * i + 2] * v[2] for i in range(3)]   # noqa: E731
        Iw, Ia = mv(w), mv(aa)
        t = [Ia[0] + (w[1] * Iw[2] - w[2] * Iw[1]), Ia[1] + (w[2] * Iw[0] - w[0] * Iw[2]), Ia[2] + (w[0] * Iw[1] - w[1] * Iw[0])]
        tot = F(totalNormThrust) * L["mass"]
        des = L["max_cmd_total"] if tot > L["max_cmd_total"] else tot
        d, kt = L["d"], L["kt"]
        f = [(-t[0] / d - t[1] / d - t[2] / kt + des) / F(4), (-t[0] / d + t[1] / d + t[2] / kt + des) / F(4),
             (+t[0] / d + t[1] / d - t[2] / kt + des) / F(4), (+t[0] / d - t[1] / d + t[2] / kt + des) / F(4)]
        for i in range(4):
            if f[i] < L["min_thrust"]:
                f[i] = L["min_thrust"]
            elif f[i] > L["max_thrust"]:
                f[i] = L["max_thrust"]
        self._desMotorForcesForTelemetry = f
        self._desMotorSpeeds = [F(0) if f[i] <= 0 else F(np.sqrt(f[i] / (F(1) * L["kf"]))) for i in range(4)]

    def RunControllerExternalRatesControl(self):                # :528-541
        m = self._msgFloats
        self._mix(m[0], [m[1], m[2], m[3]])

    def RunControllerExternalAcceleration(self):                # :459-526
        m, math = self._msgFloats, self.math
        desAcc = [m[0], m[1], m[2]]
        if desAcc[2] < F(-9.81) / F(2):                         # "Magic number!"
            self._desMotorSpeeds = [F(0)] * 4
            self._desMotorForcesForTelemetry = [F(0)] * 4
            return
        proper = [desAcc[0] + F(0), desAcc[1] + F(0), desAcc[2] + F(9.81)]
        totalNormThrust = norm2(proper)
        dirv = [proper[k] / totalNormThrust for k in range(3)]
        e3 = [F(0), F(0), F(1)]
        angle = acosf_errno(dot(dirv, e3), math)
        rotAx = cross(e3, dirv)
        n = norm2(rotAx)
        if n < F(1e-6):
            desAtt = [F(1), F(0), F(0), F(0)]
        else:
            k = F(angle / n)
            desAtt = from_rotvec([rotAx[0] * k, rotAx[1] * k, rotAx[2] * k], math)
        _, p, r = to_euler_ypr(self._kf._att, math)
        estAttNoYaw = from_euler_ypr(F(0), p, r, math)
        desAngVel = self.GetDesiredAngularVelocity(desAtt, estAttNoYaw)
        desAngVel[2] = m[3]
        self._mix(totalNormThrust, desAngVel)

    def GetDesiredAngularVelocity(self, desAtt, estAtt):        # QuadcopterAttitudeController.hpp:35-68
        math = self.math
        e3 = [F(0), F(0), F(1)]
        errAtt = q_mul(q_inv(desAtt), estAtt)
        desRotVec = to_rotvec(errAtt, math)
        zb = q_rotate(q_inv(errAtt), e3)
        ax = cross(zb, e3)
        c = dot(zb, e3)
        an = F(0) if c >= F(1) else M_PI_F if c <= F(-1) else _m(math, 2, c)
        n = norm2(ax)
        ax = [F(0), F(0), F(0)] if n < F(1e-12) else [ax[0] / n, ax[1] / n, ax[2] / n]
        k3, k12 = F(1) / F(self.cfg["tc_z"]), F(1) / F(self.cfg["tc_xy"])
        nk3, kr = -k3, (k12 - k3) * an
        return [nk3 * desRotVec[k] - kr * ax[k] for k in range(3)]


class TickGate:
    """when Quadcopter_T::Run runs the logic (Quadcopter_T.cpp:159-160): a Timer read in DOUBLE seconds against the double period,
    then moved on by AdjustTimeBySeconds<double>(-period), which truncates period * 1e6 to whole microseconds"""

    def __init__(self, clock, period):
        self.clock, self.period, self.last = clock, float(period), clock.now_us

    def fires(self):
        if float((self.clock.now_us - self.last) & U64) * 1e-6 > self.period:
            self.last = (self.last + int(-self.period * -1e6)) & U64
            return True
        return False


class Vehicle:
    """what Quadcopter_T::Run does at a logic tick (Quadcopter_T.cpp:163-185), the clock set by the caller; radio, tick, place
    and telemetry are every way tests/onboard_flight.drive_scalar touches a vehicle (a recorder with the same four methods
    turns the drive into the call list oracle/_ref/onboard_probe is given)"""

    def __init__(self, t0_us, period, logic, cfg, R, math):
        self.clock = Clock(t0_us)
        self.logic = QuadcopterLogic(self.clock, period, logic, cfg, R, math)
        self._battVoltage = F(np.float64(1.2) * np.float64(cfg["threshold"]))     # float = double * float, :72

    def radio(self, now_us, mtype, flags, floats):
        self.clock.now_us = int(now_us)
        self.logic.SetRadioMessage(mtype, flags, floats)

    def set_battery(self, volts):
        self._battVoltage = F(volts)

    def place(self, name, value):
        """afe_onboard_set_state's fields written into the members they stand for"""
        L = self.logic
        if name == "est_att4":
            L._kf._att = [F(x) for x in value]
        elif name == "est_ang_vel3":
            L._kf._angVel = [F(x) for x in value]
        elif name == "imu_initialized":
            L._kf._IMUInitialized = bool(value)
        elif name == "flight_state":
            L._state = int(value)
        elif name == "last_radio_us":
            L._timeSinceLastRadioMessage.last = int(value)
        elif name == "lowpass20":
            col = np.asarray(value, F)
            L._acc.xm0, L._acc.xm1, L._acc.ym0, L._acc.ym1 = (list(col[3 * m:3 * m + 3]) for m in range(4))
            L._batt.xm0, L._batt.xm1, L._batt.ym0, L._batt.ym1 = col[12:16]
            L._temp.xm0, L._temp.xm1, L._temp.ym0, L._temp.ym1 = col[16:20]
        else:
            raise ValueError(name)

    def telemetry(self):
        return self.logic.GetTelemetryDataPackets()

    def tick(self, T_us, gyro, acc):
        self.clock.now_us = int(T_us)
        L = self.logic
        L.SetBatteryMeasurement(self._battVoltage)
        L.SetIMUMeasurementRateGyro(*gyro)
        L.SetIMUMeasurementAccelerometer(*acc)
        L.SetIMUMeasurementTemperature(F(25))
        L.Run()
        return [F(v) for v in L._desMotorSpeeds]
