"""Offboard::GPSIMUStateEstimator restated in scalar Python, line by line (test infrastructure; the counterpart of
tests/offboard_reference.py).  The lines cited are those of the reference's
Components/Components/Offboard/GPSIMUStateEstimator.cpp unless another file is named.  tests/gps_estimator_checker.py is the
same in vectorised numpy and agri-fly_amd/csrc/afe_gps_estimator.hip the same on the device; all three must give the same
bits.  The class's own text is compiled where it lies by oracle/_ref/gps_probe (against the recording dense stand-in
oracle/eigen_dense) and tests/test_gps_reference.py holds this file to what it recorded: bit for bit outside Eigen, the
branch and the finite / non-finite mask exactly, Eigen's finite results within derived bounds.

Python floats are IEEE doubles and nothing is contracted, so a line of C++ double arithmetic is the same line here.  The
reference's float quirks are kept (f32 below narrows): acosf, the 1e-6f and -9.81f constants, GetUnitVector's float norm, the
division by 2.0f.  Eigen's evaluation order cannot be known, so this file FIXES one for finite numbers (predict_covariance,
update) and takes the DENSE products' behaviour for non-finite ones (tainted): see the header of afe_gps_estimator.hip.

math(op, x): op 0 sin, 1 cos (double), 2 acosf (x is narrowed to float, the float result widened)."""
import ctypes as _C
import ctypes.util as _Cu
import math as _m

import numpy as np

MIN_ANGLE = 4.84813681e-6                 # Rotation.hpp:39
F = np.float32

_libm = _C.CDLL(_Cu.find_library("m") or "libm.so.6")
for _n in ("sin", "cos"):
    getattr(_libm, _n).restype = _C.c_double
    getattr(_libm, _n).argtypes = [_C.c_double]
for _n in ("acosf", "sinf", "cosf"):
    getattr(_libm, _n).restype = _C.c_float
    getattr(_libm, _n).argtypes = [_C.c_float]


def f32(x):
    """(double)(float)x"""
    with np.errstate(all="ignore"):
        return float(F(x))


def glibc_math(op, x):
    x = np.asarray(x, np.float64)
    if op == 2:
        with np.errstate(all="ignore"):
            return np.array([_libm.acosf(float(F(v))) for v in x.reshape(-1)], np.float64).reshape(x.shape)
    f = _libm.sin if op == 0 else _libm.cos
    return np.array([f(float(v)) for v in x.reshape(-1)], np.float64).reshape(x.shape)


def _scalar(math, op, x):
    return float(np.asarray(math(op, np.array([x], np.float64))).reshape(-1)[0])


def div(a, b):
    """IEEE division (Python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def default_config():
    """:21-27 and QuadcopterLogic.cpp:102"""
    return dict(init_sigma_pos=3.0, init_sigma_vel=3.0, init_sigma_att=10.0 * float(_m.pi) / 180.0, sigma_acc=5.0, sigma_gyro=0.1,
                sigma_pos=0.25, accel_lowpass_cutoff=100.0)


BRANCHES = ("first_predict_level", "first_predict_tilted", "measure_before_predict", "predict", "update", "singular_nonfinite",
            "singular_tiny", "acos_domain_neg", "acos_domain_pos", "rotvec_small", "rotvec_large", "nan_position")


# ---- Vec3.hpp / Rotation.hpp -------------------------------------------------------------------------------------------
def v_norm(a):                                                  # Vec3.hpp:101-119
    return _m.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])


def q_mul(a, b):                                                # Rotation.hpp:124-131, this = a, r1 = b
    return (b[0] * a[0] - b[1] * a[1] - b[2] * a[2] - b[3] * a[3],
            b[1] * a[0] + b[0] * a[1] + b[3] * a[2] - b[2] * a[3],
            b[2] * a[0] - b[3] * a[1] + b[0] * a[2] + b[1] * a[3],
            b[3] * a[0] + b[2] * a[1] - b[1] * a[2] + b[0] * a[3])


def q_inv(q):                                                   # Rotation.hpp:66-68
    return (q[0], -q[1], -q[2], -q[3])


def q_matrix(q):                                                # Rotation.hpp:196-220
    r0, r1, r2, r3 = q[0] * q[0], q[1] * q[1], q[2] * q[2], q[3] * q[3]
    return [r0 + r1 - r2 - r3, 2 * q[1] * q[2] - 2 * q[0] * q[3], 2 * q[1] * q[3] + 2 * q[0] * q[2],
            2 * q[1] * q[2] + 2 * q[0] * q[3], r0 - r1 + r2 - r3, 2 * q[2] * q[3] - 2 * q[0] * q[1],
            2 * q[1] * q[3] - 2 * q[0] * q[2], 2 * q[2] * q[3] + 2 * q[0] * q[1], r0 - r1 - r2 + r3]


def m_rotate(R, a):                                             # Rotation.hpp:234-243
    return (R[0] * a[0] + R[1] * a[1] + R[2] * a[2], R[3] * a[0] + R[4] * a[1] + R[5] * a[2], R[6] * a[0] + R[7] * a[1] + R[8] * a[2])


def from_axis_angle(u, angle, math):                            # Rotation.hpp:91-97
    s, c = _scalar(math, 0, angle * 0.5), _scalar(math, 1, angle * 0.5)
    return (c, s * u[0], s * u[1], s * u[2])


def from_rotvec(r, math, count=None):                           # Rotation.hpp:84-89
    theta = v_norm(r)
    if theta < MIN_ANGLE:
        if count is not None:
            count["rotvec_small"] += 1
        return (1.0, 0.0, 0.0, 0.0)
    if count is not None:
        count["rotvec_large"] += 1
    return from_axis_angle((div(r[0], theta), div(r[1], theta), div(r[2], theta)), theta, math)


def align(att, meas_acc, math, count=None):
    """:77-100: the attitude that makes the measured acceleration gravity.  (In Predict the attitude is the identity Reset()
    has just set; the lines are written for any.)"""
    expected = m_rotate(q_matrix(q_inv(att)), (0.0, 0.0, 1.0))  # :79
    n = f32(v_norm(meas_acc))                                   # :80, Vec3.hpp:126-129: float const n
    unit = (div(meas_acc[0], n), div(meas_acc[1], n), div(meas_acc[2], n))
    cos_err = expected[0] * unit[0] + expected[1] * unit[1] + expected[2] * unit[2]       # :81
    ax = (unit[1] * expected[2] - unit[2] * expected[1], unit[2] * expected[0] - unit[0] * expected[2],
          unit[0] * expected[1] - unit[1] * expected[0])        # :83
    if v_norm(ax) > f32(1e-6):                                  # :84
        d = v_norm(ax)
        ax = (div(ax[0], d), div(ax[1], d), div(ax[2], d))
        if count is not None:
            count["first_predict_tilted"] += 1
    else:
        ax = (1.0, 0.0, 0.0)
        if count is not None:
            count["first_predict_level"] += 1
    angle = _scalar(math, 2, cos_err)                           # :90
    if abs(f32(cos_err)) > 1.0:                                 # :91 `if (errno)`: acosf's domain error
        if cos_err < 0:
            angle = float(_m.pi)
            if count is not None:
                count["acos_domain_neg"] += 1
        else:
            angle = 0.0
            if count is not None:
                count["acos_domain_pos"] += 1
    return q_mul(att, from_axis_angle(ax, angle, math))         # :100


# ---- the evaluation order this project fixes ------------------------------------------------------------------------------
def jacobian_entries(dt, R, a, w, k):
    """:143-191: nv[i][m] = f(I_VEL + i, I_ATT + m), na[m][j] = f(I_ATT + m, I_ATT + j) (its diagonal is not used);
    R the rotation matrix of the old attitude, a measAcc, w measGyro, k _lastMeasUpdateAttCorrection"""
    nv = [[dt * (+a[1] * R[3 * i + 2] - a[2] * R[3 * i + 1]),      # :147-152
           dt * (-a[0] * R[3 * i + 2] + a[2] * R[3 * i + 0]),      # :157-162
           dt * (+a[0] * R[3 * i + 1] - a[1] * R[3 * i + 0])]      # :167-172
          for i in range(3)]
    gx, gy, gz = dt * w[0] + k[0] / 2.0, dt * w[1] + k[1] / 2.0, dt * w[2] + k[2] / 2.0
    na = [[0.0, +gz, -gy], [-gz, 0.0, +gx], [+gy, -gx, 0.0]]        # :175-191
    return nv, na


def off_identity_rows(dt, nv, na):
    """row i of N = F - I as [(k, N[i][k])], k ascending (:133-191)"""
    rows = [[(3 + i, dt)] for i in range(3)]
    rows += [[(6, nv[i][0]), (7, nv[i][1]), (8, nv[i][2])] for i in range(3)]
    rows += [[(7, na[0][1]), (8, na[0][2])], [(6, na[1][0]), (8, na[1][2])], [(6, na[2][0]), (7, na[2][1])]]
    return rows


def tainted(P):
    """a covariance with an entry that is not finite.  The reference's products are dense: f * _cov * f.transpose() (:195),
    H * (_cov * H.transpose()) (:224) and (I - L H) * _cov (:255) multiply by the structural zeros of f, H and I - L H too,
    and 0 * NaN = 0 * Inf = NaN.  One such entry therefore makes every entry of f P f' non-finite whatever f holds, and
    every entry of S; see predict_covariance and UpdateWithMeasurement."""
    return not all(_m.isfinite(P[i][j]) for i in range(9) for j in range(9))


def predict_covariance(P, rows):
    """:195, F P F' with F = I + N.  A tainted P gives NaN in all 81 places (the dense product's mask; where the dense
    product would hold an infinity -- entry (i, j) for a lone infinity at (k, l) with F[i][k] and F[j][l] both non-zero --
    this definition says NaN as well: the next update restarts either way)."""
    if tainted(P):
        return [[float("nan")] * 9 for _ in range(9)]
    T = [[P[i][j] for j in range(9)] for i in range(9)]
    for i in range(9):
        for j in range(9):
            for k, nik in rows[i]:
                T[i][j] = T[i][j] + nik * P[k][j]
    C = [[T[i][j] for j in range(9)] for i in range(9)]
    for i in range(9):
        for j in range(9):
            for k, njk in rows[j]:
                C[i][j] = C[i][j] + T[i][k] * njk
    return C


def innovation(P, r_pos):
    """:224-228 -> (S, det, adj(S))"""
    S = [[P[i][j] + (r_pos if i == j else 0.0) for j in range(3)] for i in range(3)]
    adj = [[S[1][1] * S[2][2] - S[1][2] * S[2][1], S[0][2] * S[2][1] - S[0][1] * S[2][2], S[0][1] * S[1][2] - S[0][2] * S[1][1]],
           [S[1][2] * S[2][0] - S[1][0] * S[2][2], S[0][0] * S[2][2] - S[0][2] * S[2][0], S[0][2] * S[1][0] - S[0][0] * S[1][2]],
           [S[1][0] * S[2][1] - S[1][1] * S[2][0], S[0][1] * S[2][0] - S[0][0] * S[2][1], S[0][0] * S[1][1] - S[0][1] * S[1][0]]]
    det = (S[0][0] * (S[1][1] * S[2][2] - S[1][2] * S[2][1]) - S[0][1] * (S[1][0] * S[2][2] - S[1][2] * S[2][0])) + \
        S[0][2] * (S[1][0] * S[2][1] - S[1][1] * S[2][0])
    return S, det, adj


def gain(P, det, adj):
    """:239-240"""
    r = div(1, det)
    Si = [[adj[i][j] * r for j in range(3)] for i in range(3)]
    return [[(P[i][0] * Si[0][j] + P[i][1] * Si[1][j]) + P[i][2] * Si[2][j] for j in range(3)] for i in range(9)]


def update_covariance(P, L):
    """:255-256"""
    C = [[P[i][j] - ((L[i][0] * P[0][j] + L[i][1] * P[1][j]) + L[i][2] * P[2][j]) for j in range(9)] for i in range(9)]
    return [[0.5 * (C[i][j] + C[j][i]) for j in range(9)] for i in range(9)]


# ---- Timer.hpp on an integer microsecond master clock ----------------------------------------------------------------------
class Clock:
    def __init__(self):
        self.us = 0


class Timer:
    def __init__(self, clock):
        self.clock, self.reset_us = clock, clock.us

    def seconds(self):                                          # Timer.hpp:36-50
        return (self.clock.us - self.reset_us) * 1e-6

    def reset(self):
        self.reset_us = self.clock.us


class GPSIMUStateEstimator:
    def __init__(self, clock, cfg=None, math=glibc_math):       # :9-30
        self.cfg = default_config() if cfg is None else cfg
        self.math = math
        self.count = {k: 0 for k in BRANCHES}
        self.estimate_timer, self.last_good = Timer(clock), Timer(clock)
        self.initialized = False
        self.num_resets = 0
        self.corr = (float("nan"),) * 3                          # a Vec3d nobody sets: Vec3.hpp:34-38
        self.Reset()

    def Reset(self):                                            # :32-44
        self.num_resets += 1
        self.initialized = False
        self.pos, self.vel, self.ang_vel = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)
        self.att = (1.0, 0.0, 0.0, 0.0)
        self.estimate_timer.reset()
        self.last_good.reset()
        self.ResetVariance()

    def ResetVariance(self):                                    # :46-54
        c = self.cfg
        d = [c["init_sigma_pos"] * c["init_sigma_pos"]] * 3 + [c["init_sigma_vel"] * c["init_sigma_vel"]] * 3 + \
            [c["init_sigma_att"] * c["init_sigma_att"]] * 3
        self.cov = [[d[i] if i == j else 0.0 for j in range(9)] for i in range(9)]

    def _restart(self, meas_pos):                               # :210-215, :230-235
        self.pos, self.vel, self.ang_vel = tuple(meas_pos), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)
        self.att = (1.0, 0.0, 0.0, 0.0)
        self.ResetVariance()

    def GetCurrentEstimate(self):                               # :56-64
        return self.pos + self.vel + self.att + self.ang_vel

    def Predict(self, meas_acc, meas_gyro):                     # :66-203
        c = self.cfg
        if not self.initialized:                                # :67-103
            self.Reset()
            self.initialized = True
            self.estimate_timer.reset()
            self.att = align(self.att, meas_acc, self.math, self.count)
            return
        self.count["predict"] += 1
        dt = self.estimate_timer.seconds()                      # :107
        self.estimate_timer.reset()
        pos, vel, att = self.pos, self.vel, self.att            # :113-115
        R = q_matrix(att)
        ra = m_rotate(R, meas_acc)                              # :117
        acc = (ra[0] + 0.0, ra[1] + 0.0, ra[2] + f32(-9.81))
        self.pos = (pos[0] + dt * vel[0], pos[1] + dt * vel[1], pos[2] + dt * vel[2])      # :118
        self.vel = (vel[0] + dt * acc[0], vel[1] + dt * acc[1], vel[2] + dt * acc[2])      # :119
        self.att = q_mul(att, from_rotvec((dt * meas_gyro[0], dt * meas_gyro[1], dt * meas_gyro[2]), self.math, self.count))   # :120
        self.ang_vel = tuple(meas_gyro)                         # :121
        nv, na = jacobian_entries(dt, R, meas_acc, meas_gyro, self.corr)
        self.corr = (0.0, 0.0, 0.0)                             # :192
        C = predict_covariance(self.cov, off_identity_rows(dt, nv, na))                    # :195
        for i in range(3):                                      # :197-202
            C[3 + i][3 + i] = C[3 + i][3 + i] + c["sigma_acc"] * c["sigma_acc"] * dt * dt
            C[6 + i][6 + i] = C[6 + i][6 + i] + c["sigma_gyro"] * c["sigma_gyro"] * dt * dt
        self.cov = C

    def UpdateWithMeasurement(self, meas_pos):                  # :206-258
        c = self.cfg
        if any(v != v for v in meas_pos):
            self.count["nan_position"] += 1
        if not self.initialized:                                # :208-217
            self.count["measure_before_predict"] += 1
            self.initialized = True
            self._restart(meas_pos)
            return False
        S, det, adj = innovation(self.cov, c["sigma_pos"] * c["sigma_pos"])                # :224-227
        finite = all(_m.isfinite(S[i][j]) for i in range(3) for j in range(3)) and not tainted(self.cov)   # dense: see tainted
        if abs(det) < 1e-10 or not finite:                      # :228-237
            self.count["singular_tiny" if finite else "singular_nonfinite"] += 1
            self._restart(meas_pos)
            return True
        self.count["update"] += 1
        L = gain(self.cov, det, adj)                            # :239-240
        d = (meas_pos[0] - self.pos[0], meas_pos[1] - self.pos[1], meas_pos[2] - self.pos[2])   # :244
        dx = [(L[i][0] * d[0] + L[i][1] * d[1]) + L[i][2] * d[2] for i in range(9)]        # :246
        self.pos = (self.pos[0] + dx[0], self.pos[1] + dx[1], self.pos[2] + dx[2])         # :248
        self.vel = (self.vel[0] + dx[3], self.vel[1] + dx[4], self.vel[2] + dx[5])         # :249
        self.corr = (dx[6], dx[7], dx[8])                       # :250
        self.att = q_mul(self.att, from_rotvec(self.corr, self.math, self.count))          # :252
        self.cov = update_covariance(self.cov, L)               # :255-256
        self.last_good.reset()                                  # :257
        return False


# ---- the sample: QuadcopterLogic's mount and low-pass in float ---------------------------------------------------------------
def mount_matrix(yaw, pitch, roll):
    """QuadcopterLogic::_R = Rotationf::FromEulerYPR(yaw, pitch, roll).GetRotationMatrix() (QuadcopterLogic.cpp:116-117), as
    afe_params.cpp makes it: the transpose of the inverse mount's matrix, in float with libm's sinf / cosf"""
    h = F(0.5)
    cs = lambda x: (F(_libm.cosf(float(h * F(x)))), F(_libm.sinf(float(h * F(x)))))
    (cy, sy), (cp, sp), (cr, sr) = cs(yaw), cs(pitch), cs(roll)
    q0 = cy * cp * cr + sy * sp * sr
    q1 = -(cy * cp * sr - sy * sp * cr)
    q2 = -(cy * sp * cr + sy * cp * sr)
    q3 = -(sy * cp * cr - cy * sp * sr)
    r0, r1, r2, r3 = q0 * q0, q1 * q1, q2 * q2, q3 * q3
    two = F(2)
    M = [r0 + r1 - r2 - r3, two * q1 * q2 - two * q0 * q3, two * q1 * q3 + two * q0 * q2,
         two * q1 * q2 + two * q0 * q3, r0 - r1 + r2 - r3, two * q2 * q3 - two * q0 * q1,
         two * q1 * q3 - two * q0 * q2, two * q2 * q3 + two * q0 * q1, r0 - r1 - r2 + r3]
    return np.array([[M[3 * j + i] for j in range(3)] for i in range(3)], F)


def lowpass_coefficients(period, cutoff):
    """LowPassFilterSecondOrder.hpp:22-49 in float -> a1, a2, b0, b1, b2"""
    dt, wc, sqrt2, two, four = F(period), F(cutoff), F(np.sqrt(2.0)), F(2), F(4)
    den = dt * dt * wc * wc + two * sqrt2 * dt * wc + four
    return ((dt * dt * wc * wc - two * sqrt2 * dt * wc + four) / den, two * (dt * dt * wc * wc - four) / den,
            dt * dt * wc * wc / den, dt * dt * wc * wc / den, two * dt * dt * wc * wc / den)


class LowPass3:
    """LowPassFilterSecondOrder<float, Vec3f> for n vehicles: planar float32 [3, n]; Apply is :51-64"""

    def __init__(self, n, period, cutoff):
        self.a1, self.a2, self.b0, self.b1, self.b2 = lowpass_coefficients(period, cutoff)
        self.reset(n)

    def reset(self, n=None, who=None):
        if who is None:
            self.xm0, self.xm1, self.ym0, self.ym1 = (np.zeros((3, n), F) for _ in range(4))
        else:
            for a in (self.xm0, self.xm1, self.ym0, self.ym1):
                a[:, who] = 0

    def apply(self, x):
        x = np.asarray(x, F)
        out = self.b2 * x
        out = out + (+self.b0 * self.xm0 + self.b1 * self.xm1)
        out = out + (-self.a1 * self.ym0 - self.a2 * self.ym1)
        self.xm0, self.xm1 = self.xm1, x
        self.ym0, self.ym1 = self.ym1, out
        assert out.dtype == F
        return out


def mount_rotate(R, x):
    """_R * Vec3f(x) (Vec3.hpp:201-210) per vehicle: R [n, 3, 3] float32, x [3, n] float32; every product and sum rounded"""
    x = np.asarray(x, F)
    return np.stack([((F(0) + R[:, i, 0] * x[0]) + R[:, i, 1] * x[1]) + R[:, i, 2] * x[2] for i in range(3)])
