"""The GPS + IMU state estimator's specification in numpy, vectorised over vehicles (test infrastructure).
tests/gps_imu_reference.py is the definition in scalar Python, line by line from the reference's GPSIMUStateEstimator.cpp;
agri-fly_amd/csrc/afe_gps_estimator.hip follows it on the device, and this file restates it for whole ensembles.  All three
must give the same bits.

  arithmetic        float64 arrays, explicit left-to-right sums and products: the order is the contract
  transcendentals   a parameter: math(op, x), op 0 sin, 1 cos (float64), 2 acosf (x narrowed to float32, the result widened).
                    device_math(afa) asks the GPU (afe_gps_estimator_selftest_math), glibc_math asks libm through ctypes;
                    nudged(math) moves every result one ulp (of its own format) up
  the sample        Sampler: the logic's mount and the two float low-passes, fed the raw sample of afe_get_imu

Arrays are planar: [components, n]; the covariance is [9, 9, n].  Times are integer microseconds since the estimator was made."""
import numpy as np

from tests import gps_imu_reference as ref
from tests.gps_imu_reference import BRANCHES, F, MIN_ANGLE, default_config, glibc_math

D = np.float64


def device_math(afa, device=-1):
    return lambda op, x: afa.gps_estimator_selftest_math(op, x, device=device).reshape(np.shape(x))


def nudged(math):
    def f(op, x):
        y = math(op, x)
        if op == 2:
            return np.nextafter(y.astype(F), F(np.inf)).astype(D)
        return np.nextafter(y, np.inf)
    return f


def config_from(cfg):
    """a GpsEstimatorConfig of the package -> the dict the classes take"""
    return {k: float(getattr(cfg, k)) for k in default_config()}


def differing(a, b):
    """where two arrays differ in a bit.  A NaN equals any NaN: which of two NaN operands an operation hands on, and with
    which sign, IEEE 754 leaves to the implementation (x86 scalar, x86 vector and gfx950 each choose differently), and the
    reference's own unset correction vector fills the covariance with NaN in the first Predict calls."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        return (np.ascontiguousarray(a).view(u) != np.ascontiguousarray(b).view(u)) & ~(np.isnan(a) & np.isnan(b))
    return a != b


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return not differing(a, b).any()


# ---- Vec3.hpp / Rotation.hpp, as in gps_imu_reference ----------------------------------------------------------------------
def v_norm(a):
    return np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])


def q_mul(a, b):
    return np.stack([b[0] * a[0] - b[1] * a[1] - b[2] * a[2] - b[3] * a[3],
                     b[1] * a[0] + b[0] * a[1] + b[3] * a[2] - b[2] * a[3],
                     b[2] * a[0] - b[3] * a[1] + b[0] * a[2] + b[1] * a[3],
                     b[3] * a[0] + b[2] * a[1] - b[1] * a[2] + b[0] * a[3]])


def q_inv(q):
    return np.stack([q[0], -q[1], -q[2], -q[3]])


def q_matrix(q):
    r0, r1, r2, r3 = q[0] * q[0], q[1] * q[1], q[2] * q[2], q[3] * q[3]
    return [r0 + r1 - r2 - r3, 2 * q[1] * q[2] - 2 * q[0] * q[3], 2 * q[1] * q[3] + 2 * q[0] * q[2],
            2 * q[1] * q[2] + 2 * q[0] * q[3], r0 - r1 + r2 - r3, 2 * q[2] * q[3] - 2 * q[0] * q[1],
            2 * q[1] * q[3] - 2 * q[0] * q[2], 2 * q[2] * q[3] + 2 * q[0] * q[1], r0 - r1 - r2 + r3]


def m_rotate(R, a):
    return np.stack([R[0] * a[0] + R[1] * a[1] + R[2] * a[2], R[3] * a[0] + R[4] * a[1] + R[5] * a[2],
                     R[6] * a[0] + R[7] * a[1] + R[8] * a[2]])


def from_axis_angle(u, angle, math):
    s, c = math(0, angle * 0.5), math(1, angle * 0.5)
    return np.stack([c, s * u[0], s * u[1], s * u[2]])


def from_rotvec(r, math, count=None, live=None):
    theta = v_norm(r)
    small = theta < MIN_ANGLE
    th = np.where(small, 1.0, theta)
    q = from_axis_angle(np.stack([r[0] / th, r[1] / th, r[2] / th]), th, math)
    ident = np.zeros_like(q)
    ident[0] = 1.0
    if count is not None:
        live = np.ones(theta.shape, bool) if live is None else live
        count["rotvec_small"] += int((small & live).sum())
        count["rotvec_large"] += int((~small & live).sum())
    return np.where(small, ident, q)


def align(att, meas_acc, math, count=None, live=None):
    """GPSIMUStateEstimator.cpp:77-100 (gps_imu_reference.align)"""
    n = att.shape[1]
    e3 = np.stack([np.zeros(n), np.zeros(n), np.ones(n)])
    expected = m_rotate(q_matrix(q_inv(att)), e3)
    nf = v_norm(meas_acc).astype(F).astype(D)
    unit = np.stack([meas_acc[0] / nf, meas_acc[1] / nf, meas_acc[2] / nf])
    cos_err = expected[0] * unit[0] + expected[1] * unit[1] + expected[2] * unit[2]
    ax = np.stack([unit[1] * expected[2] - unit[2] * expected[1], unit[2] * expected[0] - unit[0] * expected[2],
                   unit[0] * expected[1] - unit[1] * expected[0]])
    an = v_norm(ax)
    tilted = an > D(F(1e-6))
    d = np.where(tilted, an, 1.0)
    x_axis = np.zeros_like(ax)
    x_axis[0] = 1.0
    ax = np.where(tilted, np.stack([ax[0] / d, ax[1] / d, ax[2] / d]), x_axis)
    angle = math(2, cos_err)
    outside = np.abs(cos_err.astype(F)) > F(1)
    angle = np.where(outside, np.where(cos_err < 0, D(np.pi), 0.0), angle)
    if count is not None:
        live = np.ones(n, bool) if live is None else live
        count["first_predict_tilted"] += int((tilted & live).sum())
        count["first_predict_level"] += int((~tilted & live).sum())
        count["acos_domain_neg"] += int((outside & (cos_err < 0) & live).sum())
        count["acos_domain_pos"] += int((outside & ~(cos_err < 0) & live).sum())
    return q_mul(att, from_axis_angle(ax, angle, math))


# ---- the covariance, written out on its own (not through gps_imu_reference's functions: the CPU test that holds the two
# restatements equal would otherwise compare those with themselves).  Row by row, as the kernel forms them. ------------------
def _c_row(t, dt, nv, na):
    c = [t[j] + t[3 + j] * dt for j in range(3)]
    c += [((t[3 + m] + t[6] * nv[m][0]) + t[7] * nv[m][1]) + t[8] * nv[m][2] for m in range(3)]
    c += [(t[6] + t[7] * na[0][1]) + t[8] * na[0][2], (t[7] + t[6] * na[1][0]) + t[8] * na[1][2], (t[8] + t[6] * na[2][0]) + t[7] * na[2][1]]
    return c


def tainted(P):
    """vehicles whose covariance has an entry that is not finite (gps_imu_reference.tainted); P [9, 9, n]"""
    return ~np.isfinite(P).all((0, 1))


def predict_covariance(P, dt, nv, na):
    """F P F' of GPSIMUStateEstimator.cpp:195 in the order the definition fixes, NaN everywhere for a tainted P; P [9, 9, n]"""
    return np.where(tainted(P), np.nan, _predict_finite(P, dt, nv, na))


def _predict_finite(P, dt, nv, na):
    A = [P[6], P[7], P[8]]
    rows = []
    for i in range(3):
        rows.append(_c_row([P[i][j] + dt * P[3 + i][j] for j in range(9)], dt, nv, na))
    for i in range(3):
        rows.append(_c_row([((P[3 + i][j] + nv[i][0] * A[0][j]) + nv[i][1] * A[1][j]) + nv[i][2] * A[2][j] for j in range(9)], dt, nv, na))
    rows.append(_c_row([(A[0][j] + na[0][1] * A[1][j]) + na[0][2] * A[2][j] for j in range(9)], dt, nv, na))
    rows.append(_c_row([(A[1][j] + na[1][0] * A[0][j]) + na[1][2] * A[2][j] for j in range(9)], dt, nv, na))
    rows.append(_c_row([(A[2][j] + na[2][0] * A[0][j]) + na[2][1] * A[1][j] for j in range(9)], dt, nv, na))
    return np.array(rows)


def innovation(P, r):
    """:224-228 -> (S, det by cofactors along the first row, adj(S))"""
    a, b, c = P[0][0] + r, P[0][1] + 0.0, P[0][2] + 0.0
    d, e, f = P[1][0] + 0.0, P[1][1] + r, P[1][2] + 0.0
    g, h, i = P[2][0] + 0.0, P[2][1] + 0.0, P[2][2] + r
    adj = [[e * i - f * h, c * h - b * i, b * f - c * e], [f * g - d * i, a * i - c * g, c * d - a * f], [d * h - e * g, b * g - a * h, a * e - b * d]]
    det = (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g)
    return [[a, b, c], [d, e, f], [g, h, i]], det, adj


# the branch a call took, per vehicle (Estimator.last_branch; tests/test_gps_reference.py holds it to the reference's)
CALL_BRANCHES = ("first_predict", "predict", "measure_before_predict", "singular_nonfinite", "singular_tiny", "update", "reset")
NO_CALL = 255


class Estimator:
    """GPSIMUStateEstimator for n vehicles.  imu = Predict, measure = UpdateWithMeasurement."""

    def __init__(self, n, cfg=None, math=glibc_math):
        self.n, self.cfg, self.math = n, (default_config() if cfg is None else cfg), math
        self.count = {k: 0 for k in BRANCHES}
        self.pos, self.vel, self.ang_vel = np.zeros((3, n)), np.zeros((3, n)), np.zeros((3, n))
        self.att = np.zeros((4, n))
        self.cov = np.zeros((9, 9, n))
        self.corr = np.full((3, n), np.nan)
        self.t_predict, self.t_update = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        self.initialized = np.zeros(n, bool)
        self.num_resets = np.zeros(n, np.uint32)
        self.last_branch = np.full(n, NO_CALL, np.uint8)       # index into CALL_BRANCHES of the latest call's branch
        self._reset(np.ones(n, bool), 0)

    def _fresh_cov(self, who):
        c = self.cfg
        d = [c["init_sigma_pos"] * c["init_sigma_pos"]] * 3 + [c["init_sigma_vel"] * c["init_sigma_vel"]] * 3 + \
            [c["init_sigma_att"] * c["init_sigma_att"]] * 3
        self.cov[:, :, who] = 0.0
        for i in range(9):
            self.cov[i, i, who] = d[i]

    def _restart(self, who, pos):
        self.pos[:, who] = pos[:, who]
        self.vel[:, who] = 0.0
        self.ang_vel[:, who] = 0.0
        self.att[:, who] = np.array([[1.0], [0.0], [0.0], [0.0]])
        self._fresh_cov(who)

    def _reset(self, who, now_us):
        self.num_resets[who] += 1
        self.initialized[who] = False
        self._restart(who, np.zeros((3, self.n)))
        self.t_predict[who] = now_us
        self.t_update[who] = now_us

    def reset(self, now_us, first=0, count=None):
        who = np.zeros(self.n, bool)
        who[first:self.n if count is None else first + count] = True
        self._reset(who, now_us)
        self.last_branch = np.where(who, 6, NO_CALL).astype(np.uint8)

    def set_state(self, est=None, cov=None, corr=None, first=0):
        k = next(a for a in (est, cov, corr) if a is not None).shape[1]
        s = slice(first, first + k)
        if est is not None:
            self.pos[:, s], self.vel[:, s], self.att[:, s], self.ang_vel[:, s] = est[0:3], est[3:6], est[6:10], est[10:13]
        if cov is not None:
            self.cov[:, :, s] = np.asarray(cov).reshape(9, 9, k)
        if corr is not None:
            self.corr[:, s] = corr
        self.initialized[s] = True

    def state(self):
        return {"est": np.concatenate([self.pos, self.vel, self.att, self.ang_vel]), "cov": self.cov.reshape(81, self.n).copy(),
                "last_predict_us": self.t_predict.copy(), "last_update_us": self.t_update.copy(),
                "initialized": self.initialized.astype(np.uint8), "num_resets": self.num_resets.copy()}

    def imu(self, now_us, meas_acc, meas_gyro):
        with np.errstate(all="ignore"):
            self._imu(now_us, np.asarray(meas_acc, D), np.asarray(meas_gyro, D))

    def _imu(self, now_us, a, w):
        c, n = self.cfg, self.n
        first = ~self.initialized
        self.last_branch = np.where(first, 0, 1).astype(np.uint8)
        if first.any():                                          # :67-103
            self._reset(first, now_us)
            self.initialized[first] = True
            att = align(self.att, a, self.math, self.count, first)
            self.att[:, first] = att[:, first]
        go = ~first
        if not go.any():
            return
        self.count["predict"] += int(go.sum())
        dt = (np.uint64(now_us) - self.t_predict).astype(D) * 1e-6
        pos, vel, att = self.pos, self.vel, self.att
        R = q_matrix(att)
        ra = m_rotate(R, a)
        acc = np.stack([ra[0] + 0.0, ra[1] + 0.0, ra[2] + D(F(-9.81))])
        new_pos = np.stack([pos[k] + dt * vel[k] for k in range(3)])
        new_vel = np.stack([vel[k] + dt * acc[k] for k in range(3)])
        new_att = q_mul(att, from_rotvec(np.stack([dt * w[0], dt * w[1], dt * w[2]]), self.math, self.count, go))
        nv = [[dt * (+a[1] * R[3 * i + 2] - a[2] * R[3 * i + 1]), dt * (-a[0] * R[3 * i + 2] + a[2] * R[3 * i + 0]),
               dt * (+a[0] * R[3 * i + 1] - a[1] * R[3 * i + 0])] for i in range(3)]
        k = self.corr
        gx, gy, gz = dt * w[0] + k[0] / 2.0, dt * w[1] + k[1] / 2.0, dt * w[2] + k[2] / 2.0
        zero = np.zeros(n)
        na = [[zero, +gz, -gy], [-gz, zero, +gx], [+gy, -gx, zero]]
        C = predict_covariance(self.cov, dt, nv, na)
        for i in range(3):
            C[3 + i, 3 + i] = C[3 + i, 3 + i] + c["sigma_acc"] * c["sigma_acc"] * dt * dt
            C[6 + i, 6 + i] = C[6 + i, 6 + i] + c["sigma_gyro"] * c["sigma_gyro"] * dt * dt
        self.pos[:, go], self.vel[:, go], self.att[:, go], self.ang_vel[:, go] = new_pos[:, go], new_vel[:, go], new_att[:, go], w[:, go]
        self.cov[:, :, go] = C[:, :, go]
        self.corr[:, go] = 0.0
        self.t_predict[go] = now_us

    def measure(self, now_us, meas_pos):
        """-> vehicles that took the singular branch"""
        with np.errstate(all="ignore"):
            return self._measure(now_us, np.asarray(meas_pos, D))

    def _measure(self, now_us, z):
        c = self.cfg
        self.count["nan_position"] += int(np.isnan(z).any(0).sum())
        first = ~self.initialized
        self.count["measure_before_predict"] += int(first.sum())
        S, det, adj = innovation(self.cov, c["sigma_pos"] * c["sigma_pos"])
        finite = ~tainted(self.cov)
        for i in range(3):
            for j in range(3):
                finite &= np.isfinite(S[i][j])
        singular = ~first & ((np.abs(det) < 1e-10) | ~finite)
        self.count["singular_tiny"] += int((singular & finite).sum())
        self.count["singular_nonfinite"] += int((singular & ~finite).sum())
        go = ~first & ~singular
        self.count["update"] += int(go.sum())
        self.last_branch = np.where(first, 2, np.where(singular, np.where(finite, 4, 3), 5)).astype(np.uint8)
        r = 1 / det
        Si = [[adj[i][j] * r for j in range(3)] for i in range(3)]
        P = self.cov
        L = [[(P[i][0] * Si[0][j] + P[i][1] * Si[1][j]) + P[i][2] * Si[2][j] for j in range(3)] for i in range(9)]
        d = [z[k] - self.pos[k] for k in range(3)]
        dx = [(L[i][0] * d[0] + L[i][1] * d[1]) + L[i][2] * d[2] for i in range(9)]
        new_pos = np.stack([self.pos[k] + dx[k] for k in range(3)])
        new_vel = np.stack([self.vel[k] + dx[3 + k] for k in range(3)])
        corr = np.stack(dx[6:9])
        new_att = q_mul(self.att, from_rotvec(corr, self.math, self.count, go))
        C = np.array([[P[i][j] - ((L[i][0] * P[0][j] + L[i][1] * P[1][j]) + L[i][2] * P[2][j]) for j in range(9)] for i in range(9)])
        C = 0.5 * (C + C.transpose(1, 0, 2))
        self.pos[:, go], self.vel[:, go], self.att[:, go], self.corr[:, go] = new_pos[:, go], new_vel[:, go], new_att[:, go], corr[:, go]
        self.cov[:, :, go] = C[:, :, go]
        self.t_update[go] = now_us
        again = first | singular
        self.initialized[first] = True
        self._restart(again, z)
        return int(singular.sum())


class Sampler:
    """What the simulated vehicle's GetAccelerometer / GetRateGyro return (Quadcopter_T.hpp:75-82): _R * sample in float and a
    second-order low-pass each (QuadcopterLogic.hpp:40-52, :71-77), from the raw samples of afe_get_imu.  mounts: (yaw, pitch,
    roll) per type; types [n]; cutoffs in rad/s."""

    def __init__(self, n, period, mounts, types, gyro_cutoff, accel_cutoff=100.0):
        table = np.stack([ref.mount_matrix(*m) for m in mounts])
        self.R = table[np.asarray(types, int)]
        self.gyro = ref.LowPass3(n, period, np.asarray(gyro_cutoff, F)[np.asarray(types, int)])      # (a cutoff per type)
        self.acc = ref.LowPass3(n, period, accel_cutoff)

    def sample(self, gyro_raw, acc_raw):
        """one logic tick -> (meas_acc, meas_gyro) float64 [3, n]"""
        with np.errstate(all="ignore"):
            w = self.gyro.apply(ref.mount_rotate(self.R, gyro_raw) - F(0))
            a = self.acc.apply(ref.mount_rotate(self.R, acc_raw))
        return a.astype(D), w.astype(D)


# ---- the scripted call list --------------------------------------------------------------------------------------------------
# Reaches every branch of the definition a caller of the ABI can reach.  (The two acosf domain branches are not among them:
# Reset() at :68 makes the attitude the identity before :79-90, so cosAngleError is a component of a vector divided by its
# own float norm and |float(cosAngleError)| <= 1; tests/test_gps_estimator_cpu.py reaches them through align() itself.)
SCRIPT_BRANCHES = tuple(b for b in BRANCHES if not b.startswith("acos_domain"))
SCRIPT_MIN_N = 14
IMU_PERIOD_US = 2000


def make_script(n):
    """events: ("imu",), ("measure",), ("reset", first, count), ("set_state", kind, first, count).  The last vehicle is
    expected to have a NaN position throughout."""
    assert n == 1 or n >= SCRIPT_MIN_N
    period = [("imu",)] * 5 + [("measure",)]
    ev = period * 3                 # first Predict; the NaN correction poisons the covariance; the first update is singular
    if n >= SCRIPT_MIN_N:
        ev += [("reset", 2, 3), ("measure",)]                       # a measurement before any Predict: no alignment ever
        ev += [("imu",)] * 2
        ev += [("reset", 5, 2), ("imu",)]                           # a first Predict again
        ev += [("set_state", "tiny", 7, 2), ("set_state", "inf", 9, 1), ("set_state", "far", 10, 3), ("measure",)]
    else:
        ev += [("set_state", "tiny", 0, 1), ("measure",), ("set_state", "inf", 0, 1), ("measure",), ("set_state", "far", 0, 1), ("measure",)]
    ev += period * 8                 # (and past 100 ms, where the follower's scripted plans begin)
    if n >= 24:                      # the estimate a follower's tick behind the script is judged on: attitudes all over the sphere
        ev += [("set_state", "sphere", 0, n)] + period
    return ev


# ---- the phase groups: 0 to 5 ordinary Predicts between the alignment and the first measurement -----------------------------------
# A 500 Hz IMU and a 100 Hz GPS that start out of phase.  Vehicle v is in group (v + shift) % 6; group g is Reset() before
# every tick up to tick 6 - g (a Reset() leaves _lastMeasUpdateAttCorrection the NaN the constructor left, so the vehicle
# keeps aligning and makes no ordinary Predict), aligns for the last time at tick 6 - g, makes g ordinary Predicts and meets
# the measurement behind tick 6.  Groups 1 to 5 find a covariance the NaN correction has tainted and restart; group 0
# makes an ordinary update, which overwrites the correction.  Three offboard periods follow.
PHASE_GROUPS = 6
PHASE_FIRST_MEASURE = 11                                            # the index of that measurement in make_phase_script


def phase_group(n, shift=0):
    return (np.arange(n) + shift) % PHASE_GROUPS


def phase_ranges(n, shift, upto):
    """[(first, count)] covering the vehicles of groups 0 .. upto"""
    who = phase_group(n, shift) <= upto
    edges = np.flatnonzero(np.diff(np.concatenate([[0], who.astype(int), [0]])))
    return [(int(a), int(b - a)) for a, b in zip(edges[0::2], edges[1::2])]


def make_phase_script(n, shift=0):
    """events as make_script's, and ("reset_ranges", [(first, count), ...])"""
    ev = [("imu",)]
    for tick in range(2, PHASE_GROUPS + 1):
        ev += [("reset_ranges", phase_ranges(n, shift, PHASE_GROUPS - tick)), ("imu",)]
    ev += [("measure",)]
    assert len(ev) - 1 == PHASE_FIRST_MEASURE
    return ev + ([("imu",)] * 5 + [("measure",)]) * 3


# the single non-finite covariance entries: a diagonal and an off-diagonal place in each of the six blocks (pos/pos, pos/vel,
# pos/att, vel/vel, vel/att, att/att; the blocks below the diagonal by the transposed place), each with NaN, +Inf and -Inf
POISON_PLACES = ((0, 0), (1, 2), (0, 3), (4, 2), (1, 7), (8, 0), (4, 4), (3, 5), (5, 8), (6, 4), (7, 7), (8, 6))
POISON_VALUES = (np.nan, np.inf, -np.inf)
N_POISON = len(POISON_PLACES) * len(POISON_VALUES)


def payload(kind, count, near):
    """set_state's arrays: (est13, cov81, corr3).  near [3, count]: where the vehicles are, roughly"""
    rng = np.random.default_rng({"tiny": 1, "inf": 2, "far": 3, "sphere": 4, "poison": 5, "skew": 6}[kind])
    est = np.zeros((13, count))
    est[0:3] = np.where(np.isfinite(near), near, 0.0)
    est[6] = 1.0
    cov = np.zeros((9, 9, count))
    corr = np.zeros((3, count))
    if kind == "poison":                                            # a full finite covariance with ONE entry that is not finite
        A = rng.normal(size=(9, 9, count)) * 0.3
        cov = np.einsum("ikn,jkn->ijn", A, A)
        for i in range(9):
            cov[i, i] += 0.5
        for v in range(count):
            i, j = POISON_PLACES[(v // len(POISON_VALUES)) % len(POISON_PLACES)]
            cov[i, j, v] = POISON_VALUES[v % len(POISON_VALUES)]
    elif kind == "tiny":                                             # S = P[0:3][0:3] + 0.0625 I with a determinant of 1e-15
        for i in range(3):
            cov[i, i] = -0.0625 + 1e-5
            cov[3 + i, 3 + i] = 1.0
            cov[6 + i, 6 + i] = 0.01
    elif kind == "inf":
        for i in range(9):
            cov[i, i] = 1.0
        cov[0, 0] = np.inf
    elif kind == "sphere":                                          # the follower tests' states (follower_checker.make_state)
        from tests import follower_checker as fc
        _, vel, att = fc.make_state(count, 9)
        est[3:6], est[6:10] = vel * 0.3, att
        for i in range(9):
            cov[i, i] = 1.0 if i < 6 else 0.01
    else:                                                           # an estimate a metre off under a full covariance: every gain is alive
        A = rng.normal(size=(9, 9, count)) * 0.3
        cov = np.einsum("ikn,jkn->ijn", A, A)
        for i in range(9):
            cov[i, i] += 0.5
        est[0:3] += rng.uniform(0.5, 1.0, (3, count))
        est[3:6] = rng.normal(0, 0.5, (3, count))
        q = rng.normal(size=(4, count))
        est[6:10] = q / np.sqrt((q * q).sum(0)) * 1.001             # and an attitude that is not a unit quaternion
        est[10:13] = rng.normal(0, 0.2, (3, count))
        corr = rng.normal(0, 1e-3, (3, count))
        if kind == "skew":                                          # ... and a covariance that is not symmetric: 0.5 (C + C') of :256 acts
            B = rng.normal(size=(9, 9, count)) * 0.05
            cov = cov + (B - B.transpose(1, 0, 2))
    return est, cov.reshape(81, count), corr


def run_script(script, est, inputs, sampler=None):
    """inputs[k], by event: imu (now_us, acc, gyro) -- raw float32 samples when a Sampler is given, else what Predict is
    handed --, measure (now_us, pos), reset now_us, set_state near.  -> est.state() after every event, n singular per measure"""
    states, singular = [], {}
    for k, ev in enumerate(script):
        if ev[0] == "imu":
            now, a, w = inputs[k]
            if sampler is not None:
                a, w = sampler.sample(w, a)
            est.imu(now, a, w)
        elif ev[0] == "measure":
            singular[k] = est.measure(*inputs[k])
        elif ev[0] == "reset":
            est.reset(inputs[k], ev[1], ev[2])
            if sampler is not None:
                sampler.acc.reset(who=slice(ev[1], ev[1] + ev[2]))
        elif ev[0] == "reset_ranges":
            for first, count in ev[1]:
                est.reset(inputs[k], first, count)
                if sampler is not None:
                    sampler.acc.reset(who=slice(first, first + count))
        else:
            e13, c81, k3 = payload(ev[1], ev[3], inputs[k])
            est.set_state(e13, c81, k3, first=ev[2])
        states.append(est.state())
    return states, singular


def synthetic_inputs(script, n, seed=0):
    """a flight nobody flew: level vehicles (the first half) and tilted ones, some turning, the last with a NaN position"""
    rng = np.random.default_rng(seed)
    level = np.arange(n) < max(1, n // 2)
    pos = rng.uniform(-5, 5, (3, n))
    pos[:, n - 1] = np.nan if n > 1 else pos[:, n - 1]
    acc0 = np.where(level, np.array([[0.0], [0.0], [9.81]]), rng.normal(0, 4, (3, n)) + np.array([[0.0], [0.0], [9.0]]))
    gyro0 = np.where(np.arange(n) % 3 == 0, 0.0, rng.normal(0, 0.5, (3, n)))
    inputs, now = [], 0
    for ev in script:
        if ev[0] == "imu":
            now += IMU_PERIOD_US
            wob = np.where(level, 0.0, rng.normal(0, 0.05, (3, n)))
            inputs.append((now, (acc0 + wob).astype(F).astype(D), (gyro0 * (1 + wob)).astype(F).astype(D)))
        elif ev[0] == "measure":
            pos = pos + rng.normal(0, 0.01, (3, n))
            inputs.append((now, pos.copy()))
        elif ev[0] in ("reset", "reset_ranges"):
            inputs.append(now)
        else:
            inputs.append(pos[:, ev[2]:ev[2] + ev[3]].copy())
    return inputs
