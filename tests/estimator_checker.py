"""The mocap state estimator's specification in numpy, vectorised over vehicles (test infrastructure).  cli/mocap_estimator.hpp
is the definition, tests/offboard_reference.py the same in scalar Python; agri-fly_amd/csrc/afe_estimator.hip follows it line
by line on the device, and this file restates it for whole ensembles.  All three must give the same bits.

  arithmetic        float64 arrays, explicit left-to-right sums and products in the order of the C++ lines: the order is
                    the contract
  transcendentals   a parameter: math(op, x), op 0..4 = sin, cos, asin, acos, exp (float64 in and out).  device_math(afa)
                    asks the GPU (afe_estimator_selftest_math), glibc_math asks libm through ctypes, numpy_math numpy;
                    nudged(math, ulps) moves every result by so many ulps (how far does one ulp carry?)
  the pipe          one list of messages for the ensemble (every vehicle is announced to in the same call).  Ring(slots)
                    keeps the newest `slots` and refuses by the rule of csrc/afe_estimator_ring.h, mirrored here;
                    Deque() keeps everything and forgets per vehicle as ClearExpiredMessages does.

Arrays are planar: [components, n].  Times are integer microseconds since the estimator was made."""
import ctypes as _C
import ctypes.util as _Cu

import numpy as np

D = np.float64
TICK = 1e-6
MIN_ANGLE = 4.84813681e-6
MAX_SLOTS = 16

_libm = _C.CDLL(_Cu.find_library("m") or "libm.so.6")
_NAMES = ("sin", "cos", "asin", "acos", "exp")
for _n in _NAMES:
    getattr(_libm, _n).restype = _C.c_double
    getattr(_libm, _n).argtypes = [_C.c_double]


def glibc_math(op, x):
    x = np.asarray(x, D)
    f = getattr(_libm, _NAMES[op])
    return np.array([f(float(v)) for v in x.reshape(-1)], D).reshape(x.shape)


def numpy_math(op, x):
    with np.errstate(all="ignore"):
        return (np.sin, np.cos, np.arcsin, np.arccos, np.exp)[op](np.asarray(x, D))


def device_math(afa, device=-1):
    return lambda op, x: afa.estimator_selftest_math(op, x, device=device).reshape(np.shape(x))


def nudged(math, ulps=1):
    """every transcendental result moved `ulps` ulps up"""
    def f(op, x):
        y = math(op, x)
        for _ in range(ulps):
            y = np.nextafter(y, np.inf)
        return y
    return f


def default_config():
    """afe_estimator_default_config without the library"""
    return dict(command_delay_s=0.03, rate_time_constant_s=0.04, gate=6.0, sigma_pos=0.02, sigma_att=5 * np.pi / 180,
                sigma_acc=1.0 * 9.81, sigma_ang_acc=200.0, offboard_period_us=10000, max_measure_gap_us=10000)


def config_from(cfg):
    """an EstimatorConfig of the package -> the dict the classes below take"""
    return {k: (int if k.endswith("_us") else float)(getattr(cfg, k)) for k in default_config()}


# ---- the ring's rule, mirrored from csrc/afe_estimator_ring.h ------------------------------------------------------------------
def ring_slots(cfg):
    """(ceil(delay * 1e6) + 2 * max gap) / period + 3; None where the header refuses (period 0, more than 16)"""
    if cfg["offboard_period_us"] == 0:
        return None
    delay_us = int(np.ceil(cfg["command_delay_s"] * 1e6))
    k = (delay_us + 2 * cfg["max_measure_gap_us"]) // cfg["offboard_period_us"] + 3
    return None if k > MAX_SLOTS else int(k)


class Refused(Exception):
    """AFE_ERR_OUT_OF_RANGE of an announce"""


class Ring:
    """EstimatorRing: message k in slot k % slots; need = the measure call before the last, held down by a reset until two
    measure calls have passed"""

    def __init__(self, slots):
        self.slots, self.msgs = int(slots), []           # msgs: every message ever announced (from, acc, ang_vel); the ring is its tail
        self.t_last = self.t_prev = 0
        self.reset_pending, self.reset_floor, self.calls_since_reset = True, 0, 0

    def need_us(self):
        return self.reset_floor if self.reset_pending and self.reset_floor < self.t_prev else self.t_prev

    def measured(self, t_us, valid_us, first):
        self.t_prev, self.t_last = self.t_last, t_us
        if self.reset_pending:
            self.calls_since_reset += 1
            if self.calls_since_reset >= 2:
                self.reset_pending = False

    def was_reset(self, t_us):
        if not self.reset_pending:
            self.reset_floor = t_us
        self.reset_pending, self.calls_since_reset = True, 0

    def accepts(self, from_s):
        seq = len(self.msgs)
        if seq > 0 and not from_s > self.msgs[-1][0]:
            return False
        if seq >= self.slots:
            successor = self.msgs[seq - self.slots + 1][0]
            if not successor <= self.need_us() * 1e-6 - TICK:
                return False
        return True

    def lowest(self, n):
        """per vehicle, the oldest message that can still be looked at"""
        return np.full(n, max(0, len(self.msgs) - self.slots), np.int64)


class Deque:
    """PredictionPipe as it is: nothing is ever refused or overwritten; ClearExpiredMessages per vehicle (PredictionPipe.hpp:57-68)"""

    def __init__(self):
        self.msgs, self.front, self.fronts_differed = [], None, False

    def measured(self, t_us, valid_us, first):
        """first: the vehicles whose first measurement this was -- UpdateWithMeasurement returns before it clears anything"""
        if self.front is None:
            self.front = np.zeros(valid_us.size, np.int64)
        at = valid_us.astype(D) * 1e-6
        total = len(self.msgs)
        frm = np.array([m[0] for m in self.msgs] + [np.inf, np.inf])
        for _ in range(total):
            pop = ~first & (total - self.front >= 2) & (frm[np.minimum(self.front + 1, total)] <= at)
            self.front = self.front + pop
        self.fronts_differed |= bool(self.front.min() < self.front.max())

    def was_reset(self, t_us):
        pass

    def accepts(self, from_s):
        return True

    def lowest(self, n):
        return np.zeros(n, np.int64) if self.front is None else self.front


# ---- Rotation.hpp / Vec3.hpp -----------------------------------------------------------------------------------------------------
def q_mul(a, b):
    """Rotation.hpp:124-131, this = a, r1 = b"""
    return np.stack([b[0] * a[0] - b[1] * a[1] - b[2] * a[2] - b[3] * a[3],
                     b[1] * a[0] + b[0] * a[1] + b[3] * a[2] - b[2] * a[3],
                     b[2] * a[0] - b[3] * a[1] + b[0] * a[2] + b[1] * a[3],
                     b[3] * a[0] + b[2] * a[1] - b[1] * a[2] + b[0] * a[3]])


def q_inv(q):
    return np.stack([q[0], -q[1], -q[2], -q[3]])


def v_norm(v):
    return np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def from_rotvec(r, math, small_out=None):
    """Rotation.hpp:84-97"""
    theta = v_norm(r)
    small = theta < MIN_ANGLE
    th = np.where(small, 1.0, theta)
    half = th * 0.5
    s, c = math(0, half), math(1, half)
    q = np.stack([c, s * (r[0] / th), s * (r[1] / th), s * (r[2] / th)])
    q[:, small] = np.array([[1.0], [0.0], [0.0], [0.0]])
    if small_out is not None:
        small_out.append(small)
    return q


def to_rotvec(q, math, small_out=None):
    """Rotation.hpp:144-161"""
    pos_w = q[0] > 0
    n = np.where(pos_w, q[1:4], -q[1:4])
    norm = v_norm(n)
    angle = math(2, norm) * 2
    small = angle < MIN_ANGLE
    k = angle / np.where(small, 1.0, norm)
    if small_out is not None:
        small_out.append(small)
    return np.where(small, 0.0, np.stack([n[0] * k, n[1] * k, n[2] * k]))


def _grow(V, h, s):
    """F V F' + Q, the dense product's operand order (MocapStateEstimator.cpp:157-172)"""
    vv, vr, rv, rr = V
    a, b = 1 * vv + h * rv, 1 * vr + h * rr
    c, d = 0 * vv + 1 * rv, 0 * vr + 1 * rr
    return [(a * 1 + b * h) + h * h * h * h * s / 4, (a * 0 + b * 1) + 0, (c * 1 + d * h) + 0, (c * 0 + d * 1) + h * h * s]


def _shrink(V, g0, g1):
    """(I - g [1 0]) V   (:236-242)"""
    vv, vr, rv, rr = V
    a, b, c, d = 1 - g0 * 1, 0 - g0 * 0, 0 - g1 * 1, 1 - g1 * 0
    return [a * vv + b * rv, a * vr + b * rr, c * vv + d * rv, c * vr + d * rr]


def _symmetrise(V):
    vv, vr, rv, rr = V
    return [(vv + vv) * 0.5, (vr + rv) * 0.5, (rv + vr) * 0.5, (rr + rr) * 0.5]


BRANCHES = ("init", "accept", "reject", "forced_reset", "ballistic", "none_active_yet", "one_trip", "two_trip", "overshoot",
            "theta_small", "angle_small", "nan_gate")


class Estimator:
    """MocapEstimator of cli/mocap_estimator.hpp for n vehicles.  pipe: Ring(slots) or Deque()."""

    def __init__(self, n, cfg, math, pipe):
        self.n, self.cfg, self.math, self.pipe = n, cfg, math, pipe
        self.count = {k: 0 for k in BRANCHES}
        self.rejected = np.zeros(n, np.uint32)
        self.row = np.zeros(n, np.uint32)
        self.max_trips = 0
        self._reset(np.ones(n, bool), 0, first=True)

    # -- state ------------------------------------------------------------------------------------------------------------
    def _reset(self, who, wall_us, first=False):
        if first:
            n = self.n
            self.x, self.v, self.w, self.q = np.zeros((3, n)), np.zeros((3, n)), np.zeros((3, n)), np.zeros((4, n))
            self.P, self.A = [np.zeros(n) for _ in range(4)], [np.zeros(n) for _ in range(4)]
            self.valid, self.started = np.zeros(n, np.uint64), np.zeros(n, bool)
        self.x[:, who], self.v[:, who], self.w[:, who] = 0.0, 0.0, 0.0
        self.q[:, who] = np.array([[1.0], [0.0], [0.0], [0.0]])
        self._fresh(who)
        self.valid[who] = wall_us
        self.started[who] = False

    def _fresh(self, who):
        for V, vv, rr in ((self.P, 25.0, 25.0), (self.A, 1.0, 400.0)):
            V[0][who], V[1][who], V[2][who], V[3][who] = vv, 0.0, 0.0, rr

    def reset(self, wall_us, first=0, count=None):
        who = np.zeros(self.n, bool)
        who[first:self.n if count is None else first + count] = True
        self._reset(who, wall_us)
        self.pipe.was_reset(wall_us)

    def state(self):
        """as afe_estimator_get_state reports it"""
        return dict(est=np.concatenate([self.x, self.v, self.q, self.w]),
                    cov=np.stack([self.P[0], self.P[1], self.P[3], self.A[0], self.A[1], self.A[3]]),
                    valid_at_us=self.valid.copy(), started=self.started.astype(np.uint8), rejected_in_a_row=self.row.copy(),
                    rejected=self.rejected.copy())

    # -- the pipe -----------------------------------------------------------------------------------------------------------
    def announce(self, wall_us, ang_vel, acc):
        from_s = wall_us * 1e-6 + self.cfg["command_delay_s"]
        if not self.pipe.accepts(from_s):
            raise Refused(from_s)
        self.pipe.msgs.append((from_s, np.array(acc, D), np.array(ang_vel, D)))

    def _active(self, t, live):
        """PredictionPipe.hpp:33-55 -> acc, ang_vel, free_fall, span, from (of the active message)"""
        n, msgs = self.n, self.pipe.msgs
        lo = self.pipe.lowest(n)
        idx, span, frm = np.full(n, -1, np.int64), np.full(n, 1e10), np.zeros(n)
        nxt = 1e10
        for j in range(len(msgs) - 1, int(lo.min()) - 1, -1):
            ok = (idx < 0) & (j >= lo) & ((t + TICK) >= msgs[j][0])
            span, frm, idx = np.where(ok, nxt - msgs[j][0], span), np.where(ok, msgs[j][0], frm), np.where(ok, j, idx)
            nxt = msgs[j][0]
        acc, w = np.zeros((3, n)), np.zeros((3, n))
        for j in np.unique(idx[idx >= 0]):
            m = idx == j
            acc[:, m], w[:, m] = msgs[j][1][:, m], msgs[j][2][:, m]
        free = idx < 0
        self.count["ballistic"] += int((free & live).sum())
        if msgs:
            self.count["none_active_yet"] += int((free & live & (len(msgs) > lo)).sum())
        return acc, w, free, span, frm

    # -- UpdateWithMeasurement -------------------------------------------------------------------------------------------------
    def measure(self, wall_us, pos, att):
        """-> measurements rejected by this call"""
        cfg, math, n = self.cfg, self.math, self.n
        pos, att = np.asarray(pos, D), np.asarray(att, D)
        with np.errstate(all="ignore"):
            init = ~self.started
            run = self.started.copy()
            self.count["init"] += int(init.sum())
            now = D(wall_us) * 1e-6
            go = run & (now > self.valid.astype(D) * 1e-6)
            trips = np.zeros(n, np.int64)
            while True:
                at = self.valid.astype(D) * 1e-6
                go = go & ~((at + TICK) >= now)
                if not go.any():
                    break
                acc, cmd, free, span, frm = self._active(at, go)
                h = now - at
                cut = h > (span + TICK)
                h = np.where(cut, span, h)
                self.count["overshoot"] += int((go & cut & ((at - frm) > TICK)).sum())
                x0, v0, w0, q0 = self.x, self.v, self.w, self.q
                x1 = np.stack([x0[k] + v0[k] * h for k in range(3)])
                v1 = np.stack([v0[k] + acc[k] * h for k in range(3)])
                small = []
                q1 = q_mul(q0, from_rotvec(np.stack([w0[k] * h for k in range(3)]), math, small))
                self.count["theta_small"] += int((go & small[0]).sum())
                keep = np.where(free, 1.0, math(4, np.where(go, -h / cfg["rate_time_constant_s"], 0.0)))
                w1 = np.stack([keep * w0[k] + (1 - keep) * cmd[k] for k in range(3)])
                self.x, self.v, self.w, self.q = (np.where(go, x1, x0), np.where(go, v1, v0), np.where(go, w1, w0), np.where(go, q1, q0))
                step = (0.5 + np.where(go, h, 0.0) * 1e6).astype(np.uint64)
                self.valid = np.where(go, self.valid + step, self.valid).astype(np.uint64)
                P1, A1 = _grow(self.P, h, cfg["sigma_acc"]), _grow(self.A, h, cfg["sigma_ang_acc"])
                self.P = [np.where(go, a, b) for a, b in zip(P1, self.P)]
                self.A = [np.where(go, a, b) for a, b in zip(A1, self.A)]
                trips += go
                assert trips.max() <= len(self.pipe.msgs) + 2, "the propagation does not end"
            self.count["one_trip"] += int((trips == 1).sum())
            self.count["two_trip"] += int((trips == 2).sum())
            self.max_trips = max(self.max_trips, int(trips.max()))
            sp2, sa2 = cfg["sigma_pos"] * cfg["sigma_pos"], cfg["sigma_att"] * cfg["sigma_att"]
            sP, sA = self.P[0] + sp2, self.A[0] + sa2
            ex = pos - self.x
            dP = v_norm(ex) / np.sqrt(3 * sP)
            r0 = q_mul(q_inv(att), self.q)[0]
            dA = math(3, np.abs(r0)) * 2.0 / np.sqrt(sA)
            outlier = (dP > cfg["gate"]) | (dA > cfg["gate"])
            reject = run & outlier & (self.row < 10)
            update = run & ~reject
            forced = update & (self.row >= 10)
            self.count["reject"] += int(reject.sum())
            self.count["accept"] += int(update.sum())
            self.count["forced_reset"] += int(forced.sum())
            self.count["nan_gate"] += int((update & (np.isnan(dP) | np.isnan(dA))).sum())
            self.rejected = np.where(reject, self.rejected + 1, self.rejected).astype(np.uint32)
            self.row = np.where(reject, self.row + 1, np.where(update, 0, self.row)).astype(np.uint32)
            if forced.any():
                self._reset(forced, wall_us)
                sP, sA = self.P[0] + sp2, self.A[0] + sa2
            gP0, gP1 = self.P[0] * (1 / sP), self.P[2] * (1 / sP)
            gA0, gA1 = self.A[0] * (1 / sA), self.A[2] * (1 / sA)
            ex = pos - self.x
            x1 = np.stack([self.x[k] + gP0 * ex[k] for k in range(3)])
            v1 = np.stack([self.v[k] + gP1 * ex[k] for k in range(3)])
            small_a, small_t = [], []
            ea = to_rotvec(q_mul(q_inv(self.q), att), math, small_a)
            q1 = q_mul(self.q, from_rotvec(np.stack([gA0 * ea[k] for k in range(3)]), math, small_t))
            w1 = np.stack([self.w[k] + gA1 * ea[k] for k in range(3)])
            self.count["angle_small"] += int((update & small_a[0]).sum())
            self.count["theta_small"] += int((update & small_t[0]).sum())
            P1, A1 = _shrink(self.P, gP0, gP1), _shrink(self.A, gA0, gA1)
            self.x, self.v, self.w, self.q = (np.where(update, x1, self.x), np.where(update, v1, self.v), np.where(update, w1, self.w),
                                              np.where(update, q1, self.q))
            P1 = [np.where(update, a, b) for a, b in zip(P1, self.P)]
            A1 = [np.where(update, a, b) for a, b in zip(A1, self.A)]
            self.P = [np.where(run, a, b) for a, b in zip(_symmetrise(P1), self.P)]
            self.A = [np.where(run, a, b) for a, b in zip(_symmetrise(A1), self.A)]
            # the first measurement: the state is the measurement, nothing else happens (no Symmetrise, no ClearExpiredMessages)
            if init.any():
                self.x[:, init], self.q[:, init] = pos[:, init], att[:, init]
                self.v[:, init], self.w[:, init] = 0.0, 0.0
                self._fresh(init)
                self.started[init] = True
        self.pipe.measured(wall_us, self.valid, init)
        return int(reject.sum())

    # -- GetPrediction -------------------------------------------------------------------------------------------------------------
    def predict(self, wall_us, ahead):
        """-> [13, n]: position 3, velocity 3, attitude 4, body rates 3; the state is not touched"""
        cfg, math, n = self.cfg, self.math, self.n
        with np.errstate(all="ignore"):
            until = ahead + D(wall_us) * 1e-6
            t = self.valid.astype(D) * 1e-6
            x, v, q, w = self.x, self.v, self.q, self.w
            trips = np.zeros(n, np.int64)
            while True:
                go = (t + TICK) < until
                if not go.any():
                    break
                acc, cmd, free, span, frm = self._active(t, go)
                h = until - t
                cut = h > (span + TICK)
                h = np.where(cut, span, h)
                self.count["overshoot"] += int((go & cut & ((t - frm) > TICK)).sum())
                x1 = np.stack([x[k] + self.v[k] * h + acc[k] * h * h / 2 for k in range(3)])         # sic: the filter's own velocity
                v1 = np.stack([v[k] + acc[k] * h for k in range(3)])
                q1 = q_mul(q, from_rotvec(np.stack([self.w[k] * h for k in range(3)]), math))        # sic: the filter's own rate
                keep = np.where(free, 1.0, math(4, np.where(go, -h / cfg["rate_time_constant_s"], 0.0)))
                w1 = np.stack([keep * w[k] + (1 - keep) * cmd[k] for k in range(3)])
                x, v, q, w = np.where(go, x1, x), np.where(go, v1, v), np.where(go, q1, q), np.where(go, w1, w)
                t = np.where(go, t + h, t)
                trips += go
                assert trips.max() <= len(self.pipe.msgs) + 2, "the prediction does not end"
            self.max_trips = max(self.max_trips, int(trips.max()))
        return np.concatenate([x, v, q, w])


def announced(att, thrust, ang_vel):
    """what an attached tick announces (main.cpp:647-649): (cmdAngVel, att * e3 * cmdThrust - (0, 0, 9.81)), all double;
    att [4, n], thrust [n], ang_vel [3, n] -> (ang_vel, acc)"""
    from tests.follower_checker import m_rotate, q_matrix
    n = att.shape[1]
    e3 = np.stack([np.zeros(n), np.zeros(n), np.ones(n)])
    with np.errstate(all="ignore"):
        up = m_rotate(q_matrix(att), e3)
        return ang_vel, np.stack([up[0] * thrust - 0.0, up[1] * thrust - 0.0, up[2] * thrust - 9.81])


# ---- the scripted flight -----------------------------------------------------------------------------------------------------------
N_CALLS = 40
GAPS_MS = (3, 5, 7)
JUMP_CALL, NAN_CALL = 12, 5
REST, NAN_POS, Q0_ABOVE_1 = 0, 1, 2
TELEPORTED, ROTATED = slice(3, 7), slice(7, 11)
N_SPECIAL = 11
PREDICT_EVERY = 10


def script_config():
    cfg = default_config()
    cfg["max_measure_gap_us"] = 1000 * max(GAPS_MS)
    return cfg


def _rot(axis_angle):
    """quaternions of rotation vectors [3, n] (setup, not part of the contract)"""
    th = np.sqrt((axis_angle * axis_angle).sum(0))
    k = np.where(th > 0, np.sin(th / 2) / np.where(th > 0, th, 1.0), 0.5)
    return np.stack([np.cos(th / 2), axis_angle[0] * k, axis_angle[1] * k, axis_angle[2] * k])


def make_script(n, seed, far=None):
    """40 measure calls 3, 5 and 7 ms apart, an announce every 10 ms from 1 ms after the second call, a predict after every
    tenth call.  -> dict(events, pos [40, 3, n], att [40, 4, n], ang_vel / acc [announces, 3, n]); events are ("step", ms),
    ("measure", call), ("announce", k), ("predict", call) in the order they happen.  far = (first, count, metres): that
    group flies `metres` out along x.

      vehicle 0      exactly at rest, identity attitude, zero commands: theta < MIN_ANGLE and angle < MIN_ANGLE
      vehicle 1      its position is NaN from call 5 on
      vehicle 2      at rest with |q0| one float ulp above 1: acos gives NaN, and NaN passes the gate
      vehicles 3-6   teleported 4 m at call 12: ten rejections, then the forced reset
      vehicles 7-10  rotated by 2 rad at call 12: the attitude gate, the same way"""
    assert n >= 2 * N_SPECIAL
    rng = np.random.default_rng(seed)
    t_meas, t = [], 0
    for c in range(N_CALLS):
        t += GAPS_MS[c % len(GAPS_MS)]
        t_meas.append(t)
    t_ann = list(range(t_meas[1] + 1, t_meas[-1], 10))
    events, now, k = [], 0, 0
    for c, tm in enumerate(t_meas, 1):
        while k < len(t_ann) and t_ann[k] < tm:
            events += [("step", t_ann[k] - now), ("announce", k)]
            now, k = t_ann[k], k + 1
        events += [("step", tm - now), ("measure", c)]
        now = tm
        if c % PREDICT_EVERY == 0:
            events.append(("predict", c))
    n_ann = k
    p0 = rng.uniform(-5, 5, (3, n))
    p0[2] = rng.uniform(0.5, 3, n)
    v0 = rng.uniform(-1.5, 1.5, (3, n))
    amp, phase = rng.uniform(0, 0.2, (3, n)), rng.uniform(0, 6.28, (3, n))
    tilt, tphase = rng.uniform(-0.3, 0.3, (3, n)), rng.uniform(0, 6.28, (3, n))
    if far is not None:
        first, count, metres = far
        assert first >= N_SPECIAL
        p0[0, first:first + count] += metres
    pos, att = np.empty((N_CALLS, 3, n)), np.empty((N_CALLS, 4, n))
    turn = _rot(np.array([[0.0], [0.0], [2.0]]))
    for c, tm in enumerate(t_meas, 1):
        s = tm * 1e-3
        p = p0 + v0 * s + amp * np.sin(3.0 * s + phase)
        q = _rot(tilt * np.sin(4.0 * s + tphase))
        p[:, REST], q[:, REST] = p0[:, REST], (1.0, 0.0, 0.0, 0.0)
        p[:, Q0_ABOVE_1], q[:, Q0_ABOVE_1] = p0[:, Q0_ABOVE_1], (float(np.nextafter(np.float32(1), np.float32(2))), 0.0, 0.0, 0.0)
        if c >= NAN_CALL:
            p[:, NAN_POS] = np.nan
        if c >= JUMP_CALL:
            p[0, TELEPORTED] += 4.0
            q[:, ROTATED] = q_mul(q[:, ROTATED], np.tile(turn, (1, 4)))
        pos[c - 1], att[c - 1] = p, q
    ang_vel, acc = rng.uniform(-0.5, 0.5, (n_ann, 3, n)), rng.uniform(-1.0, 1.0, (n_ann, 3, n))
    ang_vel[:, :, REST], acc[:, :, REST] = 0.0, 0.0
    ang_vel[:, :, Q0_ABOVE_1], acc[:, :, Q0_ABOVE_1] = 0.0, 0.0
    return dict(events=events, pos=pos, att=att, ang_vel=ang_vel, acc=acc, t_meas_ms=t_meas, t_ann_ms=t_ann[:n_ann])


def run_script(script, est, truth=None):
    """the script through a checker.  truth: {call: (pos, att)} replaces the script's poses (what an engine reported).
    -> dict(states {call: state()}, predictions {call: [13, n]}, n_rejected {call: int})"""
    out = dict(states={}, predictions={}, n_rejected={})
    now_ms = 0
    for kind, arg in script["events"]:
        if kind == "step":
            now_ms += arg
        elif kind == "announce":
            est.announce(now_ms * 1000, script["ang_vel"][arg], script["acc"][arg])
        elif kind == "measure":
            pos, att = (script["pos"][arg - 1], script["att"][arg - 1]) if truth is None else truth[arg]
            out["n_rejected"][arg] = est.measure(now_ms * 1000, pos, att)
            out["states"][arg] = est.state()
        else:
            out["predictions"][arg] = est.predict(now_ms * 1000, 0.03)
    return out


def drift(a, b):
    """the largest |difference| between two results of run_script, per kind: est (the states' and the predictions' 13
    values; a value that is NaN in both counts as equal), cov; valid_at_us and the counters must be equal"""
    out = {"est": 0.0, "cov": 0.0}
    with np.errstate(all="ignore"):
        for c in a["states"]:
            sa, sb = a["states"][c], b["states"][c]
            for k in ("valid_at_us", "started", "rejected_in_a_row", "rejected"):
                assert np.array_equal(sa[k], sb[k]), (c, k)
            for k in ("est", "cov"):
                assert np.array_equal(np.isnan(sa[k]), np.isnan(sb[k])), (c, k)
                out[k] = max(out[k], float(np.nanmax(np.abs(sa[k] - sb[k]))))
        for c in a["predictions"]:
            pa, pb = a["predictions"][c], b["predictions"][c]
            assert np.array_equal(np.isnan(pa), np.isnan(pb)), c
            out["est"] = max(out["est"], float(np.nanmax(np.abs(pa - pb))))
    return out


def same_bits(a, b):
    """equal as bit patterns (so -0 and +0 differ, and a NaN equals itself)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    u = {4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize]
    return bool(np.array_equal(a.view(u), b.view(u)))
