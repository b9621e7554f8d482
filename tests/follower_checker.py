"""The trajectory follower's specification in numpy (agri-fly_amd/csrc/afe_follower.hip states it operation by
operation; this file restates it, and the two must give the same bits).

  double arithmetic   explicit left-to-right sums and products, no einsum, no dot: the order is the contract
  float arithmetic    float32 arrays throughout, in the reference's order (Offboard::QuadcopterController::RunTracking,
                      QuadcopterController.cpp:76-132; QuadcopterAttitudeController.hpp:35-68; Rotation.hpp), the radio
                      codec from tests/offboard_stub.py
  transcendentals     a parameter: math(op, x) with op 0..3 = sinf, cosf, asinf, acosf (float32 in and out) and
                      op 4 = acos (float64).  device_math(afa) asks the GPU (afe_follower_selftest_math), glibc_math
                      asks libm through ctypes, numpy_math numpy.

Arrays are planar: [components, n]."""
import ctypes as _C
import ctypes.util as _Cu

import numpy as np

from tests.offboard_stub import F, radio_quantise

D = np.float64
MIN_ANGLE = F(4.84813681e-6)
PI_F = F(np.pi)

_libm = _C.CDLL(_Cu.find_library("m") or "libm.so.6")
for _n in ("sinf", "cosf", "asinf", "acosf"):
    getattr(_libm, _n).restype = _C.c_float
    getattr(_libm, _n).argtypes = [_C.c_float]
_libm.acos.restype = _C.c_double
_libm.acos.argtypes = [_C.c_double]
_NAMES = ("sinf", "cosf", "asinf", "acosf", "acos")


def glibc_math(op, x):
    x = np.asarray(x, D if op == 4 else F)
    f = getattr(_libm, _NAMES[op])
    return np.array([f(float(v)) for v in x.reshape(-1)], x.dtype).reshape(x.shape)


def numpy_math(op, x):
    x = np.asarray(x, D if op == 4 else F)
    with np.errstate(all="ignore"):
        return (np.sin, np.cos, np.arcsin, np.arccos, np.arccos)[op](x).astype(x.dtype)


def device_math(afa, device=-1):
    return lambda op, x: afa.follower_selftest_math(op, x, device=device).reshape(np.shape(x))


def default_config():
    """afe_follower_default_config(5) without the library (MINIQUAD, derived in float as QuadcopterConstants.hpp:225-228)"""
    av_xy = F(0.04)
    return dict(period_us=10000, delay_us=30000, lookahead=0.04, omega_step=0.02, hover_thrust=9.81,
                mount=np.array([0.5, -0.5, 0.5, -0.5]), nat_freq=F(2.0), damping=F(0.7), tc_xy=av_xy * F(2), tc_z=(av_xy * F(5)) * F(2))


def config_from(cfg):
    """a FollowerConfig of the package -> the dict the functions below take"""
    return dict(period_us=int(cfg.period_us), delay_us=int(cfg.delay_us), lookahead=float(cfg.lookahead_s),
                omega_step=float(cfg.omega_step_s), hover_thrust=float(cfg.hover_thrust), mount=np.array(list(cfg.mount), D),
                nat_freq=F(cfg.nat_freq), damping=F(cfg.damping), tc_xy=F(cfg.att_time_const_xy), tc_z=F(cfg.att_time_const_z))


def ring_slots(period_us, delay_us):
    return delay_us // period_us + 2


# ---- Rotation.hpp / Vec3.hpp, any one dtype -------------------------------------------------------------------------------
def q_mul(a, b):
    """Rotation.hpp:124-131, this = a, r1 = b"""
    return np.stack([b[0] * a[0] - b[1] * a[1] - b[2] * a[2] - b[3] * a[3],
                     b[1] * a[0] + b[0] * a[1] + b[3] * a[2] - b[2] * a[3],
                     b[2] * a[0] - b[3] * a[1] + b[0] * a[2] + b[1] * a[3],
                     b[3] * a[0] + b[2] * a[1] - b[1] * a[2] + b[0] * a[3]])


def q_inv(q):
    return np.stack([q[0], -q[1], -q[2], -q[3]])


def q_matrix(q):
    """Rotation.hpp:196-220 -> [9, n]"""
    r0, r1, r2, r3 = q[0] * q[0], q[1] * q[1], q[2] * q[2], q[3] * q[3]
    return np.stack([r0 + r1 - r2 - r3, 2 * q[1] * q[2] - 2 * q[0] * q[3], 2 * q[1] * q[3] + 2 * q[0] * q[2],
                     2 * q[1] * q[2] + 2 * q[0] * q[3], r0 - r1 + r2 - r3, 2 * q[2] * q[3] - 2 * q[0] * q[1],
                     2 * q[1] * q[3] - 2 * q[0] * q[2], 2 * q[2] * q[3] + 2 * q[0] * q[1], r0 - r1 - r2 + r3])


def m_rotate(R, v):
    return np.stack([R[0] * v[0] + R[1] * v[1] + R[2] * v[2],
                     R[3] * v[0] + R[4] * v[1] + R[5] * v[2],
                     R[6] * v[0] + R[7] * v[1] + R[8] * v[2]])


def v_dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def v_cross(a, b):
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


# ---- planned_trajectory.hpp, coefficients [18, n]: row 3 k + axis = coeffs[k][axis] (t^5 .. t^0) ----------------------------
def _k(c, axis):
    return [c[3 * k + axis] for k in range(6)]


def poly_pos(c, t):
    out = []
    for a in range(3):
        k5, k4, k3, k2, k1, k0 = _k(c, a)
        out.append(((((k5 * t + k4) * t + k3) * t + k2) * t + k1) * t + k0)
    return np.stack(out)


def poly_vel(c, t):
    out = []
    for a in range(3):
        k5, k4, k3, k2, k1, _ = _k(c, a)
        out.append((((5 * k5 * t + 4 * k4) * t + 3 * k3) * t + 2 * k2) * t + k1)
    return np.stack(out)


def poly_acc(c, t):
    out = []
    for a in range(3):
        k5, k4, k3, k2, _, _ = _k(c, a)
        out.append(((20 * k5 * t + 12 * k4) * t + 6 * k3) * t + 2 * k2)
    return np.stack(out)


def traj_normal(c, g, t):
    f = poly_acc(c, t) - g
    return f / np.sqrt(v_dot(f, f))


def traj_omega(c, g, t, step, math, info=None):
    """planned_trajectory.hpp:30-39; +0 where |n0 x n1| <= 1e-6 or the dot product is not below 1"""
    n0, n1 = traj_normal(c, g, t), traj_normal(c, g, t + step)
    turn = v_cross(n0, n1)
    length = np.sqrt(v_dot(turn, turn))
    dot = v_dot(n0, n1)
    zero = (length <= 1e-6) | ~(dot < 1.0)
    rate = math(4, np.where(zero, 0.0, dot)) / step
    if info is not None:
        info["small_cross"], info["dot_ge_1"] = length <= 1e-6, ~(dot < 1.0)
    safe = np.where(zero, 1.0, length)
    return np.where(zero, 0.0, np.stack([rate * (turn[0] / safe), rate * (turn[1] / safe), rate * (turn[2] / safe)]))


def planner_inputs(pos, vel, att, prev_thrust, goal, mount):
    """main.cpp:490-495 and the goal vector, as the inputs kernel forms them"""
    n = pos.shape[1]
    with np.errstate(all="ignore"):
        cam = q_mul(att, np.tile(np.asarray(mount, D)[:, None], (1, n)))
        Mi, Ma = q_matrix(q_inv(cam)), q_matrix(att)
        aw = np.stack([Ma[2] * prev_thrust, Ma[5] * prev_thrust, Ma[8] * prev_thrust - 9.81])
        gw = np.stack([np.zeros(n), np.zeros(n), np.full(n, -9.81)])
        return dict(vel0=m_rotate(Mi, vel), acc0=m_rotate(Mi, aw), grav=m_rotate(Mi, gw), cost_vec=m_rotate(Mi, goal - pos), cam=cam)


def reference(att, plans, cfg, now_us, math, info=None):
    """main.cpp:558-608 -> ref14 [14, n]"""
    c, g = plans["coeffs"], plans["grav"]
    planned = plans["planned"].astype(bool)
    n = planned.size
    with np.errstate(all="ignore"):
        tt = (np.full(n, now_us, np.uint64) - plans["t_plan_us"].astype(np.uint64)).astype(D) * 1e-6
        tf = plans["tf"]
        running = planned & (tt < tf)
        te = np.where(running, tt + cfg["lookahead"], tf)
        p, v, araw = poly_pos(c, te), poly_vel(c, te), poly_acc(c, te)
        v = np.where(running, v, 0.0)
        a = np.where(running, araw, 0.0)
        behind = p[2] < 0
        if info is not None:
            info["clamp_neg"] = planned & behind & (v[2] < 0) & (a[2] < 0)
            info["clamp_pos"] = planned & behind & (v[2] > 0) & (a[2] > 0)
        v[2] = np.where(behind & (v[2] < 0), 0.0, v[2])
        a[2] = np.where(behind & (a[2] < 0), 0.0, a[2])
        p[2] = np.where(behind, 0.0, p[2])
        Mt = q_matrix(plans["traj_att"])
        ref_pos = m_rotate(Mt, p) + plans["offset"]
        ref_vel, ref_acc = m_rotate(Mt, v), m_rotate(Mt, a)
        d = araw - g
        thrust = np.sqrt(v_dot(d, d))
        om = traj_omega(c, g, te, cfg["omega_step"], math, info)
        ref_w = m_rotate(q_matrix(q_mul(q_inv(att), plans["traj_att"])), om)
    if info is not None:
        info["unplanned"], info["running"], info["finished"] = ~planned, running, planned & ~running
        info["small_cross"] &= planned
        info["dot_ge_1"] &= planned
    out = np.empty((14, n))
    out[0:3] = np.where(planned, ref_pos, plans["hold"])
    out[3:6] = np.where(planned, ref_vel, 0.0)
    out[6:9] = np.where(planned, ref_acc, 0.0)
    out[9] = np.where(planned, thrust, cfg["hover_thrust"])
    out[10:13] = np.where(planned, ref_w, 0.0)
    out[13] = running
    return out


def _tilt_angle(c, math):
    with np.errstate(all="ignore"):
        inner = math(3, np.where((c >= F(1)) | (c <= F(-1)) | np.isnan(c), F(0), c).astype(F)).astype(F)
    # a NaN cosine fails both comparisons and goes to acosf, which answers NaN
    return np.where(c >= F(1), F(0), np.where(c <= F(-1), PI_F, np.where(np.isnan(c), F(np.nan), inner))).astype(F)


def from_rotvec(r, math, info=None):
    """Rotation.hpp:84-97"""
    theta = np.sqrt(v_dot(r, r)).astype(F)
    small = theta < MIN_ANGLE
    th = np.where(small, F(1), theta).astype(F)
    half = (th * F(0.5)).astype(F)
    s, c = math(0, half).astype(F), math(1, half).astype(F)
    q = np.stack([c, s * (r[0] / th), s * (r[1] / th), s * (r[2] / th)]).astype(F)
    q[:, small] = np.array([[1], [0], [0], [0]], F)
    if info is not None:
        info["theta_small"] = small
    return q


def to_rotvec(q, math, info=None):
    """Rotation.hpp:144-161, the norm held at 1 for asinf (tests/offboard_stub.py)"""
    pos_w = q[0] > 0
    n = np.where(pos_w, q[1:4], -q[1:4]).astype(F)
    norm = np.sqrt(v_dot(n, n)).astype(F)
    angle = (math(2, np.where(norm < F(1), norm, F(1)).astype(F)).astype(F) * F(2)).astype(F)
    small = angle < MIN_ANGLE
    k = (angle / np.where(small, F(1), norm)).astype(F)
    out = np.where(small, F(0), n * k).astype(F)
    if info is not None:
        info["w_le_0"], info["rot_small"] = ~pos_w, small
    return out


def run_tracking(pos, vel, att, ref14, cfg, math, info=None):
    """RunTracking, desired yaw 0 -> (cmdThrust [n], cmdAngVel [3, n]) in double"""
    n = pos.shape[1]
    with np.errstate(all="ignore"):
        pf, vf, qf = pos.astype(F), vel.astype(F), att.astype(F)
        rp, rv = ref14[0:3].astype(F), ref14[3:6].astype(F)
        w, z = F(cfg["nat_freq"]), F(cfg["damping"])
        acc_err = (((rp - pf) * w) * w + (((rv - vf) * F(2)) * w) * z + F(0)).astype(F)
        e3 = np.zeros((3, n), F)
        e3[2] = 1
        bz = m_rotate(q_matrix(qf), e3).astype(F)
        cmd_thrust = ref14[9] + v_dot(acc_err, bz).astype(F).astype(D)
        gf = np.zeros((3, n), F)
        gf[2] = F(9.81)
        s = (ref14[6:9] + acc_err.astype(D)) + gf.astype(D)
        nrm = np.sqrt(v_dot(s, s)).astype(F)
        tdir = (s / nrm.astype(D)).astype(F)
        cos_a = v_dot(tdir, e3).astype(F)
        angle = _tilt_angle(cos_a, math)
        ax = v_cross(e3, tdir).astype(F)
        an = np.sqrt(v_dot(ax, ax)).astype(F)
        tiny = an < F(1e-6)
        finfo = {}
        k = (angle / np.where(tiny, F(1), an)).astype(F)
        ref_att = from_rotvec(np.stack([k * ax[0], k * ax[1], k * ax[2]]).astype(F), math, finfo)
        ref_att[:, tiny] = np.array([[1], [0], [0], [0]], F)
        ident = np.zeros((4, n), F)
        ident[0] = 1
        ref_att = q_mul(ref_att, ident).astype(F)
        err = q_mul(q_inv(ref_att), qf).astype(F)
        rot = to_rotvec(err, math, info)
        zb = m_rotate(q_matrix(q_inv(err)), e3).astype(F)
        rax = v_cross(zb, e3).astype(F)
        red = _tilt_angle(v_dot(zb, e3).astype(F), math)
        rn = np.sqrt(v_dot(rax, rax)).astype(F)
        rtiny = rn < F(1e-12)
        rax = np.where(rtiny, F(0), rax / np.where(rtiny, F(1), rn)).astype(F)
        k3, k12 = F(1) / F(cfg["tc_z"]), F(1) / F(cfg["tc_xy"])
        nk3, kr = -k3, ((k12 - k3) * red).astype(F)
        we = (nk3 * rot - kr * rax).astype(F)
        cmd_w = ref14[10:13] + we.astype(D)
    if info is not None:
        info["cos_ge_1"], info["cos_le_m1"], info["n_tiny"] = cos_a >= F(1), cos_a <= F(-1), tiny
        info["theta_small"] = finfo["theta_small"] & ~tiny
    return cmd_thrust, cmd_w


def tick(pos, vel, att, plans, cfg, now_us, math, info=None):
    """one offboard period for every vehicle -> dict(ref14, cmd_thrust (the new previous_thrust), computed [4, n], sent [4, n])"""
    ref14 = reference(att, plans, cfg, now_us, math, info)
    thrust, w = run_tracking(pos, vel, att, ref14, cfg, math, info)
    with np.errstate(all="ignore"):
        computed = np.concatenate([thrust[None], w]).astype(F)
    sent = radio_quantise(computed, 35)
    if info is not None:
        info["beyond_35"] = ~((computed > F(-35)) & (computed < F(35))).all(0)
    return dict(ref14=ref14, cmd_thrust=thrust, computed=computed, sent=sent)


class DelayLine:
    """CommunicationsDelay.hpp:18-33 looked at once per tick: AddMessage, then every message with due <= now in send order"""

    def __init__(self, delay_us):
        self.delay_us, self.queue = int(delay_us), []

    def tick(self, now_us, msg):
        """-> the newest message that is due, or None"""
        self.queue.append((now_us + self.delay_us, msg))
        out = None
        while self.queue and self.queue[0][0] <= now_us:
            out = self.queue.pop(0)[1]
        return out


BRANCHES = ("unplanned", "running", "finished", "clamp_neg", "clamp_pos", "small_cross", "dot_ge_1", "cos_ge_1", "cos_le_m1",
            "n_tiny", "w_le_0", "rot_small", "beyond_35")


N_SPECIAL = 12     # the hand-made vehicles of make_state / make_plans


def make_state(n, seed, far=None):
    """A state whose first N_SPECIAL vehicles are hand-made (make_plans says for what), random ones behind them.
    far = (first, count, metres): that group stands `metres` out along x.  -> pos [3, n], vel [3, n], att [4, n]"""
    assert n >= 2 * N_SPECIAL
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-5, 5, (3, n))
    pos[2] = rng.uniform(0.5, 3, n)
    vel = rng.uniform(-2, 2, (3, n))
    att = rng.normal(size=(4, n))
    att /= np.sqrt((att * att).sum(0))
    for i in (0, 1, 2, 3):                       # level and at rest
        att[:, i], vel[:, i] = (1.0, 0.0, 0.0, 0.0), 0.0
    att[:, 4], vel[:, 4] = (-1.0, 0.0, 0.0, 0.0), 0.0      # level with the sign flipped: quaternion w <= 0
    pos[2, 1] = 8.0                              # (a height from which make_plans' hold point is an exact float away)
    if far is not None:
        first, count, metres = far
        assert first >= N_SPECIAL
        pos[0, first:first + count] += metres
    return pos, vel, att


def make_plans(pos, seed, now_us):
    """Plans, hold points and goals for vehicles standing at pos (as the engine reports it) that, with make_state's
    attitudes and velocities, reach every branch of a tick at time now_us."""
    n = pos.shape[1]
    assert n >= 2 * N_SPECIAL and now_us >= 100000
    rng = np.random.default_rng(seed + 1000)
    planned = (rng.random(n) < 0.75).astype(np.uint8)
    coeffs = rng.uniform(-1, 1, (18, n)) * np.repeat([0.02, 0.05, 0.2, 0.5, 1.0, 0.3], 3)[:, None]
    tf = rng.uniform(0.01, 2.0 * now_us * 1e-6, n)                   # some finished, some running
    t_plan_us = rng.integers(0, now_us + 1, n).astype(np.uint64)
    traj_att = rng.normal(size=(4, n))
    traj_att /= np.sqrt((traj_att * traj_att).sum(0))
    offset = pos + rng.uniform(-0.3, 0.3, (3, n))
    grav = m_rotate(q_matrix(q_inv(traj_att)), np.stack([np.zeros(n), np.zeros(n), np.full(n, -9.81)]))
    hold = pos + rng.uniform(-1, 1, (3, n))
    goal = pos + rng.uniform(-20, 20, (3, n))

    def plan(i, z_coeffs, running=True):
        """a plan along the camera axis only, planned in the world frame with gravity (0, 0, -9.81)"""
        planned[i], coeffs[:, i] = 1, 0.0
        for k, val in z_coeffs.items():
            coeffs[3 * k + 2, i] = val
        tf[i] = 2.0 if running else 0.05
        t_plan_us[i] = now_us - 100000
        traj_att[:, i], offset[:, i], grav[:, i] = (1.0, 0.0, 0.0, 0.0), pos[:, i], (0.0, 0.0, -9.81)

    # 0: hovering exactly on its hold point: cosAngle >= 1, n < 1e-6, rotation below an arc second
    planned[0] = 0
    hold[:, 0] = pos[:, 0]
    # 1: hold 9.81f / 2 below: the proper acceleration is (0, 0, -9.81f) exactly, straight down: cosAngle <= -1
    planned[1] = 0
    hold[:, 1] = pos[:, 1] + np.array([0.0, 0.0, -float(F(9.81)) / 2])
    # 2: hold 100 m away: values beyond +35
    planned[2] = 0
    hold[:, 2] = pos[:, 2] + np.array([100.0, -100.0, 50.0])
    # 3: a tilt of 1e-5 rad: n >= 1e-6 but the cosine rounds to 1, FromRotationVector's own small-angle exit
    planned[3] = 0
    hold[:, 3] = pos[:, 3] + np.array([2.5e-5, 0.0, 0.0])
    # 4: (make_state) quaternion w <= 0; hold 100 m below: a thrust beyond -35
    planned[4] = 0
    hold[:, 4] = pos[:, 4] + np.array([0.0, 0.0, -100.0])
    # 5, 6: behind the camera, moving and accelerating backwards / forwards
    plan(5, {5: -1.0, 4: -1.0, 3: -1.0})
    plan(6, {5: -1.0, 4: 1.0, 3: 1.0})
    # 7: constant acceleration: n0 == n1, the cross product is zero and the dot product is not below 1
    plan(7, {3: 0.5, 4: 0.2, 5: 0.1})
    # 8: a thrust direction that turns by 5e-7 rad per step: small cross product, dot product below 1
    plan(8, {5: 0.1})
    coeffs[3 * 2 + 0, 8] = 4e-5
    # 9: finished (position held at the end, velocity and acceleration zero)
    plan(9, {2: 0.05, 3: 0.3, 4: 0.5, 5: 0.1}, running=False)
    # 10: planned in the future: the time difference wraps, the plan counts as finished
    plan(10, {4: 0.5, 5: 0.1})
    t_plan_us[10] = now_us + 5
    # 11: running, turning fast
    plan(11, {1: 0.3, 2: -0.8, 3: 1.0, 4: 0.5, 5: 0.2})
    coeffs[3 * 2 + 1, 11] = 2.0
    return dict(planned=planned, coeffs=coeffs, tf=tf, t_plan_us=t_plan_us, traj_att=traj_att, offset=offset, grav=grav, hold=hold,
                goal=goal)


def make_cases(n, seed, now_us, far=None):
    """-> dict(pos, vel, att, plans)"""
    pos, vel, att = make_state(n, seed, far)
    return dict(pos=pos, vel=vel, att=att, plans=make_plans(pos, seed, now_us))


def same_bits(a, b):
    """equal as bit patterns (so -0 and +0 differ, and a NaN equals itself)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    u = {4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize]
    return bool(np.array_equal(a.view(u), b.view(u)))


def code_distance(sent_a, sent_b):
    """radio codes apart, per value (one code is 35 / 32768)"""
    step = 35.0 / 32768.0
    return np.rint(np.abs(sent_a.astype(D) - sent_b.astype(D)) / step).astype(np.int64)
