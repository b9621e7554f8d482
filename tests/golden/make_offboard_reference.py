"""tests/golden/offboard_reference.npz: what the REFERENCE's own offboard controller, safety net and prediction pipe computed
(oracle/_ref/offboard_probe: QuadcopterController.cpp, SafetyNet.hpp and PredictionPipe.hpp compiled where they lie), on the
populations below, with the values of sinf / cosf / asinf / acosf / acos that the recording machine's libm gave while the checkers
reproduced those outputs bit for bit.

    python tests/golden/make_offboard_reference.py     # needs oracle/_ref/offboard_probe (built where the reference is)

The file holds numbers only.  What is in it:

  trk_*   RunTracking on 130 vehicles of follower_checker.make_state (the 12 hand-made ones, attitudes all over the sphere)
          and 32 near-level ones (tilt below 2 degrees), all float-representable so that an fp32 engine holds the same
          state.  The tracking reference ref14 is follower_checker.reference's on make_plans(pos, SEED, NOW_US): the plans
          are not stored, the tests make them again and must arrive at the stored ref14.
  run_*   Run on 130 vehicles, true doubles, with the hand-placed edges of make_run_population.
  msn_*   Run inside a teacher-forced mission of the stage machine (traj_id 5: no sin or cos in front of the controller):
          the trk states are put in before every tick, stages_checker.tick forms the controller's inputs, the reference's
          Run answers.  The inputs are not stored; a SHA-256 of their bytes per tick is, and the tests form them again.
  net_*   SafetyNet on faces, corners, the height rule, the timeout and NaNs; every value exactly a float.
  pipe_*  a script of AddMessage / timer advance / GetActiveMessage / ClearExpiredMessages.
  tab_*   the function table: per function the argument bits (sorted) and the result bits libm gave.  table_math looks an
          argument up by its bits and fails by name on one that is not there.

The seed of the capped populations: SEED below.  The radio-code cap (at most 1 % of the sent values differ from the
reference's, each by one code) is judged on the CPU with numpy's functions standing in for "another library's"; seeds 1..8
were looked at (python tests/golden/make_offboard_reference.py --seeds), all eight pass it on both sphere populations and
on the mission (at most 1 of 520 and 3 of 2 080 codes, each one code), and the first, 1, was taken.

Also the loader and the helpers the two test files share (tests/test_offboard_reference.py on the CPU,
tests/test_gpu_offboard_reference.py on the device); the tests never run the probe except to check staleness."""
import hashlib
import io
import os
import struct
import subprocess
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import follower_checker as fc          # noqa: E402
from tests import stages_checker as sc            # noqa: E402
from tests.offboard_stub import radio_quantise    # noqa: E402

FIXTURE = os.path.join(HERE, "offboard_reference.npz")
PROBE = os.path.join(ROOT, "oracle", "_ref", "offboard_probe")
MAGIC = 0x31464f52                                 # "ROF1"
D, F = np.float64, np.float32
N_SPHERE, N_LEVEL = 130, 32
N_TRK = N_SPHERE + N_LEVEL
N_RUN = 130
SEED = 1                                           # see the module's text; SEEDS_LOOKED_AT in that order
SEEDS_LOOKED_AT = (1, 2, 3, 4, 5, 6, 7, 8)
NOW_US = 200000                                    # the follower's tick: the engine has stepped 200 ms
SIZE_LIMIT = 81658                                 # tests/golden/rigid_body_reference.npz

# ---- the function table -------------------------------------------------------------------------------------------------------
TABLE_NAMES = ("sinf", "cosf", "asinf", "acosf", "acos", "sin", "cos")
_FOLLOWER_OPS = ("sinf", "cosf", "asinf", "acosf", "acos")                 # follower_checker's math(op, x)
_STAGES_OPS = ("sin", "cos", "sinf", "cosf", "asinf", "acosf")             # stages_checker's


def _is_double(name):
    return not name.endswith("f")


def _glibc(name, x):
    if name in _FOLLOWER_OPS:
        return fc.glibc_math(_FOLLOWER_OPS.index(name), x)
    return sc.glibc_math(_STAGES_OPS.index(name), x)


class Recorder:
    """glibc_math that remembers every (function, argument bits) -> result bits it was asked for"""

    def __init__(self):
        self.seen = {k: {} for k in TABLE_NAMES}

    def call(self, name, x):
        x = np.asarray(x, D if _is_double(name) else F)
        y = _glibc(name, x)
        u = np.uint64 if _is_double(name) else np.uint32
        for a, r in zip(np.ascontiguousarray(x).reshape(-1).view(u), np.ascontiguousarray(y).reshape(-1).view(u)):
            self.seen[name][int(a)] = int(r)
        return y

    def follower(self):
        return lambda op, x: self.call(_FOLLOWER_OPS[op], x)

    def stages(self):
        return lambda op, x: self.call(_STAGES_OPS[op], x)

    def arrays(self):
        out = {}
        for name in TABLE_NAMES:
            u = np.uint64 if _is_double(name) else np.uint32
            keys = sorted(self.seen[name])
            out["tab_%s_arg" % name] = np.array(keys, u)
            out["tab_%s_res" % name] = np.array([self.seen[name][k] for k in keys], u)
        return out


class MissingArgument(KeyError):
    """a restatement asked for a function value at an argument the table does not hold: it evaluated another argument than
    the checkers did when the table was recorded"""


class Table:
    def __init__(self, fx):
        self.arg = {k: fx["tab_%s_arg" % k] for k in TABLE_NAMES}
        self.res = {k: fx["tab_%s_res" % k] for k in TABLE_NAMES}

    def call(self, name, x, missing_is_nan=False):
        dt = D if _is_double(name) else F
        u = np.uint64 if _is_double(name) else np.uint32
        x = np.ascontiguousarray(np.asarray(x, dt))
        bits = x.reshape(-1).view(u)
        arg, res = self.arg[name], self.res[name]
        at = np.minimum(np.searchsorted(arg, bits), max(arg.size - 1, 0))
        found = (arg[at] == bits) if arg.size else np.zeros(bits.size, bool)
        if not found.all() and not missing_is_nan:
            bad = x.reshape(-1)[~found][0]
            raise MissingArgument("%s(%r) [bits 0x%x] is not in the recorded function table" % (name, float(bad), int(bits[~found][0])))
        out = np.where(found, res[at] if arg.size else 0, 0).astype(u).view(dt)
        if missing_is_nan:
            out = np.where(found, out, dt(np.nan)).astype(dt)
        return out.reshape(x.shape)

    def follower(self):
        return lambda op, x: self.call(_FOLLOWER_OPS[op], x)

    def stages(self):
        return lambda op, x: self.call(_STAGES_OPS[op], x)

    def first_entry_libm_misses(self):
        """-> None where this machine's libm gives every recorded result, else a string naming the first that differs"""
        for name in TABLE_NAMES:
            dt = D if _is_double(name) else F
            u = np.uint64 if _is_double(name) else np.uint32
            if not self.arg[name].size:
                continue
            got = np.ascontiguousarray(_glibc(name, self.arg[name].view(dt))).view(u)
            bad = np.flatnonzero(got != self.res[name])
            if bad.size:
                k = bad[0]
                return "%s(%r): recorded 0x%x, this libm 0x%x" % (name, float(self.arg[name].view(dt)[k]), int(self.res[name][k]), int(got[k]))
        return None


# ---- the probe ---------------------------------------------------------------------------------------------------------------
def run_probe(probe, request):
    """the probe twice on the same request: the bytes must be identical"""
    outs = []
    for _ in range(2):
        r = subprocess.run([probe], input=request, stdout=subprocess.PIPE)
        assert r.returncode == 0, r.returncode
        outs.append(r.stdout)
    assert outs[0] == outs[1], "the probe gave different bytes on the same request"
    return outs[0]


def _head(mode, n):
    return struct.pack("<3i", MAGIC, mode, n)


def _body(ans, mode, n):
    assert struct.unpack("<3i", ans[:12]) == (MAGIC, mode, n)
    return ans[12:]


def controller_params(cfg):
    """SetParameters' four doubles, from the float-derived values of default_config"""
    return [float(cfg["nat_freq"]), float(cfg["damping"]), float(cfg["tc_xy"]), float(cfg["tc_z"])]


def probe_run(probe, cfg, pos, vel, att, des_pos, des_vel, des_acc, yaw):
    """-> thrust [n], rates [3, n] (float64)"""
    n = pos.shape[1]
    rec = np.concatenate([pos, vel, att, des_pos, des_vel, des_acc, np.asarray(yaw, D)[None]]).T.astype("<f8")
    ans = _body(run_probe(probe, _head(0, n) + np.array(controller_params(cfg), "<f8").tobytes() + rec.tobytes()), 0, n)
    out = np.frombuffer(ans, "<f8").reshape(n, 4)
    return out[:, 0].copy(), out[:, 1:4].T.copy()


def probe_run_tracking(probe, cfg, pos, vel, att, ref14):
    """-> thrust [n], rates [3, n] (float64), cmd_att [4, n] (float32)"""
    n = pos.shape[1]
    rec = np.concatenate([pos, vel, att, ref14[0:9], np.zeros((1, n)), ref14[9:13]]).T.astype("<f8")
    ans = _body(run_probe(probe, _head(1, n) + np.array(controller_params(cfg), "<f8").tobytes() + rec.tobytes()), 1, n)
    out = np.frombuffer(ans, np.dtype([("d", "<f8", 4), ("q", "<f4", 4)]))
    return out["d"][:, 0].copy(), out["d"][:, 1:4].T.copy(), out["q"].T.copy()


def probe_safety_net(probe, cfg, pos, att, since, fresh, set_unsafe):
    """-> [n, 5] uint8: vehicleNotSeen, unsafePosition, upsideDownAndLow, userUnsafe, GetIsSafe()"""
    n = pos.shape[1]
    rec = np.zeros(n, np.dtype([("d", "<f8", 8), ("i", "<i4", 2)]))
    rec["d"] = np.concatenate([pos, att, np.asarray(since, D)[None]]).T
    rec["i"] = np.stack([fresh, set_unsafe]).T
    corners = np.concatenate([cfg["min_corner"], cfg["max_corner"], [cfg["min_normal_height"]]]).astype("<f8")
    ans = _body(run_probe(probe, _head(2, n) + corners.tobytes() + rec.tobytes()), 2, n)
    return np.frombuffer(ans, np.uint8).reshape(n, 5).copy()


PIPE_OP = np.dtype([("op", "<i4"), ("id", "<i4"), ("ballistic", "<i4"), ("pad", "<i4"), ("advance_us", "<i8"), ("t", "<f8")])
PIPE_OUT = np.dtype([("found", "<i4"), ("id", "<i4"), ("ballistic", "<i4"), ("size", "<i4"), ("remaining", "<f8")])
ADD, ADVANCE, GET, CLEAR = range(4)


def probe_pipe(probe, delay, ops):
    ans = _body(run_probe(probe, _head(3, len(ops)) + struct.pack("<d", delay) + ops.tobytes()), 3, len(ops))
    return np.frombuffer(ans, PIPE_OUT).copy()


# ---- populations ---------------------------------------------------------------------------------------------------------------
def _f32(a):
    """rounded to float and widened again: what an fp32 engine holds is the same number"""
    return np.asarray(a, D).astype(F).astype(D)


def make_tracking_population(seed):
    """-> pos [3, 162], vel [3, 162], att [4, 162], float-representable; the first 130 are make_state's"""
    pos, vel, att = fc.make_state(N_SPHERE, seed)
    rng = np.random.default_rng(seed + 500)
    pl = rng.uniform(-5, 5, (3, N_LEVEL))
    pl[2] = rng.uniform(0.5, 3, N_LEVEL)
    vl = rng.uniform(-2, 2, (3, N_LEVEL))
    tilt, heading = np.radians(rng.uniform(0.0, 2.0, N_LEVEL)), rng.uniform(0, 2 * np.pi, N_LEVEL)
    al = np.stack([np.cos(tilt / 2), np.sin(tilt / 2) * np.cos(heading), np.sin(tilt / 2) * np.sin(heading), np.zeros(N_LEVEL)])
    return _f32(np.concatenate([pos, pl], 1)), _f32(np.concatenate([vel, vl], 1)), _f32(np.concatenate([att, al], 1))


def tilt_degrees(att):
    with np.errstate(all="ignore"):
        bz = fc.m_rotate(fc.q_matrix(att), np.stack([np.zeros(att.shape[1]), np.zeros(att.shape[1]), np.ones(att.shape[1])]))[2]
        return np.degrees(np.arccos(np.clip(bz / np.sqrt((att * att).sum(0)), -1, 1)))


def _norm_f(x, y, z):
    x, y, z = F(x), F(y), F(z)
    return np.sqrt(x * x + y * y + z * z)


def _scan(start, count):
    """`count` consecutive floats either side of start"""
    up, down = [F(start)], [F(start)]
    for _ in range(count):
        up.append(np.nextafter(up[-1], F(np.inf)))
        down.append(np.nextafter(down[-1], F(-np.inf)))
    return np.array(down[:0:-1] + up, F)


# the hand-made vehicles of the Run population (make_state's own hand-made ones stand at 0..4; 0 is used as it is)
RUN_HOVER, RUN_NORM, RUN_Z, RUN_THRUST, RUN_INVERTED, RUN_YAW = 0, slice(12, 17), slice(17, 22), slice(22, 24), 24, slice(25, 30)
RUN_FAR = slice(30, 40)


def make_run_population(seed):
    """-> dict(pos, vel, att, des_pos, des_vel, des_acc [.., 130], yaw [130]), true doubles.  Hand-made:
      0         level, at rest on its desired position, nothing asked for: cosAngle >= 1, n < 1e-6
      12..16    on the desired position at rest, a desired acceleration along x such that |properAcc| is 20 - 2 ulp, 20 - 1 ulp,
                20, 20 + 1 ulp, 20 + 2 ulp (float ulps of 20): the saturation's comparison on either side
      17..21    the same way, properAcc.z at float(4.905) - 2 ulp .. + 2 ulp: the floor's comparison on either side
      22, 23    asking for hover, tilted about x until the thrust is the float just above -1, and just below it
      24        inverted, asking for hover
      25..29    yaw 0, +pi, -pi (the doubles), 4 and -7
      30..39    20 to 60 m from the desired position: saturation on ordinary inputs
    Every third vehicle from 40 on asks for no velocity, no acceleration and no yaw (what OffboardHover can express)."""
    n = N_RUN
    pos, vel, att = fc.make_state(n, seed + 1)
    rng = np.random.default_rng(seed + 2000)
    des_pos = pos + rng.uniform(-3, 3, (3, n))
    des_vel, des_acc, yaw = rng.uniform(-1, 1, (3, n)), rng.uniform(-2, 2, (3, n)), rng.uniform(-3, 3, n)
    plain = np.arange(n) % 3 == 1
    plain[:40] = False
    des_vel[:, plain], des_acc[:, plain], yaw[plain] = 0.0, 0.0, 0.0
    des_pos[:, RUN_FAR] = pos[:, RUN_FAR] + rng.uniform(20, 60, (3, 10)) * rng.choice([-1.0, 1.0], (3, 10))
    des_vel[:, 30:35], des_acc[:, 30:35], yaw[30:35] = 0.0, 0.0, 0.0

    def still(i):
        vel[:, i], des_vel[:, i], des_acc[:, i], yaw[i] = 0.0, 0.0, 0.0, 0.0
        des_pos[:, i] = pos[:, i]

    still(RUN_HOVER)
    g = F(9.81)
    # |(x, 0, 9.81f)| around 20
    xs = _scan(np.sqrt(400.0 - float(g) ** 2), 40)
    norms = np.array([_norm_f(x, 0, g) for x in xs], F)
    want = [F(20)]
    for _ in range(2):
        want = [np.nextafter(want[0], F(0))] + want + [np.nextafter(want[-1], F(np.inf))]
    for i, target in zip(range(12, 17), want):
        hit = np.flatnonzero(norms == target)
        assert hit.size, "no x gives the norm %r" % target
        still(i)
        des_acc[0, i] = float(xs[hit[0]])
    # properAcc.z = float(daz + 9.81f) around float(4.905), with properAcc.x = 1
    half = F(0.5 * 9.81)
    zs = _scan(float(half) - float(g), 40)
    got = (zs + g).astype(F)
    want = [half]
    for _ in range(2):
        want = [np.nextafter(want[0], F(0))] + want + [np.nextafter(want[-1], F(np.inf))]
    for i, target in zip(range(17, 22), want):
        hit = np.flatnonzero(got == target)
        assert hit.size, "no z gives %r" % target
        still(i)
        des_acc[0, i], des_acc[2, i] = 1.0, float(zs[hit[0]])
    # thrust = 9.81f * (R e3).z just above and just below -1
    th = np.arccos(-1.0 / float(g)) + np.linspace(-2e-5, 2e-5, 4001)
    qa = np.stack([np.cos(th / 2), np.sin(th / 2), np.zeros_like(th), np.zeros_like(th)])
    z3 = np.zeros((3, th.size))
    with np.errstate(all="ignore"):                          # the checker's own thrust line (no function of libm is in it)
        thrust = sc.run_position(z3, z3, qa, z3, z3, z3, np.zeros(th.size), sc.default_config(), sc.numpy_math)[0]
    above, below = np.flatnonzero(thrust > -1.0), np.flatnonzero(thrust <= -1.0)
    assert above.size and below.size
    i_above, i_below = above[np.argmin(thrust[above])], below[np.argmax(thrust[below])]
    for i, k in ((22, i_above), (23, i_below)):
        still(i)
        att[:, i] = qa[:, k]
    still(RUN_INVERTED)
    att[:, RUN_INVERTED] = (0.0, 1.0, 0.0, 0.0)
    yaw[RUN_YAW] = (0.0, np.pi, -np.pi, 4.0, -7.0)
    return dict(pos=pos, vel=vel, att=att, des_pos=des_pos, des_vel=des_vel, des_acc=des_acc, yaw=yaw)


def run_expressible_by_hover(p):
    """the Run records OffboardHover.controller can express: desired velocity and acceleration 0, yaw 0"""
    return (p["des_vel"] == 0).all(0) & (p["des_acc"] == 0).all(0) & (p["yaw"] == 0)


# ---- the mission -----------------------------------------------------------------------------------------------------------------
MISSION_DT_US = (100000, 20000, 60000, 20000, 60000, 120000, 20000, 200000, 20000, 100000)
MISSION_START, MISSION_STOP = (0,), (7,)
MISSION_RECORDED = (4, 5, 7, 9)       # Takeoff at 3/8 of its time, Takeoff's last tick, Flight with yaw, Landing under way
MISSION_STAGE_BEFORE = (sc.WAIT, sc.SPOOLUP, sc.SPOOLUP, sc.TAKEOFF, sc.TAKEOFF, sc.TAKEOFF, sc.FLIGHT, sc.FLIGHT, sc.LANDING, sc.LANDING)


def mission_config():
    cfg = sc.default_config(traj_id=5)
    cfg.update(spool_up_time=0.04, takeoff_time=0.16, get_into_action_time=0.32)
    return cfg


def mission_desired(n):
    return sc.desired_for(n)[0]


def fly_mission(pos, vel, att, math, on_run=None):
    """the teacher-forced mission through stages_checker.tick: the same state is put in before every tick.  on_run(k, inputs)
    is handed what tick k gives QuadcopterController::Run: (des_pos, des_vel, des_acc, yaw).  -> list per tick of
    dict(now_us, stage_before, fields after the tick, inputs, thrust, rates)"""
    n = pos.shape[1]
    cfg = mission_config()
    st = sc.new_state(n, cfg)
    st["desired_pos"] = mission_desired(n)
    out, now = [], 0
    orig = sc.run_position
    seen = {}

    def capture(p, v, q, dp, dv, da, yaw, c, m, info=None):
        thrust, rates = orig(p, v, q, dp, dv, da, yaw, c, m, info)
        seen.update(inputs=(np.array(dp, D), np.array(dv, D), np.array(da, D), np.array(yaw, D)), thrust=thrust, rates=rates)
        return thrust, rates

    sc.run_position = capture
    try:
        for k, dt_us in enumerate(MISSION_DT_US):
            now += dt_us
            before = st["stage"].copy()
            sc.tick(st, cfg, now, pos, vel, att, np.zeros(n), k in MISSION_START, k in MISSION_STOP, math)
            out.append(dict(now_us=now, stage_before=before, fields={f: np.array(st[f]) for f in sc.GET_FIELDS}, **seen))
            if on_run is not None:
                on_run(k, seen["inputs"])
    finally:
        sc.run_position = orig
    return out


def inputs_digest(inputs):
    h = hashlib.sha256()
    for a in inputs:
        h.update(np.ascontiguousarray(a, "<f8").tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


# ---- the safety net --------------------------------------------------------------------------------------------------------------
def make_safety_population():
    """-> dict(pos [3, n], att [4, n], since [n], fresh [n], set_unsafe [n], gpu [n]); every value exactly a float.  gpu: the rows
    an engine without an estimator can be put in (since == 0; everything else the ABI reaches)"""
    cfg = sc.default_config()
    lo, hi = cfg["min_corner"], cfg["max_corner"]
    level, inverted = (1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0)
    h = float(F(np.sqrt(0.5)))
    on_edge = (h, h, 0.0, 0.0)                      # (att e3).z = h h - h h = 0 exactly
    rows = []

    def row(pos, att=level, since=0.0, set_unsafe=0):
        rows.append((tuple(float(x) for x in pos), att, float(since), 1, set_unsafe))

    for axis in range(3):
        for corner, outward in ((lo, -1.0), (hi, 1.0)):
            c = F(corner[axis])
            assert float(c) == corner[axis]
            for v in (np.nextafter(c, F(-outward * np.inf)), c, np.nextafter(c, F(outward * np.inf))):     # inside, on, outside
                p = [0.0, 0.0, 1.0]
                p[axis] = float(v)
                row(p)
    row((lo[0], lo[1], lo[2]))                       # exactly on two corners
    row((hi[0], hi[1], hi[2]))
    hmin = F(cfg["min_normal_height"])
    for z in (hmin, np.nextafter(hmin, F(-np.inf))):  # exactly at the height, and the float below it
        for q in (inverted, on_edge, level):
            row((0.0, 0.0, float(z)), att=q)
    timeout = F(cfg["not_seen_timeout"])
    row((0.0, 0.0, 1.0), since=timeout)
    row((0.0, 0.0, 1.0), since=np.nextafter(timeout, F(np.inf)))
    row((0.0, 0.0, 1.0), since=0.625)
    row((np.nan, 0.0, 1.0))
    row((np.nan, np.nan, np.nan), since=np.nan)      # every comparison is false
    row((0.0, 0.0, 1.0), since=np.nan)
    row((0.0, 0.0, 1.0), set_unsafe=1)
    row((150.0, 0.0, -1.0), att=inverted, since=1.0, set_unsafe=1)     # all four
    rows.append(((0.0, 0.0, 1.0), level, 0.0, 0, 0))  # not fresh: userUnsafe stays from the row before
    pos = np.array([r[0] for r in rows]).T
    att = np.array([r[1] for r in rows]).T
    since = np.array([r[2] for r in rows])
    fresh, set_unsafe = np.array([r[3] for r in rows], np.int32), np.array([r[4] for r in rows], np.int32)
    for a in (pos, att, since):
        assert fc.same_bits(_f32(a), np.asarray(a, D))
    gpu = (since == 0) & (fresh == 1)
    return dict(pos=pos, att=att, since=since, fresh=fresh, set_unsafe=set_unsafe, gpu=gpu)


# ---- the pipe's script -------------------------------------------------------------------------------------------------------------
PIPE_DELAY = 0.03


def make_pipe_script():
    """-> ops (PIPE_OP).  Times of ClearExpiredMessages are whole microseconds times 1e-6 (what a restatement on an integer
    clock can be asked)."""
    ops, clock = [], [0]

    def add(i, ballistic=0):
        ops.append((ADD, i, ballistic, 0, 0, 0.0))
        return clock[0] * 1e-6 + PIPE_DELAY

    def advance(us):
        clock[0] += us
        ops.append((ADVANCE, 0, 0, 0, us, 0.0))

    def get(t):
        ops.append((GET, 0, 0, 0, 0, float(t)))

    def clear(t_us):
        ops.append((CLEAR, 0, 0, 0, 0, t_us * 1e-6))

    get(0.0)                                         # empty
    clear(0)
    advance(1000)
    ta0 = add(0)
    get(0.01)                                        # messages, none active
    edge = ta0 - 1e-6
    for t in (np.nextafter(edge, -np.inf), edge, np.nextafter(edge, np.inf), ta0):
        get(t)
    clear(40000)                                     # one message: it stays
    advance(10000)
    ta1 = add(1)
    advance(10000)
    ta2 = add(2, ballistic=1)
    for t in (0.0311, ta1, 0.045, ta2 - 1e-6, 0.06):  # oldest, middle, middle, newest, newest
        get(t)
    assert ta1 == 41000 * 1e-6, "pick times at which timeActive is a whole microsecond"
    clear(41000)                                     # _messages[1].timeActive == currentTime: the front goes
    get(0.045)
    get(0.0311)                                      # before what is left: nothing is active any more
    clear(45000)                                     # _messages[1] is not due: nothing goes
    # two announces 10 ms apart with 30 ms of delay, as the estimator's script has them
    advance(79000)
    ta3 = add(3)
    advance(10000)
    ta4 = add(4)
    for us in (105000, 129999, 130000, 135000, 139999, 140000, 150000):
        get(us * 1e-6)
    clear(135000)
    get(0.135)
    clear(140000)
    get(0.135)
    get(0.15)
    clear(1000000)                                   # everything is due: all go but the last, which always stays
    clear(2000000)                                   # one message left
    get(2.0)
    assert ta3 < ta4
    return np.array(ops, PIPE_OP)


# ---- the fixture -----------------------------------------------------------------------------------------------------------------
def _same(a, b):
    """bit for bit; a NaN equals any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        both = np.isnan(a) & np.isnan(b)
        return fc.same_bits(np.where(both, 0, a).astype(a.dtype), np.where(both, 0, b).astype(b.dtype))
    return bool(np.array_equal(a, b))


same = _same


def code_differences(sent_a, sent_b):
    """-> (how many of the sent values differ, of how many, the largest distance in codes)"""
    dist = fc.code_distance(sent_a, sent_b)
    return int(np.count_nonzero(dist)), int(dist.size), int(dist.max())


def sent_of(thrust, rates):
    with np.errstate(all="ignore"):
        return radio_quantise(np.concatenate([np.asarray(thrust)[None], rates]).astype(F), 35)


def make_offboard_reference(probe=PROBE, seed=SEED, verbose=False):
    rec = Recorder()
    fx = dict(seed=np.int64(seed), now_us=np.int64(NOW_US), n_sphere=np.int32(N_SPHERE), n_level=np.int32(N_LEVEL))
    # RunTracking
    fcfg = fc.default_config()
    pos, vel, att = make_tracking_population(seed)
    plans = fc.make_plans(pos, seed, NOW_US)
    info = {}
    t = fc.tick(pos, vel, att, plans, fcfg, NOW_US, rec.follower(), info)
    ref14 = t["ref14"]
    thrust, rates, cmd_att = probe_run_tracking(probe, fcfg, pos, vel, att, ref14)
    with np.errstate(all="ignore"):
        want_w = np.stack([t["computed"][k].astype(D) for k in range(1, 4)])
    chk_thrust, chk_rates = fc.run_tracking(pos, vel, att, ref14, fcfg, rec.follower())
    assert _same(chk_thrust, thrust) and _same(chk_rates, rates), "follower_checker.run_tracking differs from the reference: that is the finding"
    assert _same(chk_thrust, t["cmd_thrust"]) and _same(chk_rates.astype(F).astype(D), want_w)
    fx.update(trk_pos=pos.astype(F), trk_vel=vel.astype(F), trk_att=att.astype(F), trk_ref14=ref14, trk_thrust=thrust, trk_rates=rates,
              trk_cmd_att=cmd_att)
    names = fc.BRANCHES + ("theta_small",)
    fx["trk_branch"] = np.packbits(np.stack([np.asarray(info[k], bool) for k in names]), axis=1)
    # Run
    scfg = sc.default_config()
    p = make_run_population(seed)
    rinfo = {}
    chk_thrust, chk_rates = sc.run_position(p["pos"], p["vel"], p["att"], p["des_pos"], p["des_vel"], p["des_acc"], p["yaw"], scfg, rec.stages(), rinfo)
    thrust, rates = probe_run(probe, scfg, p["pos"], p["vel"], p["att"], p["des_pos"], p["des_vel"], p["des_acc"], p["yaw"])
    assert _same(chk_thrust, thrust) and _same(chk_rates, rates), "stages_checker.run_position differs from the reference: that is the finding"
    assert _same(rates.astype(F).astype(D), rates) and _same(thrust.astype(F).astype(D), thrust)
    for k, v in p.items():
        fx["run_" + k] = v
    fx.update(run_thrust=thrust.astype(F), run_rates=rates.astype(F))
    fx["run_branch"] = np.packbits(np.stack([np.asarray(rinfo[k], bool) for k in RUN_BRANCHES]), axis=1)
    # the mission
    mcfg = mission_config()
    flown = fly_mission(pos, vel, att, sc.glibc_math)
    digests, m_thrust, m_rates = [], [], []
    for k, tick in enumerate(flown):
        assert (tick["stage_before"] == MISSION_STAGE_BEFORE[k]).all(), (k, tick["stage_before"][:4])
        digests.append(inputs_digest(tick["inputs"]))
        if MISSION_STAGE_BEFORE[k] in (sc.TAKEOFF, sc.FLIGHT, sc.LANDING):
            dp, dv, da, yaw = tick["inputs"]
            thrust, rates = probe_run(probe, mcfg, pos, vel, att, dp, dv, da, yaw)
            assert _same(tick["thrust"], thrust) and _same(tick["rates"], rates), "the mission's Run differs from the reference at tick %d" % k
            assert _same(rates.astype(F).astype(D), rates) and _same(thrust.astype(F).astype(D), thrust)
            if k in MISSION_RECORDED:
                m_thrust.append(thrust.astype(F))
                m_rates.append(rates.astype(F))
    assert (flown[-1]["fields"]["stage"] == sc.LANDING).all()
    fx.update(msn_dt_us=np.array(MISSION_DT_US, np.int32), msn_recorded=np.array(MISSION_RECORDED, np.int32), msn_digest=np.stack(digests),
              msn_thrust=np.stack(m_thrust), msn_rates=np.stack(m_rates))
    # the safety net
    s = make_safety_population()
    flags = probe_safety_net(probe, scfg, s["pos"], s["att"], s["since"], s["fresh"], s["set_unsafe"])
    for k, v in s.items():
        fx["net_" + k] = v.astype(F) if v.dtype == D else v
    fx["net_flags"] = flags
    # the pipe
    ops = make_pipe_script()
    fx.update(pipe_delay=np.float64(PIPE_DELAY), pipe_ops=ops, pipe_out=probe_pipe(probe, PIPE_DELAY, ops))
    fx.update(rec.arrays())
    check_coverage(fx)
    if verbose:
        for k, v in standin_counts(fx).items():
            print("numpy in place of libm, %s: %d of %d codes differ, largest distance %d" % ((k,) + v))
    return fx


RUN_BRANCHES = ("sat_norm", "z_floor", "thrust_floor", "yaw_nonzero", "cos_ge_1", "n_tiny", "cos_le_m1")


def branch_counts(fx, which):
    names = (fc.BRANCHES + ("theta_small",)) if which == "trk" else RUN_BRANCHES
    n = N_TRK if which == "trk" else N_RUN
    bits = np.unpackbits(fx[which + "_branch"], axis=1)[:, :n]
    return {k: int(bits[i].sum()) for i, k in enumerate(names)}


def check_coverage(fx):
    """every live branch behind the reference was reached by the recorded inputs, and the populations are the issue's"""
    trk = branch_counts(fx, "trk")
    assert all(v > 0 for v in trk.values()), trk
    run = branch_counts(fx, "run")
    assert all(run[k] > 0 for k in RUN_BRANCHES if sc.BRANCHES[k]) and run["cos_le_m1"] == 0, run
    tilt = tilt_degrees(fx["trk_att"].astype(D))
    assert (tilt[N_SPHERE:] < 2.0).all() and (tilt[:N_SPHERE] > 90).sum() > 30
    flags = fx["net_flags"]
    assert all(flags[:, k].any() and not flags[:, k].all() for k in range(5))
    out = fx["pipe_out"][fx["pipe_ops"]["op"] == GET]
    assert (out["found"] == 0).any() and set(out["id"][out["found"] == 1]) == {0, 1, 2, 3, 4} and (out["ballistic"] == 1).any()


def standin_counts(fx):
    """the CPU stand-in for the device: the checkers with numpy's functions against the reference's codes"""
    out = {}
    pos, vel, att = (fx[k].astype(D) for k in ("trk_pos", "trk_vel", "trk_att"))
    thrust, rates = fc.run_tracking(pos, vel, att, fx["trk_ref14"], fc.default_config(), fc.numpy_math)
    got, ref = sent_of(thrust, rates), sent_of(fx["trk_thrust"], fx["trk_rates"])
    out["RunTracking sphere"] = code_differences(got[:, :N_SPHERE], ref[:, :N_SPHERE])
    out["RunTracking near-level"] = code_differences(got[:, N_SPHERE:], ref[:, N_SPHERE:])
    p = {k: fx["run_" + k] for k in ("pos", "vel", "att", "des_pos", "des_vel", "des_acc", "yaw")}
    thrust, rates = sc.run_position(p["pos"], p["vel"], p["att"], p["des_pos"], p["des_vel"], p["des_acc"], p["yaw"], sc.default_config(), sc.numpy_math)
    out["Run sphere"] = code_differences(sent_of(thrust, rates), sent_of(fx["run_thrust"], fx["run_rates"]))
    flown = fly_mission(pos, vel, att, sc.numpy_math)
    sphere, level = [0, 0, 0], [0, 0, 0]
    for r, k in enumerate(fx["msn_recorded"]):
        got, ref = sent_of(flown[k]["thrust"], flown[k]["rates"]), sent_of(fx["msn_thrust"][r], fx["msn_rates"][r])
        for acc, cols in ((sphere, slice(0, N_SPHERE)), (level, slice(N_SPHERE, None))):
            d = code_differences(got[:, cols], ref[:, cols])
            acc[0], acc[1], acc[2] = acc[0] + d[0], acc[1] + d[1], max(acc[2], d[2])
    out["mission sphere"], out["mission near-level"] = tuple(sphere), tuple(level)
    return out


CAPPED = ("RunTracking sphere", "Run sphere", "mission sphere")


def within_cap(differing, of, largest):
    return largest <= 1 and differing <= 0.01 * of


def write_fixture(fx, path=FIXTURE):
    """an .npz whose bytes depend on its arrays alone (np.savez stamps the time of day into the archive)"""
    with zipfile.ZipFile(path, "w") as z:
        for name in sorted(fx):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(fx[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def load_fixture(path=FIXTURE):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":
    if not os.path.exists(PROBE):
        sys.exit("oracle/_ref/offboard_probe is not built (make -C oracle ref, where the reference sources are present)")
    if "--seeds" in sys.argv:
        for s in SEEDS_LOOKED_AT:
            counts = standin_counts(make_offboard_reference(seed=s))
            print("seed %d: %s  %r" % (s, "passes" if all(within_cap(*counts[k]) for k in CAPPED) else "misses the cap", counts))
        sys.exit(0)
    fixture = make_offboard_reference(verbose=True)
    write_fixture(fixture)
    size = os.path.getsize(FIXTURE)
    print("written", FIXTURE, size, "bytes")
    assert size <= SIZE_LIMIT, "larger than rigid_body_reference.npz"
