"""Writes tests/golden/gps_reference.npz: what the reference's own Offboard::GPSIMUStateEstimator -- GPSIMUStateEstimator.cpp
compiled where it lies into oracle/_ref/gps_probe, against the recording dense stand-in oracle/eigen_dense -- holds after every
call of two scripts, and the stand-in's tape of every call.  Numbers only.  tests/test_gps_reference.py holds the two
restatements (tests/gps_imu_reference.py, tests/gps_estimator_checker.py) to it without the probe; tests/test_gpu_gps_reference.py
holds the device to its free-running branches and masks.

    python tests/golden/make_gps_reference.py         (needs oracle/_ref/gps_probe: make -C oracle ref)

THE SCRIPTS (tests/gps_estimator_checker.py's events; inputs from synthetic_inputs, seeded)
  m   14 vehicles: make_phase_script (0 to 5 ordinary Predicts between alignment and first measurement, three periods), then
      make_script's special events -- a measurement before any Predict, a first Predict again, the tiny / inf / far payloads --,
      the skew payload (a finite covariance that is not symmetric, so that :256 acts) and two more periods, one accelerometer
      sample of vehicle 1 NaN; the last vehicle's position is NaN throughout
  p   36 vehicles: the "poison" payload (one NaN, +Inf or -Inf in a finite covariance: a diagonal and an off-diagonal place
      of each of the six blocks), Predict, measurement; the payload again, measurement at once; a period
TWO RECORDINGS of each: tf, teacher-forced (the definition's state loaded in front of every call, so that differences of
evaluation order cannot pile up), and fr, free-running (nothing loaded behind the constructor but the script's own set_state).

WHAT IS KEPT
  {s}_{tf,fr}_branch [E, n] uint8   index into gps_estimator_checker.CALL_BRANCHES, NO_CALL where the event calls nothing
  {s}_{tf,fr}_int    [E, 4, n]      _initialized, _numResets, both timers' reset stamps, after the call
  {s}_{tf,fr}_mask   [E, 97, n]     finite? of pos, vel, att, angVel (13), _lastMeasUpdateAttCorrection (3), _cov (81)
  {s}_fr_singular    [measures]     vehicles in the singular branch
  {s}_tf_est, _corr, _diag          the mean, the correction and the covariance's diagonal after the call; _offzero: every
                                    off-diagonal entry is +0 or -0
  {s}_tf_f [imu events, 81, n]      f of :126-191, the first product's first operand
  {s}_tf_S, _d                      innovationCov (determinant()'s operand) and deltaPos
  {s}_tf_{T,C,det,inv,L,dx,M}_off / _cls
      the stand-in's results -- f * _cov, (f * _cov) * f', determinant(), inverse(), _cov * H' * Sinv, L * deltaPos,
      (I - L H) * _cov -- as ORDINAL OFFSETS from the correctly rounded exact value of the operation on its recorded
      operands (an integer: how many doubles up or down; the reference's bits are that many steps from a value the test
      computes from the operands in integer arithmetic), and a class where the exact value does not exist: 1 NaN, 2 +Inf,
      3 -Inf.  Lossless; 81 small integers where 81 doubles would not fit a fixture.
  tab_*   sin, cos and acosf as this machine's libm gave them for every argument the definition asked for
  digest  of the scripts and inputs

The generator asserts what keeps a bound from hiding a branch flip: every |det| further from 1e-10 and every rotation
vector's norm further from MIN_ANGLE than its bound, and every branch reachable behind Reset() taken."""
import hashlib
import io
import math
import os
import sys
import zipfile
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import gps_estimator_checker as gc            # noqa: E402
from tests import gps_imu_reference as ref               # noqa: E402
from tests import gps_probe as gp                        # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "gps_reference.npz")
D = np.float64
SEED = 11
N_MAIN = gc.SCRIPT_MIN_N
NAN_ACC_VEHICLE = 1
U = Fraction(1, 2 ** 53)


def gamma(n):
    return n * U / (1 - n * U)


# ---- the scripts ----------------------------------------------------------------------------------------------------------------
def scripts():
    """-> {name: (n, script, inputs)}"""
    n = N_MAIN
    period = [("imu",)] * 5 + [("measure",)]
    special = gc.make_script(n)[18:28]
    assert special[0][0] == "reset" and special[-1] == ("measure",) and [e[1] for e in special if e[0] == "set_state"] == ["tiny", "inf", "far"]
    main = gc.make_phase_script(n) + special + [("set_state", "skew", 3, 2), ("measure",)] + period * 2
    inputs = gc.synthetic_inputs(main, n, SEED)
    k_nan = len(main) - 3                                  # an ordinary Predict of the last period
    assert main[k_nan] == ("imu",)
    now, a, w = inputs[k_nan]
    a = a.copy()
    a[:, NAN_ACC_VEHICLE] = np.nan
    inputs[k_nan] = (now, a, w)
    p = gc.N_POISON
    poison = [("set_state", "poison", 0, p), ("imu",), ("measure",), ("set_state", "poison", 0, p), ("measure",)] + period
    return {"m": (n, main, inputs), "p": (p, poison, gc.synthetic_inputs(poison, p, SEED + 1))}


def digest(all_scripts):
    h = hashlib.sha256()
    for name in sorted(all_scripts):
        n, script, inputs = all_scripts[name]
        h.update(repr((name, n, script)).encode())
        for x in inputs:
            for a in (x if isinstance(x, tuple) else (x,)):
                h.update(np.ascontiguousarray(np.asarray(a, D)).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


# ---- the function table ---------------------------------------------------------------------------------------------------------
TABLE_OPS = ("sin", "cos", "acosf")


class Recorder:
    """glibc_math that remembers every (function, argument bits) -> result bits it was asked for (acosf: of the narrowed
    argument)"""

    def __init__(self):
        self.seen = [{}, {}, {}]

    def __call__(self, op, x):
        x = np.asarray(x, D)
        y = ref.glibc_math(op, x)
        with np.errstate(all="ignore"):
            key = x.astype(np.float32).astype(D) if op == 2 else x
        for a, r in zip(np.ascontiguousarray(key).reshape(-1).view(np.uint64), np.ascontiguousarray(y).reshape(-1).view(np.uint64)):
            self.seen[op][int(a)] = int(r)
        return y

    def arrays(self):
        out = {}
        for op, name in enumerate(TABLE_OPS):
            keys = sorted(self.seen[op])
            out["tab_%s_arg" % name] = np.array(keys, np.uint64)
            out["tab_%s_res" % name] = np.array([self.seen[op][k] for k in keys], np.uint64)
        return out


class Table:
    """the recorded functions.  An argument the table lacks is answered by this machine's libm and written into `misses`
    (tests/test_gps_reference.py asserts there are none, behind the tests that say WHICH number of a restatement moved)"""

    def __init__(self, fx):
        self.arg = [fx["tab_%s_arg" % k] for k in TABLE_OPS]
        self.res = [fx["tab_%s_res" % k] for k in TABLE_OPS]
        self.misses = []

    def __call__(self, op, x):
        x = np.asarray(x, D)
        with np.errstate(all="ignore"):
            key = np.ascontiguousarray(x.astype(np.float32).astype(D) if op == 2 else x)
        bits = key.reshape(-1).view(np.uint64)
        arg, res = self.arg[op], self.res[op]
        at = np.minimum(np.searchsorted(arg, bits), arg.size - 1)
        found = arg[at] == bits
        nan = np.isnan(key.reshape(-1))                    # (which NaN an operation hands on is the machine's business)
        out = np.where(nan, np.nan, res[at].view(D))
        if not (found | nan).all():
            self.misses.append("%s(%r)" % (TABLE_OPS[op], float(key.reshape(-1)[~(found | nan)][0])))
            out = np.where(found | nan, out, ref.glibc_math(op, key.reshape(-1)))
        return out.reshape(x.shape)

    def first_entry_libm_misses(self):
        for op, name in enumerate(TABLE_OPS):
            got = np.ascontiguousarray(ref.glibc_math(op, self.arg[op].view(D))).view(np.uint64)
            bad = np.flatnonzero(got != self.res[op])
            if bad.size:
                return "%s(%r): recorded 0x%x, this libm 0x%x" % (name, float(self.arg[op].view(D)[bad[0]]), int(self.res[op][bad[0]]), int(got[bad[0]]))
        return None


# ---- the definition's run ----------------------------------------------------------------------------------------------------------
def run_definition(n, script, inputs, math):
    """the numpy checker over the script -> (state BEFORE every event with `corr`, state after every event with `corr` and
    `branch`, singular per measure, counts)"""
    chk = gc.Estimator(n, math=math)

    def snap():
        return dict(chk.state(), corr=chk.corr.copy())

    before, after, singular = [], [], {}
    for k, ev in enumerate(script):
        before.append(snap())
        chk.last_branch = np.full(n, gc.NO_CALL, np.uint8)
        one, sing = gc.run_script([ev], chk, [inputs[k]])
        if ev[0] == "reset_ranges":                        # (several reset calls: the union)
            who = np.zeros(n, bool)
            for first, count in ev[1]:
                who[first:first + count] = True
            chk.last_branch = np.where(who, 6, gc.NO_CALL).astype(np.uint8)
        if ev[0] == "measure":
            singular[k] = sing[0]
        if ev[0] == "set_state":
            chk.last_branch = np.full(n, gc.NO_CALL, np.uint8)
        after.append(dict(snap(), branch=chk.last_branch.copy()))
    return before, after, singular, chk.count


# ---- exact arithmetic on doubles: a double is m * 2^e, sums of products are integers over a common power of two ---------------------
def _sc(x):
    m, e = math.frexp(x)
    return int(m * 9007199254740992.0), e - 53


def exact_dot(a, b):
    """sum a[k] b[k] and sum |a[k] b[k]| exactly -> (S, A, e): the values are S * 2^e and A * 2^e; None if a term is not finite"""
    terms = []
    for x, y in zip(a, b):
        if not (math.isfinite(x) and math.isfinite(y)):
            return None
        (m1, e1), (m2, e2) = _sc(x), _sc(y)
        terms.append((m1 * m2, e1 + e2))
    e = min(t[1] for t in terms)
    S = sum(m << (ee - e) for m, ee in terms)
    A = sum(abs(m) << (ee - e) for m, ee in terms)
    return S, A, e


def frac(S, e):
    return Fraction(S) * (Fraction(2) ** e)


def round_to_double(fr):
    """the double nearest a Fraction (CPython's integer true division is correctly rounded)"""
    return fr.numerator / fr.denominator


def ordinal(x):
    """doubles in their order as integers: +0 is 0, -0 is -1"""
    b = int(np.array(x, D).view(np.int64))
    return b if b >= 0 else -(b & 0x7fffffffffffffff) - 1


def from_ordinal(o):
    b = o if o >= 0 else (-o - 1) | (1 << 63)
    return float(np.array(b, np.uint64).view(D))


def classify(x):
    return 0 if math.isfinite(x) else 1 if x != x else 2 if x > 0 else 3


CLASS_VALUE = (None, float("nan"), float("inf"), float("-inf"))


def encode(value, exact):
    """(offset, class) of a recorded result against the exact value of its operands (a Fraction, or None)"""
    if exact is None:
        assert not math.isfinite(value), "the stand-in gave a finite result where a term is not finite"
        return 0, classify(value)
    assert math.isfinite(value), "the stand-in gave a result that is not finite from finite terms"
    off = ordinal(value) - ordinal(round_to_double(exact))
    assert abs(off) < 2 ** 62, off
    return off, 0


def decode(off, cls, exact):
    if cls:
        return CLASS_VALUE[int(cls)]
    return from_ordinal(ordinal(round_to_double(exact)) + int(off))


def product_exact(A, B, r, k, c):
    """entry by entry: (exact value or None, |A||B| exactly or None); A, B flat row major"""
    out = []
    for i in range(r):
        for j in range(c):
            d = exact_dot([A[i * k + t] for t in range(k)], [B[t * c + j] for t in range(k)])
            out.append((None, None) if d is None else (frac(d[0], d[2]), frac(d[1], d[2])))
    return out


# ---- the derived bounds (tests/test_gps_reference.py's docstring carries the derivation) ------------------------------------------
def det_exact_and_bound(S):
    """S [3][3] of Fractions -> (det, bound): any evaluation by products of three entries and sums rounds each of the six
    triple products at most 7 times (cofactors along a row: 2 products, a difference, a product, two sums = 5; six triple
    products summed: 2 + 5): gamma_7 times the permanent of |S|"""
    det = (S[0][0] * (S[1][1] * S[2][2] - S[1][2] * S[2][1]) - S[0][1] * (S[1][0] * S[2][2] - S[1][2] * S[2][0])) + \
        S[0][2] * (S[1][0] * S[2][1] - S[1][1] * S[2][0])
    a = [[abs(x) for x in row] for row in S]
    perm = a[0][0] * (a[1][1] * a[2][2] + a[1][2] * a[2][1]) + a[0][1] * (a[1][0] * a[2][2] + a[1][2] * a[2][0]) + \
        a[0][2] * (a[1][0] * a[2][1] + a[1][1] * a[2][0])
    return det, gamma(7) * perm


def inverse_exact_and_bound(S):
    """-> (Sinv [3][3], bound [3][3]) for cofactor / determinant, the quotient by one division or by a reciprocal and a
    product (two roundings): with c the exact cofactor, Ec = gamma_2 (|ab| + |cd|) its bound, d the determinant and Ed its
    bound, |c^/d^ - c/d| <= (Ec + |c| Ed / |d|) / (|d| - Ed), and the two roundings add gamma_2 (|c| + Ec) / (|d| - Ed)"""
    det, Ed = det_exact_and_bound(S)
    assert abs(det) > Ed
    inv = [[None] * 3 for _ in range(3)]
    bound = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            a, b, c, e = (j + 1) % 3, (j + 2) % 3, (i + 1) % 3, (i + 2) % 3
            cof = S[a][c] * S[b][e] - S[a][e] * S[b][c]
            Ec = gamma(2) * (abs(S[a][c] * S[b][e]) + abs(S[a][e] * S[b][c]))
            inv[i][j] = cof / det
            bound[i][j] = (Ec + abs(cof) * Ed / abs(det)) / (abs(det) - Ed) + gamma(2) * (abs(cof) + Ec) / (abs(det) - Ed)
    return inv, bound


def update_chain(P, S, d):
    """The exact update of :239-256 from its primary operands, and for every computed quantity a bound that holds for ANY
    evaluation order of the products, determinant() and inverse() -- the stand-in's and the definition's alike.
    P [9][9], S [3][3], d [3] as doubles -> dict of (exact, bound) lists of Fractions: inv [3][3], L [9][3], dx [9],
    M [9][9] (= (I - L H) P), cov [9][9] (= 0.5 (M + M'))"""
    Pf = [[Fraction(x) for x in row] for row in P]
    Sf = [[Fraction(x) for x in row] for row in S]
    df = [Fraction(x) for x in d]
    inv, Einv = inverse_exact_and_bound(Sf)
    g3, g9 = gamma(3), gamma(9)
    L = [[sum(Pf[i][k] * inv[k][j] for k in range(3)) for j in range(3)] for i in range(9)]
    EL = [[sum(abs(Pf[i][k]) * Einv[k][j] for k in range(3)) + g3 * sum(abs(Pf[i][k]) * (abs(inv[k][j]) + Einv[k][j]) for k in range(3))
           for j in range(3)] for i in range(9)]
    dx = [sum(L[i][k] * df[k] for k in range(3)) for i in range(9)]
    Edx = [sum(abs(df[k]) * EL[i][k] for k in range(3)) + g3 * sum((abs(L[i][k]) + EL[i][k]) * abs(df[k]) for k in range(3)) for i in range(9)]
    # I - L H: one rounding where H has its ones; the definition forms P - L P[0:3] without it, and is covered
    EN = [[EL[i][k] + U * (1 + abs(L[i][k]) + EL[i][k]) for k in range(3)] for i in range(9)]
    M = [[Pf[i][j] - sum(L[i][k] * Pf[k][j] for k in range(3)) for j in range(9)] for i in range(9)]
    EM = [[sum(EN[i][k] * abs(Pf[k][j]) for k in range(3)) +
           g9 * (abs(Pf[i][j]) + sum((abs(L[i][k]) + EN[i][k]) * abs(Pf[k][j]) for k in range(3))) for j in range(9)] for i in range(9)]
    cov = [[(M[i][j] + M[j][i]) / 2 for j in range(9)] for i in range(9)]
    Ecov = [[(EM[i][j] + EM[j][i]) / 2 + U * (abs(M[i][j]) + abs(M[j][i]) + EM[i][j] + EM[j][i]) / 2 for j in range(9)] for i in range(9)]
    return dict(inv=(inv, Einv), L=(L, EL), dx=(dx, Edx), M=(M, EM), cov=(cov, Ecov))


def predict_bound(f, P):
    """exact f P f' and the bound of a product of a product, inner dimensions 9 and 9, in any order:
    (2 gamma_9 + gamma_9^2) |f| |P| |f'| -> (C [81], bound [81]) of Fractions, or (None, None) per entry where a term is
    not finite"""
    g = 2 * gamma(9) + gamma(9) ** 2
    fF = [[Fraction(x) for x in f[9 * i:9 * i + 9]] for i in range(9)]
    PF = [[Fraction(x) for x in P[9 * i:9 * i + 9]] for i in range(9)]
    nz = [[k for k in range(9) if fF[i][k] != 0] for i in range(9)]
    T = [[sum(fF[i][k] * PF[k][j] for k in nz[i]) for j in range(9)] for i in range(9)]
    Ta = [[sum(abs(fF[i][k] * PF[k][j]) for k in nz[i]) for j in range(9)] for i in range(9)]
    C = [sum(T[i][k] * fF[j][k] for k in nz[j]) for i in range(9) for j in range(9)]
    B = [g * sum(Ta[i][k] * abs(fF[j][k]) for k in nz[j]) for i in range(9) for j in range(9)]
    return C, B


# ---- reading a block's tape ----------------------------------------------------------------------------------------------------------
def split_tape(block):
    """the entries of one call by what they are"""
    t = block["tape"]
    shapes = [(e["kind"], e["r"], e["k"], e["c"]) for e in t]
    if block["branch"] == "predict":
        assert shapes == [(0, 9, 9, 9)] * 2, shapes
        return dict(FP=t[0], FPF=t[1])
    head = [(0, 9, 9, 3), (0, 3, 9, 3), (1, 3, 3, 1)]
    if block["branch"] == "singular":
        assert shapes == head, shapes
        return dict(PH=t[0], HPH=t[1], det=t[2])
    if block["branch"] == "update":
        assert shapes == head + [(2, 3, 3, 3), (0, 9, 9, 3), (0, 9, 3, 3), (0, 9, 3, 1), (0, 9, 3, 9), (0, 9, 9, 9)], shapes
        return dict(PH=t[0], HPH=t[1], det=t[2], inv=t[3], PH2=t[4], L=t[5], dx=t[6], LH=t[7], M=t[8])
    assert shapes == [], (block["branch"], shapes)
    return {}


def unified_branch(block):
    b = block["branch"]
    if b == "singular":
        S = split_tape(block)["det"]["a"]
        b = "singular_tiny" if np.isfinite(S).all() else "singular_nonfinite"
    return gc.CALL_BRANCHES.index(b)


def same(a, b):
    return gc.same_bits(np.asarray(a, D), np.asarray(b, D))


# ---- the recordings ---------------------------------------------------------------------------------------------------------------
def _common(events, n, script):
    E = len(script)
    branch = np.full((E, n), gc.NO_CALL, np.uint8)
    ints = np.zeros((E, 4, n), np.int64)
    mask = np.zeros((E, 97, n), bool)
    singular = []
    for k, calls in enumerate(events):
        for v, b in calls.items():
            branch[k, v] = unified_branch(b)
            ints[k, :, v] = (b["initialized"], b["num_resets"], b["last_predict_us"], b["last_update_us"])
            mask[k, :, v] = np.isfinite(np.concatenate([b["est"], b["corr"], b["cov"]]))
        if script[k][0] == "measure":
            singular.append(sum(b["branch"] == "singular" for b in calls.values()))
    return branch, ints, mask, np.array(singular, np.int32)


def record(name, n, script, inputs, before, rec, verbose=False):
    fx, ratios = {}, {}
    free, _ = gp.fly(script, inputs, n)
    forced, constructed = gp.fly(script, inputs, n, teacher=before)
    for b in constructed:                                  # the constructor: Reset() once, the correction NaN
        assert b["num_resets"] == 1 and b["initialized"] == 0 and np.isnan(b["corr"]).all() and same(b["last_meas_att"], [1, 0, 0, 0])
    fx["fr_branch"], fx["fr_int"], fx["fr_mask"], fx["fr_singular"] = _common(free, n, script)
    fx["tf_branch"], fx["tf_int"], fx["tf_mask"], _ = _common(forced, n, script)
    E = len(script)
    imu = [k for k, ev in enumerate(script) if ev[0] == "imu"]
    mea = [k for k, ev in enumerate(script) if ev[0] == "measure"]
    est, corr, diag = np.full((E, 13, n), np.nan), np.full((E, 3, n), np.nan), np.full((E, 9, n), np.nan)
    offzero = np.zeros((E, n), bool)
    f = np.full((len(imu), 81, n), np.nan)
    S, d = np.full((len(mea), 9, n), np.nan), np.full((len(mea), 3, n), np.nan)
    sizes = dict(T=(len(imu), 81), C=(len(imu), 81), det=(len(mea), 1), inv=(len(mea), 9), L=(len(mea), 27), dx=(len(mea), 9), M=(len(mea), 81))
    off = {q: np.zeros(s + (n,), np.int64) for q, s in sizes.items()}
    cls = {q: np.zeros(s + (n,), np.uint8) for q, s in sizes.items()}

    def note(what, err, bound):
        if bound > 0:
            ratios[what] = max(ratios.get(what, 0.0), float(err / bound))
        else:
            assert err == 0, (what, err)

    def keep(q, row, v, values, exact):
        for t, (x, ex) in enumerate(zip(values, exact)):
            off[q][row, t, v], cls[q][row, t, v] = encode(float(x), ex)

    def judge_product(what, e):
        """a product on the tape against the exact value of its recorded operands: gamma_k |A| |B|"""
        ex = product_exact(e["a"], e["b"], e["r"], e["k"], e["c"])
        g = gamma(e["k"])
        for x, (val, ab) in zip(e["out"], ex):
            if val is None:
                assert not math.isfinite(x), what
            else:
                assert math.isfinite(x), what
                err = abs(Fraction(float(x)) - val)
                assert err <= g * ab, (what, float(err), float(g * ab))
                note(what, err, g * ab)
        return [val for val, _ in ex]

    for k, calls in enumerate(forced):
        for v, b in calls.items():
            est[k, :, v], corr[k, :, v] = b["est"], b["corr"]
            C = b["cov"].reshape(9, 9)
            diag[k, :, v] = np.diag(C)
            offzero[k, v] = bool((C[~np.eye(9, dtype=bool)] == 0).all())
            t = split_tape(b)
            P = before[k]["cov"][:, v]
            if b["branch"] == "predict":
                r = imu.index(k)
                assert same(t["FP"]["b"], P) and same(t["FPF"]["a"], t["FP"]["out"]), "the tape's operands are not the loaded state"
                f[r, :, v] = t["FP"]["a"]
                assert same(t["FPF"]["b"], t["FP"]["a"].reshape(9, 9).T.reshape(81))
                keep("T", r, v, t["FP"]["out"], judge_product("f * _cov", t["FP"]))
                keep("C", r, v, t["FPF"]["out"], judge_product("(f * _cov) * f'", t["FPF"]))
                both = np.isfinite(t["FPF"]["out"]) == np.isfinite(b["cov"])      # the noise of :197-202 flips no mask
                assert both.all()
            elif b["branch"] in ("singular", "update"):
                r = mea.index(k)
                assert same(t["PH"]["a"], P), "the tape's operand is not the loaded state"
                judge_product("_cov * H'", t["PH"])
                judge_product("H * (_cov * H')", t["HPH"])
                S[r, :, v] = t["det"]["a"]
                fin = np.isfinite(t["det"]["a"]).all()
                if fin:
                    Sf = [[Fraction(float(x)) for x in t["det"]["a"][3 * i:3 * i + 3]] for i in range(3)]
                    det, Ed = det_exact_and_bound(Sf)
                    err = abs(Fraction(float(t["det"]["out"][0])) - det)
                    assert err <= Ed
                    note("determinant()", err, Ed)
                    # the condition that keeps the bound from hiding a branch flip
                    assert abs(abs(det) - Fraction(1e-10)) > Ed, "a recorded |det| is nearer 1e-10 than its bound"
                    keep("det", r, v, t["det"]["out"], [det])
                else:
                    keep("det", r, v, t["det"]["out"], [None])
                assert (b["branch"] == "singular") == (not fin or abs(float(t["det"]["out"][0])) < 1e-10)
            if b["branch"] == "update":
                P9 = [[float(x) for x in P[9 * i:9 * i + 9]] for i in range(9)]
                S3 = [[float(x) for x in t["det"]["a"][3 * i:3 * i + 3]] for i in range(3)]
                d[r, :, v] = t["dx"]["b"]
                finite_in = np.isfinite(t["dx"]["b"]).all()
                assert same(t["inv"]["a"], t["det"]["a"]) and same(t["PH2"]["out"], t["PH"]["out"]) and same(t["L"]["a"], t["PH2"]["out"])
                assert same(t["L"]["b"], t["inv"]["out"]) and same(t["dx"]["a"], t["L"]["out"]) and same(t["LH"]["a"], t["L"]["out"])
                assert same(t["M"]["b"], P)
                chain = update_chain(P9, S3, [float(x) if math.isfinite(x) else 0.0 for x in t["dx"]["b"]])
                inv_x = [x for row in chain["inv"][0] for x in row]
                keep("inv", r, v, t["inv"]["out"], inv_x)
                for x, ex, bd in zip(t["inv"]["out"], inv_x, [x for row in chain["inv"][1] for x in row]):
                    err = abs(Fraction(float(x)) - ex)
                    assert err <= bd
                    note("inverse()", err, bd)
                keep("L", r, v, t["L"]["out"], judge_product("_cov * H' * Sinv", t["L"]))
                keep("dx", r, v, t["dx"]["out"], judge_product("L * deltaPos", t["dx"]))
                judge_product("L * H", t["LH"])
                # I - L H: one IEEE subtraction per entry, whatever the order
                LH = t["LH"]["out"].reshape(9, 9)
                assert same(t["M"]["a"], (np.eye(9) - LH).reshape(81))
                keep("M", r, v, t["M"]["out"], judge_product("(I - L H) * _cov", t["M"]))
                Mo = t["M"]["out"].reshape(9, 9)
                assert same(b["cov"], (0.5 * (Mo + Mo.T)).reshape(81))          # :256, one rounding and an exact halving
                assert same(b["corr"], t["dx"]["out"][6:9])
                if finite_in:                               # the table learns the arguments of :252 on the reference's correction
                    ref.from_rotvec(tuple(float(x) for x in b["corr"]), rec)
                # the stand-in against the chain's bounds (the definition is held to the same in the test)
                for q, got in (("L", t["L"]["out"]), ("dx", t["dx"]["out"]), ("M", t["M"]["out"]), ("cov", b["cov"])):
                    if q == "dx" and not finite_in:
                        continue
                    ex, bd = chain[q]
                    ex = [x for row in ex for x in row] if q != "dx" else ex
                    bd = [x for row in bd for x in row] if q != "dx" else bd
                    for x, e1, b1 in zip(got, ex, bd):
                        err = abs(Fraction(float(x)) - e1)
                        assert err <= b1, (q, float(err), float(b1))
                        note("chain " + q, err, b1)
                if finite_in:                               # the rotation vector's norm against MIN_ANGLE
                    ex, bd = chain["dx"]
                    norm = math.sqrt(float(sum(x * x for x in ex[6:9])))
                    slack = math.sqrt(float(sum(x * x for x in bd[6:9]))) + 4 * 2.0 ** -53 * norm
                    assert abs(norm - ref.MIN_ANGLE) > slack, "a rotation vector's norm is nearer MIN_ANGLE than its bound"
    for key, arr in (("tf_est", est), ("tf_corr", corr), ("tf_diag", diag), ("tf_offzero", offzero), ("tf_f", f), ("tf_S", S), ("tf_d", d)):
        fx[key] = arr
    for q in off:
        fx["tf_%s_off" % q], fx["tf_%s_cls" % q] = off[q], cls[q]
    for key in list(fx):                                    # one NaN, so that the bytes do not depend on which NaN a machine hands on
        if fx[key].dtype == D:
            fx[key] = np.where(np.isnan(fx[key]), np.nan, fx[key])
    if verbose:
        print(name, "worst ratio to the bound:", {k: "%.3g" % r for k, r in sorted(ratios.items())})
    return {"%s_%s" % (name, k): a for k, a in fx.items()}, ratios


def check_branches(counts_by_script, fixture):
    total = {b: sum(c[b] for c in counts_by_script.values()) for b in ref.BRANCHES}
    for b in gc.SCRIPT_BRANCHES:
        assert total[b] > 0, "no vehicle takes the branch %r" % b
    for s in counts_by_script:
        for kind in ("tf", "fr"):
            seen = set(np.unique(fixture["%s_%s_branch" % (s, kind)]))
            assert seen - {gc.NO_CALL}, s
    seen = set(np.unique(np.concatenate([fixture["%s_fr_branch" % s].reshape(-1) for s in counts_by_script]))) - {gc.NO_CALL}
    assert seen == set(range(len(gc.CALL_BRANCHES))), "the reference does not reach every branch: %r" % seen


def make_gps_reference(verbose=False):
    all_scripts = scripts()
    rec = Recorder()
    fx, ratios, counts = {"digest": digest(all_scripts)}, {}, {}
    for name in sorted(all_scripts):
        n, script, inputs = all_scripts[name]
        before, after, singular, counts[name] = run_definition(n, script, inputs, rec)
        part, r = record(name, n, script, inputs, before, rec, verbose)
        fx.update(part)
        for k, x in r.items():
            ratios[k] = max(ratios.get(k, 0.0), x)
    fx.update(rec.arrays())
    check_branches(counts, fx)
    for k in list(fx):
        if fx[k].dtype == bool:
            fx[k] = np.packbits(fx[k].reshape(-1))
    return fx, ratios


def unpack(fx, key, shape):
    return np.unpackbits(fx[key])[:int(np.prod(shape))].reshape(shape).astype(bool)


def write_fixture(fx, path=FIXTURE):
    """an .npz whose bytes depend on its arrays alone (np.savez_compressed stamps the time of day into the archive)"""
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
    if not os.path.exists(gp.PROBE):
        sys.exit("oracle/_ref/gps_probe is not built (make -C oracle ref, where the reference sources are present)")
    fixture, worst = make_gps_reference(verbose=True)
    write_fixture(fixture)
    size = os.path.getsize(FIXTURE)
    print("written", FIXTURE, size, "bytes")
    print("worst ratios:", {k: "%.4g" % v for k, v in sorted(worst.items())})
    assert size <= 1 << 20
