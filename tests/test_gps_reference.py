"""The GPS + IMU estimator's two restatements (tests/gps_imu_reference.py, tests/gps_estimator_checker.py) against the
REFERENCE's own Offboard::GPSIMUStateEstimator, as tests/golden/gps_reference.npz recorded it from oracle/_ref/gps_probe
(GPSIMUStateEstimator.cpp compiled where it lies against the recording dense stand-in oracle/eigen_dense; the generator,
tests/golden/make_gps_reference.py, says what the fixture holds).  CPU, no GPU, and no probe at test time: sin, cos and
acosf come from the table recorded with the fixture.

WHAT IS CONCLUDED, and no more (oracle/eigen_dense/Eigen/Dense):
  bit for bit   what the reference computes outside Eigen
  exactly       the branch of every call, the finite / non-finite mask of every member, the number of singular restarts --
                teacher-forced AND free-running
  within a derived bound, never a measured one: what Eigen's products, determinant() and inverse() give for finite numbers

THE BOUNDS.  u = 2^-53, gamma_n = n u / (1 - n u).  Every bound is computed in rational arithmetic from RECORDED OPERANDS.
  * A product with inner dimension n, summed in any order: |fl(A B) - A B| <= gamma_n (|A| |B|) (Higham, Accuracy and
    Stability, 3.5).  f P f' as a product of a product: gamma_9 |f| |P| |f'| from the inner one carried through |f'|, plus
    gamma_9 |T^| |f'| with |T^| <= (1 + gamma_9) |f| |P|: (2 gamma_9 + gamma_9^2) |f| |P| |f'|.  The definition's sparse
    order rounds each term fewer times and is covered.  The noise of :197-202 is one more rounding: u (|C| + bound + |q|).
  * determinant() of S: the determinant is the sum of six signed triple products.  Cofactors along a row or column round
    each triple product 5 times (inner product, difference, outer product, two sums), six triple products summed 7 times
    (two products, five sums): |det^ - det| <= gamma_7 perm(|S|) =: Ed.
  * inverse(): entry = cofactor c over det, c^ with Ec = gamma_2 (|ab| + |cd|), the quotient by a division or by a
    reciprocal and a product (two roundings): |c^/d^ - c/d| <= (Ec + |c| Ed / |d|) / (|d| - Ed), plus
    gamma_2 (|c| + Ec) / (|d| - Ed) =: Einv.  (|d| > Ed is asserted.)
  * L = P[:, 0:3] Sinv, three terms: EL = |P| Einv + gamma_3 |P| (|Sinv| + Einv).  (_cov * H' copies: its sums add zeros.)
  * dx = L dpos, three terms, dpos bit for bit: Edx = EL |dpos| + gamma_3 (|L| + EL) |dpos|.
  * (I - L H) * _cov: I - L H is one rounding where H has its ones, EN = EL + u (1 + |L| + EL); nine terms:
    EM = EN |P[0:3]| + gamma_9 (|P[i][j]| + (|L| + EN) |P[0:3]|).  The definition forms P - L P[0:3] in four roundings a
    term and is covered (its |P[i][j]| + |L[i][i]| |P[i][j]| is what the second part carries).
  * 0.5 (C + C'): one rounding, an exact halving: Ecov = (EM + EM') / 2 + u (|M| + |M'| + EM + EM') / 2.
  * The updated mean: pos + dx[0:3] and vel + dx[3:6] are one rounding more, Edx + u (|x| + |dx| + Edx);
    _lastMeasUpdateAttCorrection is dx[6:9], Edx.  The attitude of :252 is NOT bounded: the line is held bit for bit on
    the reference's own recorded correction, and its only order-dependent input is that correction.
The stand-in's results are held to the same bounds by the generator, and here again from the fixture.  Worst ratios to
each bound, stand-in and definition (figures, not thresholds), are in profiles/gps_reference.json; the largest is 0.92."""
import importlib.util
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import gps_estimator_checker as gc
from tests import gps_imu_reference as ref
from tests import gps_probe as gp

D = np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
R_POS = ref.default_config()["sigma_pos"] ** 2


def _generator():
    spec = importlib.util.spec_from_file_location("make_gps_reference", os.path.join(HERE, "golden", "make_gps_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _scalar_run(n, script, inputs, math):
    """the scalar restatement, one object per vehicle -> the state after every event, with corr and the branch of the call"""
    clock = ref.Clock()
    ests = [ref.GPSIMUStateEstimator(clock, math=math) for _ in range(n)]
    after = []

    def branch_of(e, call):
        before = dict(e.count)
        call()
        took = {k for k in e.count if e.count[k] != before[k]}
        for name in ("predict", "measure_before_predict", "singular_nonfinite", "singular_tiny", "update"):
            if name in took:
                return gc.CALL_BRANCHES.index(name)
        assert took & {"first_predict_level", "first_predict_tilted"}, took
        return 0

    for k, ev in enumerate(script):
        branch = np.full(n, gc.NO_CALL, np.uint8)
        if ev[0] == "imu":
            now, a, w = inputs[k]
            clock.us = now
            for v, e in enumerate(ests):
                branch[v] = branch_of(e, lambda: e.Predict(tuple(float(x) for x in a[:, v]), tuple(float(x) for x in w[:, v])))
        elif ev[0] == "measure":
            now, z = inputs[k]
            clock.us = now
            for v, e in enumerate(ests):
                branch[v] = branch_of(e, lambda: e.UpdateWithMeasurement(tuple(float(x) for x in z[:, v])))
        elif ev[0] in ("reset", "reset_ranges"):
            clock.us = inputs[k]
            for first, count in ([(ev[1], ev[2])] if ev[0] == "reset" else ev[1]):
                for v in range(first, first + count):
                    ests[v].Reset()
                    branch[v] = 6
        else:
            e13, c81, k3 = gc.payload(ev[1], ev[3], inputs[k])
            for i, e in enumerate(ests[ev[2]:ev[2] + ev[3]]):
                e.pos, e.vel = tuple(map(float, e13[0:3, i])), tuple(map(float, e13[3:6, i]))
                e.att, e.ang_vel = tuple(map(float, e13[6:10, i])), tuple(map(float, e13[10:13, i]))
                e.cov = [[float(c81[9 * a + b, i]) for b in range(9)] for a in range(9)]
                e.corr = tuple(map(float, k3[:, i]))
                e.initialized = True
        after.append({"est": np.array([e.GetCurrentEstimate() for e in ests]).T, "cov": np.array([np.array(e.cov).reshape(81) for e in ests]).T,
                      "corr": np.array([e.corr for e in ests]).T,
                      "last_predict_us": np.array([e.estimate_timer.reset_us for e in ests], np.uint64),
                      "last_update_us": np.array([e.last_good.reset_us for e in ests], np.uint64),
                      "initialized": np.array([e.initialized for e in ests], np.uint8),
                      "num_resets": np.array([e.num_resets for e in ests], np.uint32), "branch": branch})
    return after


@pytest.fixture(scope="module")
def world():
    """the fixture, the generator's module, and both restatements run over both scripts with the recorded function table"""
    mod = _generator()
    fx = mod.load_fixture()
    table = mod.Table(fx)
    runs = {}
    for name, (n, script, inputs) in mod.scripts().items():
        before, after, singular, count = mod.run_definition(n, script, inputs, table)
        runs[name] = dict(n=n, script=script, inputs=inputs, before=before, after=after, singular=singular, count=count,
                          scalar=_scalar_run(n, script, inputs, table))
    return mod, fx, table, runs


def _shape(run, width):
    return (len(run["script"]), width, run["n"])


def _restatements(run):
    return (("checker", run["after"]), ("scalar", run["scalar"]))


def test_recipe_and_fixture_agree(world):
    """the scripts and inputs are the recorded ones; where the probe is built (the reference is present) the generator gives
    the committed fixture again, array for array"""
    mod, fx, table, runs = world
    assert np.array_equal(fx["digest"], mod.digest(mod.scripts())), "tests/golden/gps_reference.npz was recorded from other scripts or inputs"
    if os.path.exists(gp.PROBE):
        again, _ = mod.make_gps_reference()
        assert sorted(again) == sorted(fx)
        for k in fx:
            assert again[k].dtype == fx[k].dtype and again[k].shape == fx[k].shape, k
            assert np.array_equal(again[k], fx[k], equal_nan=fx[k].dtype == D), "the probe and the committed fixture differ in %s" % k


def test_the_two_restatements_are_bit_identical_on_the_recorded_scripts(world):
    mod, fx, table, runs = world
    for name, run in runs.items():
        for k, (a, b) in enumerate(zip(run["after"], run["scalar"])):
            for key in a:
                assert gc.same_bits(np.asarray(a[key]), np.asarray(b[key]).astype(np.asarray(a[key]).dtype)), (name, k, run["script"][k], key)


@pytest.mark.parametrize("kind", ["fr", "tf"])
def test_branch_mask_and_restarts_equal_the_references(world, kind):
    """EXACTLY, at every call of every vehicle: the branch, the finite / non-finite mask of mean, correction and covariance,
    _initialized, _numResets and both timers, and per measurement the number of singular restarts -- in the FREE-RUNNING
    record (kind fr: the reference ran on its own dense products from the constructor on) and teacher-forced (tf).  Before
    the definition took the dense algebra's non-finite behaviour this failed at the phase groups with one and two ordinary
    Predicts between alignment and first measurement: the definition made an ordinary update on a covariance whose
    attitude rows were NaN and handed on a NaN velocity and attitude; the reference restarts."""
    mod, fx, table, runs = world
    for name, run in runs.items():
        n, script = run["n"], run["script"]
        branch = fx["%s_%s_branch" % (name, kind)]
        ints = fx["%s_%s_int" % (name, kind)]
        mask = mod.unpack(fx, "%s_%s_mask" % (name, kind), _shape(run, 97))
        for who, after in _restatements(run):
            m = 0
            for k, st in enumerate(after):
                called = branch[k] != gc.NO_CALL
                assert np.array_equal(st["branch"], branch[k]), \
                    "%s %s %s event %d %r: branches %r, the reference's %r" % (who, name, kind, k, script[k], st["branch"].tolist(), branch[k].tolist())
                got = np.concatenate([np.isfinite(st["est"]), np.isfinite(st["corr"]), np.isfinite(st["cov"])])
                bad = np.argwhere(got[:, called] != mask[k][:, called])
                assert bad.size == 0, "%s %s %s event %d %r: %d mask entries differ, first (entry, call) %r" % (who, name, kind, k, script[k], len(bad), bad[0].tolist())
                mine = np.stack([st["initialized"], st["num_resets"], st["last_predict_us"], st["last_update_us"]]).astype(np.int64)
                assert np.array_equal(mine[:, called], ints[k][:, called]), (who, name, kind, k, script[k])
                if script[k][0] == "measure":
                    singular = int(np.isin(st["branch"], (3, 4)).sum())
                    assert singular == fx["%s_fr_singular" % name][m] and (who != "checker" or singular == run["singular"][k]), (who, name, k)
                    m += 1


def _f_of(before, k, v, inputs):
    """f as the scalar restatement's jacobian_entries and off_identity_rows place it, from the state before the call"""
    now, a, w = inputs[k]
    dt = (int(now) - int(before["last_predict_us"][v])) * 1e-6
    R = ref.q_matrix(tuple(float(x) for x in before["est"][6:10, v]))
    rows = ref.off_identity_rows(dt, *ref.jacobian_entries(dt, R, tuple(map(float, a[:, v])), tuple(map(float, w[:, v])),
                                                           tuple(map(float, before["corr"][:, v]))))
    f = np.eye(9)
    for i, row in enumerate(rows):
        for kk, val in row:
            f[i, kk] = val
    return f.reshape(81), dt


def _decode(mod, fx, key, row, v, exact):
    off, cls = fx[key + "_off"][row, :, v], fx[key + "_cls"][row, :, v]
    return np.array([mod.decode(o, c, e) for o, c, e in zip(off, cls, exact)], D)


def test_everything_outside_eigen_is_bit_identical(world):
    """Teacher-forced: the reference started every call from the definition's state.  Bit for bit: the alignment (float
    norm, 1e-6f, acosf and `if (errno)`), dt from the timers, _pos, _vel, _att and _angVel after Predict, all 81 entries of f
    each in its place and with its sign, the process noise of :197-202 on the stand-in's product, innovationCov and deltaPos,
    the restart's members and ResetVariance's diagonal, and :248-252 on the reference's own dx."""
    mod, fx, table, runs = world
    cfg = ref.default_config()
    seen = {b: 0 for b in gc.CALL_BRANCHES}
    for name, run in runs.items():
        n, script, inputs = run["n"], run["script"], run["inputs"]
        imu = [k for k, ev in enumerate(script) if ev[0] == "imu"]
        mea = [k for k, ev in enumerate(script) if ev[0] == "measure"]
        branch = fx[name + "_tf_branch"]
        offzero = mod.unpack(fx, name + "_tf_offzero", (len(script), n))
        for k, ev in enumerate(script):
            before, after = run["before"][k], run["after"][k]
            for v in np.flatnonzero(branch[k] != gc.NO_CALL):
                b = gc.CALL_BRANCHES[branch[k, v]]
                seen[b] += 1
                where = (name, k, ev, int(v), b)
                r_est, r_corr, r_diag = fx[name + "_tf_est"][k, :, v], fx[name + "_tf_corr"][k, :, v], fx[name + "_tf_diag"][k, :, v]
                if b != "update":
                    assert gc.same_bits(after["est"][:, v], r_est), where
                    assert gc.same_bits(after["corr"][:, v], r_corr), where
                if b not in ("update", "predict"):                # ResetVariance, or a covariance nobody touched (first Predict: Reset's)
                    C = after["cov"][:, v].reshape(9, 9)
                    assert gc.same_bits(np.diag(C).copy(), r_diag), where
                    assert offzero[k, v] == bool((C[~np.eye(9, dtype=bool)] == 0).all()), where
                if b == "predict":
                    r = imu.index(k)
                    f, dt = _f_of(before, k, v, inputs)
                    assert gc.same_bits(f, fx[name + "_tf_f"][r, :, v]), (where, np.flatnonzero(gc.differing(f, fx[name + "_tf_f"][r, :, v])))
                    # the stand-in's C of :195, then the reference's own += of :197-202
                    P = before["cov"][:, v]
                    T = _decode(mod, fx, name + "_tf_T", r, v, [x for x, _ in mod.product_exact(f, P, 9, 9, 9)])
                    C = _decode(mod, fx, name + "_tf_C", r, v, [x for x, _ in mod.product_exact(T, f.reshape(9, 9).T.reshape(81), 9, 9, 9)])
                    want = np.diag(C.reshape(9, 9)).copy()
                    for i in range(3):
                        want[3 + i] = want[3 + i] + cfg["sigma_acc"] * cfg["sigma_acc"] * dt * dt
                        want[6 + i] = want[6 + i] + cfg["sigma_gyro"] * cfg["sigma_gyro"] * dt * dt
                    assert gc.same_bits(want, r_diag), where
                if b in ("update", "singular_tiny", "singular_nonfinite"):
                    r = mea.index(k)
                    P = [[float(x) for x in before["cov"][9 * i:9 * i + 9, v]] for i in range(9)]
                    S, det, adj = ref.innovation(P, R_POS)
                    assert gc.same_bits(np.array(S).reshape(9), fx[name + "_tf_S"][r, :, v]) or ref.tainted(P), where
                    assert not np.isfinite(fx[name + "_tf_S"][r, :, v]).any() or not ref.tainted(P), where   # dense: a tainted P, S all non-finite
                if b == "update":
                    z = inputs[k][1][:, v]
                    d = z - before["est"][0:3, v]
                    assert gc.same_bits(d, fx[name + "_tf_d"][r, :, v]), where
                    # :248-252 on the reference's own dx: its dx is what its L and deltaPos give, decoded from the tape
                    S3 = [[float(x) for x in fx[name + "_tf_S"][r, 3 * i:3 * i + 3, v]] for i in range(3)]
                    fin = bool(np.isfinite(d).all())
                    chain = mod.update_chain(P, S3, [float(x) if fin else 0.0 for x in d])
                    inv = _decode(mod, fx, name + "_tf_inv", r, v, [x for row in chain["inv"][0] for x in row])
                    PH = np.array(P)[:, 0:3].reshape(27)
                    L = _decode(mod, fx, name + "_tf_L", r, v, [x for x, _ in mod.product_exact(PH, inv, 9, 3, 3)])
                    dx = _decode(mod, fx, name + "_tf_dx", r, v, [x for x, _ in mod.product_exact(L, d, 9, 3, 1)])
                    assert gc.same_bits(dx[6:9], r_corr), where
                    e = before["est"][:, v]
                    want = np.concatenate([e[0:3] + dx[0:3], e[3:6] + dx[3:6],
                                           ref.q_mul(tuple(map(float, e[6:10])), ref.from_rotvec(tuple(map(float, dx[6:9])), table)), e[10:13]])
                    assert gc.same_bits(want, r_est), where
    print(seen)
    assert all(seen[b] > 0 for b in gc.CALL_BRANCHES), seen


def _held(ratios, what, got, exact, bound, where):
    err = abs(Fraction(float(got)) - exact)
    assert err <= bound, "%s: off by %.3g, the bound is %.3g at %r" % (what, float(err), float(bound), where)
    if bound > 0:
        ratios[what] = max(ratios.get(what, 0.0), float(err / bound))


def test_order_dependent_results_are_within_their_derived_bounds(world):
    """Teacher-forced.  Every result on the stand-in's tape against the exact value of its recorded operands, and the
    definition's results against the exact value from the same primary operands; both within the bounds derived at the head
    of this file (the module's docstring carries the derivation).  Prints the worst ratio to each bound."""
    mod, fx, table, runs = world
    U = mod.U
    cfg = ref.default_config()
    ratios = {}
    n_predict = n_update = 0
    for name, run in runs.items():
        script, inputs = run["script"], run["inputs"]
        imu = [k for k, ev in enumerate(script) if ev[0] == "imu"]
        mea = [k for k, ev in enumerate(script) if ev[0] == "measure"]
        branch = fx[name + "_tf_branch"]
        for k, ev in enumerate(script):
            before, after = run["before"][k], run["after"][k]
            for v in np.flatnonzero(branch[k] != gc.NO_CALL):
                b = gc.CALL_BRANCHES[branch[k, v]]
                where = (name, k, int(v), b)
                P = before["cov"][:, v]
                if b == "predict" and np.isfinite(P).all():
                    r = imu.index(k)
                    f = fx[name + "_tf_f"][r, :, v]
                    if not np.isfinite(f).all():
                        continue                                       # (a NaN sample or correction: the masks are held exactly, above)
                    n_predict += 1
                    dt = float(f[3])
                    # the stand-in, product by product
                    ex1 = mod.product_exact(f, P, 9, 9, 9)
                    T = _decode(mod, fx, name + "_tf_T", r, v, [x for x, _ in ex1])
                    ex2 = mod.product_exact(T, f.reshape(9, 9).T.reshape(81), 9, 9, 9)
                    C = _decode(mod, fx, name + "_tf_C", r, v, [x for x, _ in ex2])
                    for got, (x, ab) in zip(T, ex1):
                        _held(ratios, "stand-in f * _cov", got, x, mod.gamma(9) * ab, where)
                    for got, (x, ab) in zip(C, ex2):
                        _held(ratios, "stand-in (f * _cov) * f'", got, x, mod.gamma(9) * ab, where)
                    # the definition (and the stand-in) against f P f' exactly
                    Cx, Bx = mod.predict_bound([float(x) for x in f], [float(x) for x in P])
                    q = [0.0] * 3 + [cfg["sigma_acc"] * cfg["sigma_acc"] * dt * dt] * 3 + [cfg["sigma_gyro"] * cfg["sigma_gyro"] * dt * dt] * 3
                    for i in range(9):
                        for j in range(9):
                            x, bd = Cx[9 * i + j], Bx[9 * i + j]
                            _held(ratios, "stand-in f P f'", C[9 * i + j], x, bd, where)
                            if i == j and i >= 3:
                                x, bd = x + Fraction(q[i]), bd + U * (abs(x) + bd + Fraction(q[i]))
                            _held(ratios, "definition f P f'", after["cov"][9 * i + j, v], x, bd, where)
                if b == "update":
                    r = mea.index(k)
                    n_update += 1
                    P9 = [[float(x) for x in P[9 * i:9 * i + 9]] for i in range(9)]
                    S3 = [[float(x) for x in fx[name + "_tf_S"][r, 3 * i:3 * i + 3, v]] for i in range(3)]
                    d = fx[name + "_tf_d"][r, :, v]
                    fin = bool(np.isfinite(d).all())
                    chain = mod.update_chain(P9, S3, [float(x) if fin else 0.0 for x in d])
                    flat = {q: ([x for row in chain[q][0] for x in row], [x for row in chain[q][1] for x in row]) for q in ("inv", "L", "M", "cov")}
                    flat["dx"] = chain["dx"]
                    # determinant(): the stand-in's and the definition's
                    det_x, Ed = mod.det_exact_and_bound([[Fraction(x) for x in row] for row in S3])
                    _held(ratios, "stand-in determinant()", _decode(mod, fx, name + "_tf_det", r, v, [det_x])[0], det_x, Ed, where)
                    S, det, adj = ref.innovation(P9, R_POS)
                    _held(ratios, "definition determinant()", det, det_x, Ed, where)
                    assert abs(abs(det_x) - Fraction(1e-10)) > Ed, where
                    # the stand-in's tape, decoded link by link, each against its own operands and against the chain
                    inv = _decode(mod, fx, name + "_tf_inv", r, v, flat["inv"][0])
                    exL = mod.product_exact(np.array(P9)[:, 0:3].reshape(27), inv, 9, 3, 3)
                    L = _decode(mod, fx, name + "_tf_L", r, v, [x for x, _ in exL])
                    exd = mod.product_exact(L, d, 9, 3, 1)
                    dx = _decode(mod, fx, name + "_tf_dx", r, v, [x for x, _ in exd])
                    N = (np.eye(9) - np.concatenate([L.reshape(9, 3), np.zeros((9, 6))], 1)).reshape(81)
                    exM = mod.product_exact(N, P, 9, 9, 9)
                    M = _decode(mod, fx, name + "_tf_M", r, v, [x for x, _ in exM])
                    for what, got, ex, g in (("stand-in _cov * H' * Sinv", L, exL, mod.gamma(3)), ("stand-in (I - L H) * _cov", M, exM, mod.gamma(9))) + \
                            ((("stand-in L * deltaPos", dx, exd, mod.gamma(3)),) if fin else ()):
                        for a, (x, ab) in zip(got, ex):
                            _held(ratios, what, a, x, g * ab, where)
                    Mm = M.reshape(9, 9)
                    for q, got in (("inv", inv), ("L", L), ("M", M), ("cov", (0.5 * (Mm + Mm.T)).reshape(81))) + ((("dx", dx),) if fin else ()):
                        for a, x, bd in zip(got, *flat[q]):
                            _held(ratios, "stand-in chain " + q, a, x, bd, where)
                    # the definition against the chain
                    Ld = ref.gain(P9, det, adj)
                    for a, x, bd in zip([x for row in Ld for x in row], *flat["L"]):
                        _held(ratios, "definition L", a, x, bd, where)
                    for a, x, bd in zip(after["cov"][:, v], *flat["cov"]):
                        _held(ratios, "definition covariance update", a, x, bd, where)
                    if fin:
                        e0 = before["est"][:, v]
                        for i in range(3):
                            _held(ratios, "definition correction", after["corr"][i, v], flat["dx"][0][6 + i], flat["dx"][1][6 + i], where)
                        for i in range(6):
                            x, bd = Fraction(float(e0[i])) + flat["dx"][0][i], flat["dx"][1][i]
                            bd = bd + U * (abs(Fraction(float(e0[i]))) + abs(flat["dx"][0][i]) + bd)
                            _held(ratios, "definition mean", after["est"][i, v], x, bd, where)
                        # the rotation vector's norm stays on its side of MIN_ANGLE
                        norm = math.sqrt(float(sum(x * x for x in flat["dx"][0][6:9])))
                        slack = math.sqrt(float(sum(x * x for x in flat["dx"][1][6:9]))) + 4 * 2.0 ** -53 * norm
                        assert abs(norm - ref.MIN_ANGLE) > slack, where
    print("predicts %d, updates %d; worst ratio to each bound:" % (n_predict, n_update))
    for what in sorted(ratios):
        print("    %-36s %.4g" % (what, ratios[what]))
    assert n_predict > 200 and n_update > 50
    assert max(ratios.values()) <= 1.0


def test_the_scripts_take_every_branch_reachable_behind_reset(world):
    mod, fx, table, runs = world
    total = {b: sum(run["count"][b] for run in runs.values()) for b in ref.BRANCHES}
    print(total)
    for b in gc.SCRIPT_BRANCHES:
        assert total[b] > 0, b
    assert total["acos_domain_neg"] == 0 and total["acos_domain_pos"] == 0


def test_this_machines_libm_against_the_recorded_table(world):
    """Every argument the restatements asked for is in the recorded table (one that is not means a restatement evaluated
    another argument than the definition did when the table was recorded; the tests above say which number moved).  Whether
    this machine's libm reproduces the table is not a requirement of the pin, a finding worth printing."""
    mod, fx, table, runs = world
    assert not table.misses, table.misses[:4]
    print("this machine's libm against the recorded table:", table.first_entry_libm_misses() or "every entry reproduced")
