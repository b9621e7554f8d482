"""The GPS + IMU estimator's definition on the CPU: the scalar restatement (tests/gps_imu_reference.py) against the numpy
checker (tests/gps_estimator_checker.py) bit for bit, the evaluation order this project fixes against numpy's dense
products, the configuration defaults through the library, and the scripted call list's branch table."""
import numpy as np

from tests import gps_estimator_checker as gc
from tests import gps_imu_reference as ref

N = 20


def _scalar_run(script, inputs, n, math=ref.glibc_math):
    clock = ref.Clock()
    ests = [ref.GPSIMUStateEstimator(clock, math=math) for _ in range(n)]
    states = []
    for k, ev in enumerate(script):
        if ev[0] == "imu":
            now, a, w = inputs[k]
            clock.us = now
            for v, e in enumerate(ests):
                e.Predict(tuple(float(x) for x in a[:, v]), tuple(float(x) for x in w[:, v]))
        elif ev[0] == "measure":
            now, z = inputs[k]
            clock.us = now
            for v, e in enumerate(ests):
                e.UpdateWithMeasurement(tuple(float(x) for x in z[:, v]))
        elif ev[0] == "reset":
            clock.us = inputs[k]
            for e in ests[ev[1]:ev[1] + ev[2]]:
                e.Reset()
        else:
            e13, c81, k3 = gc.payload(ev[1], ev[3], inputs[k])
            for i, e in enumerate(ests[ev[2]:ev[2] + ev[3]]):
                e.pos, e.vel = tuple(map(float, e13[0:3, i])), tuple(map(float, e13[3:6, i]))
                e.att, e.ang_vel = tuple(map(float, e13[6:10, i])), tuple(map(float, e13[10:13, i]))
                e.cov = [[float(c81[9 * a + b, i]) for b in range(9)] for a in range(9)]
                e.corr = tuple(map(float, k3[:, i]))
                e.initialized = True
        states.append({"est": np.array([e.GetCurrentEstimate() for e in ests]).T, "cov": np.array([np.array(e.cov).reshape(81) for e in ests]).T,
                       "last_predict_us": np.array([e.estimate_timer.reset_us for e in ests], np.uint64),
                       "last_update_us": np.array([e.last_good.reset_us for e in ests], np.uint64),
                       "initialized": np.array([e.initialized for e in ests], np.uint8),
                       "num_resets": np.array([e.num_resets for e in ests], np.uint32)})
    count = {b: sum(e.count[b] for e in ests) for b in ref.BRANCHES}
    return states, count


def test_scalar_reference_and_numpy_checker_are_bit_identical_and_the_script_reaches_every_branch():
    for n in (N, 1):
        script = gc.make_script(n)
        inputs = gc.synthetic_inputs(script, n)
        want, want_count = _scalar_run(script, inputs, n)
        chk = gc.Estimator(n)
        got, _ = gc.run_script(script, chk, inputs)
        for k, (a, b) in enumerate(zip(got, want)):
            for f in a:
                assert gc.same_bits(a[f], b[f]), (n, k, script[k], f)
        assert chk.count == want_count, (chk.count, want_count)
        print(n, chk.count)
        reach = [b for b in gc.SCRIPT_BRANCHES if not (n == 1 and b in ("measure_before_predict", "nan_position", "first_predict_tilted"))]
        for b in reach:
            assert chk.count[b] > 0, (n, b, chk.count)
        assert chk.count["acos_domain_neg"] == 0 and chk.count["acos_domain_pos"] == 0      # (unreachable behind Reset(), see the checker)
        assert np.isfinite(got[-1]["cov"][:, :max(1, n - 1)]).all()


def test_the_acosf_domain_branches_through_the_alignment_itself():
    """Predict aligns an identity attitude, from which |float(cosAngleError)| > 1 cannot arise; the lines (:79-100) are
    written for any attitude, and with a non-unit one both sides of `if (errno)` are reached -- in both restatements, with
    the same bits.  A NaN argument is neither: acosf sets no errno for it."""
    rng = np.random.default_rng(5)
    n = 64
    q = rng.normal(size=(4, n))
    q = q / np.sqrt((q * q).sum(0)) * np.where(np.arange(n) % 2 == 0, 1.5, 1.0)
    acc = rng.normal(0, 5, (3, n)).astype(np.float32).astype(np.float64)
    acc[:, 0] = np.nan
    count = {b: 0 for b in ref.BRANCHES}
    with np.errstate(all="ignore"):
        got = gc.align(q, acc, ref.glibc_math, count)
    scalar_count = {b: 0 for b in ref.BRANCHES}
    want = np.array([ref.align(tuple(map(float, q[:, v])), tuple(map(float, acc[:, v])), ref.glibc_math, scalar_count) for v in range(n)]).T
    assert gc.same_bits(got, want) and count == scalar_count
    assert count["acos_domain_neg"] > 0 and count["acos_domain_pos"] > 0
    assert np.isnan(got[:, 0]).all()
    # the angle of a domain error is pi or 0 exactly: the quaternion appended is (cos(pi/2), sin(pi/2) axis) or (1, 0 axis)
    assert ref._scalar(ref.glibc_math, 2, 1.0) == 0.0 and abs(ref._scalar(ref.glibc_math, 2, -1.0) - np.pi) < 1e-6


# The sparse order against numpy's dense F @ P @ F.T and (I - L H) P on the covariances of the scripted flight, n = 20:
# largest |sparse - dense| / max|dense| over every finite matrix (1400 of them), measured with
#     python -m pytest tests/test_gps_estimator_cpu.py -k sparse -s
SPARSE_VS_DENSE_PREDICT = 3.69e-16
SPARSE_VS_DENSE_UPDATE = 3.0e-16


def _dense_f(dt, measAcc, measGyro, corr, rotMat):
    """f of GPSIMUStateEstimator.cpp:126-191, assignment by assignment as the reference writes them (not through the
    restatement's rows): what places and signs the entries have is judged by this"""
    I_POS, I_VEL, I_ATT = 0, 3, 6
    x, y, z = 0, 1, 2
    f = np.zeros((9, 9))
    for i in range(3):
        f[I_POS + i, I_POS + i] = 1                                  # :129-131
        f[I_POS + i, I_VEL + i] = dt                                 # :134-136
        f[I_VEL + i, I_VEL + i] = 1                                  # :139-141
    f[I_VEL + 0, I_ATT + 0] = dt * (+measAcc[y] * rotMat[3 * 0 + 2] - measAcc[z] * rotMat[3 * 0 + 1])     # :147-152
    f[I_VEL + 1, I_ATT + 0] = dt * (+measAcc[y] * rotMat[3 * 1 + 2] - measAcc[z] * rotMat[3 * 1 + 1])
    f[I_VEL + 2, I_ATT + 0] = dt * (+measAcc[y] * rotMat[3 * 2 + 2] - measAcc[z] * rotMat[3 * 2 + 1])
    f[I_VEL + 0, I_ATT + 1] = dt * (-measAcc[x] * rotMat[3 * 0 + 2] + measAcc[z] * rotMat[3 * 0 + 0])     # :157-162
    f[I_VEL + 1, I_ATT + 1] = dt * (-measAcc[x] * rotMat[3 * 1 + 2] + measAcc[z] * rotMat[3 * 1 + 0])
    f[I_VEL + 2, I_ATT + 1] = dt * (-measAcc[x] * rotMat[3 * 2 + 2] + measAcc[z] * rotMat[3 * 2 + 0])
    f[I_VEL + 0, I_ATT + 2] = dt * (+measAcc[x] * rotMat[3 * 0 + 1] - measAcc[y] * rotMat[3 * 0 + 0])     # :167-172
    f[I_VEL + 1, I_ATT + 2] = dt * (+measAcc[x] * rotMat[3 * 1 + 1] - measAcc[y] * rotMat[3 * 1 + 0])
    f[I_VEL + 2, I_ATT + 2] = dt * (+measAcc[x] * rotMat[3 * 2 + 1] - measAcc[y] * rotMat[3 * 2 + 0])
    f[I_ATT + 0, I_ATT + 0] = 1                                      # :175-191
    f[I_ATT + 1, I_ATT + 0] = -(dt * measGyro[z] + corr[z] / 2.0)
    f[I_ATT + 2, I_ATT + 0] = +(dt * measGyro[y] + corr[y] / 2.0)
    f[I_ATT + 0, I_ATT + 1] = +(dt * measGyro[z] + corr[z] / 2.0)
    f[I_ATT + 1, I_ATT + 1] = 1
    f[I_ATT + 2, I_ATT + 1] = -(dt * measGyro[x] + corr[x] / 2.0)
    f[I_ATT + 0, I_ATT + 2] = -(dt * measGyro[y] + corr[y] / 2.0)
    f[I_ATT + 1, I_ATT + 2] = +(dt * measGyro[x] + corr[x] / 2.0)
    f[I_ATT + 2, I_ATT + 2] = 1
    return f


def test_the_sparse_order_is_the_dense_formula():
    """F P F' and (I - L H) P, then 0.5 (C + C'), as the reference writes them (:195, :255-256), in numpy's dense products
    against the order the definition fixes, on the flight's own covariances (every one of the scripted flight, after every
    event; the ones that are not finite are held to the dense product's mask) with a representative F and the gain of that
    covariance.  Largest relative difference (of the largest
    entry of the dense result) measured from the dense product: 3.69e-16 for the prediction and 3.0e-16 for the update;
    twice the recorded constants is asserted."""
    n = N
    script = gc.make_script(n)
    inputs = gc.synthetic_inputs(script, n)
    chk = gc.Estimator(n)
    states, _ = gc.run_script(script, chk, inputs)
    rng = np.random.default_rng(1)
    worst_p = worst_u = 0.0
    seen = seen_nonfinite = 0
    for st in states:
        P_all = st["cov"].reshape(9, 9, n)
        for v in range(n):
            P = P_all[:, :, v]
            dt = 0.002
            q = rng.normal(size=4)
            q = q / np.sqrt((q * q).sum())
            a, w, k = rng.normal(0, 6, 3), rng.normal(0, 1.5, 3), rng.normal(0, 1e-3, 3)
            R = ref.q_matrix(tuple(q))
            rows = ref.off_identity_rows(dt, *ref.jacobian_entries(dt, R, tuple(a), tuple(w), tuple(k)))
            Fm = _dense_f(dt, a, w, k, R)
            Fs = np.eye(9)
            for i, row in enumerate(rows):
                for kk, val in row:
                    Fs[i, kk] = val
            assert np.array_equal(Fs, Fm), (Fs - Fm)                # every entry in its place, with its sign
            H = np.zeros((3, 9))
            H[0, 0] = H[1, 1] = H[2, 2] = 1.0
            sparse = np.array(ref.predict_covariance(P.tolist(), rows))
            if not np.isfinite(P).all():
                # a covariance that is not finite: the definition's mask is the dense product's, all terms summed by hand
                # (k ascending; a BLAS may skip or reorder, the mask of an all-terms sum does not depend on the order).
                # Every entry is non-finite; it is NaN wherever the dense product's is (a lone infinity at (k, l) stays
                # an infinity in the dense product where F[i][k] and F[j][l] are both non-zero, and is NaN in the
                # definition: see afe_gps_estimator.hip, NON-FINITE NUMBERS).  The dense S is non-finite: :230-236.
                with np.errstate(all="ignore"):
                    T = np.array([[sum(Fm[i, k] * P[k, j] for k in range(9)) for j in range(9)] for i in range(9)])
                    dense = np.array([[sum(T[i, k] * Fm[j, k] for k in range(9)) for j in range(9)] for i in range(9)])
                    PH = np.array([[sum(P[i, k] * H[j, k] for k in range(9)) for j in range(3)] for i in range(9)])
                    Sd = np.array([[sum(H[i, k] * PH[k, j] for k in range(9)) for j in range(3)] for i in range(3)]) + 0.0625 * np.eye(3)
                assert np.array_equal(np.isfinite(sparse), np.isfinite(dense)) and not np.isfinite(dense).any(), (np.isfinite(sparse), np.isfinite(dense))
                assert np.isnan(sparse)[np.isnan(dense)].all()
                assert not np.isfinite(Sd).any() and ref.tainted(P.tolist())
                seen_nonfinite += 1
                continue
            dense = Fm @ P @ Fm.T
            worst_p = max(worst_p, np.abs(sparse - dense).max() / np.abs(dense).max())
            S, det, adj = ref.innovation(P.tolist(), 0.0625)
            if abs(det) < 1e-10:
                continue
            L = np.array(ref.gain(P.tolist(), det, adj))
            Ld = P @ H.T @ np.linalg.inv(np.array(S))
            C = (np.eye(9) - Ld @ H) @ P
            dense_u = 0.5 * (C + C.T)
            sparse_u = np.array(ref.update_covariance(P.tolist(), L.tolist()))
            worst_u = max(worst_u, np.abs(sparse_u - dense_u).max() / np.abs(dense_u).max())
            seen += 1
    print("sparse against dense: predict %.3g, update %.3g over %d covariances" % (worst_p, worst_u, seen))
    assert seen > 200 and seen_nonfinite > 50
    assert worst_p <= 2 * SPARSE_VS_DENSE_PREDICT and worst_u <= 2 * SPARSE_VS_DENSE_UPDATE


def test_config_defaults_through_the_library():
    import importlib
    afa = importlib.import_module("agri-fly_amd")
    c = afa.gps_estimator_default_config()
    assert gc.config_from(c) == ref.default_config()
    import ctypes as C
    assert c.struct_bytes == C.sizeof(afa.GpsEstimatorConfig)
    assert afa.library().afe_gps_estimator_default_config(None) == 1


def test_one_ulp_of_the_functions_stays_inside_the_followers_code_cap():
    """The GPU test compares the codes an attached follower sends on the device's estimate with those of glibc's estimator
    under glibc's follower, and allows one code in at most 1 % of the values (the follower tests' cap).  Here, without a
    GPU: the checker with glibc's functions against the checker with every function result moved one ulp up, 130 vehicles
    over the scripted flight, then one tick of follower_checker on each estimate -- the same cap holds."""
    from tests import follower_checker as fc
    n = 130
    script = gc.make_script(n)
    inputs = gc.synthetic_inputs(script, n)
    ests = []
    for math in (ref.glibc_math, gc.nudged(ref.glibc_math)):
        chk = gc.Estimator(n, math=math)
        states, _ = gc.run_script(script, chk, inputs)
        ests.append(states[-1]["est"])
    now = inputs[-1][0]
    assert now >= 100000
    plans = fc.make_plans(ests[0][0:3], 5, now)
    cfg = fc.default_config()
    sent = [fc.tick(s[0:3], s[3:6], s[6:10], plans, cfg, now, fc.glibc_math)["sent"][:, :n - 1] for s in ests]
    dist = fc.code_distance(sent[0], sent[1])
    drift = np.nanmax(np.abs(ests[0][:, :n - 1] - ests[1][:, :n - 1]))
    print("one ulp carries %.3g into the estimate; %d of %d sent codes differ, largest distance %d" % (drift, np.count_nonzero(dist), dist.size, dist.max()))
    assert 0 < drift < 1e-9
    assert dist.max() <= 1 and np.count_nonzero(dist) <= 0.01 * dist.size


# The estimate against the truth.  Largest position, velocity and tilt error of the checker (glibc's functions) against the
# CPU oracle's closed-loop flight of tests/gps_truth_flight.py, behind every update from the first on (59 updates, 299
# Predict calls, 24 vehicles), measured with
#     python -m pytest tests/test_gps_estimator_cpu.py -k truth -s
# tests/test_gpu_gps_estimator.py asserts the device's estimate against the engine's own truth within twice these.
TRUTH_POSITION_M = 1.6566e-3
TRUTH_VELOCITY_M_S = 6.4513e-2
TRUTH_TILT_RAD = 1.15126e-2


def test_estimate_against_truth_on_the_oracles_flight(ora):
    """the one check of the estimate against something independent of the restatement: the oracle flies, the checker
    estimates, and the estimate stays within millimetres, centimetres per second and a degree of where the vehicles are.
    The figures are recorded above (and must stay what is measured: 0.1 %)."""
    import importlib
    from tests import gps_truth_flight as tf
    afa = importlib.import_module("agri-fly_amd")
    r = tf.fly_oracle(ora, afa)
    print("checker against the oracle's flight: position %.5g m, velocity %.5g m/s, tilt %.6g rad; %d ticks, %d updates"
          % (r["worst"] + (r["n_ticks"], r["n_updates"])))
    assert (r["n_ticks"], r["n_updates"]) == (299, 59)
    assert r["counts"]["update"] == 58 * tf.N and r["counts"]["singular_nonfinite"] == tf.N      # the first update re-initialises (NaN correction)
    for got, recorded in zip(r["worst"], (TRUTH_POSITION_M, TRUTH_VELOCITY_M_S, TRUTH_TILT_RAD)):
        assert abs(got - recorded) <= 1e-3 * recorded, (got, recorded)
    assert r["worst"][0] < 0.01 and r["worst"][1] < 0.2 and r["worst"][2] < 0.05           # it tracks
