"""The step checker (oracle/agrifly_oracle.c: ora_step_batch, ora_clock_run, ora_params_init) against what the REFERENCE's
own Quadcopter_T::Run computed: tests/golden/rigid_body_reference.npz is what oracle/_ref/rigid_body_probe recorded --
Quadcopter_T.cpp and Motor.cpp compiled where they lie against the storage-only oracle/eigen_store, with a logic stub
that records the IMU floats and replays a command script -- on 96 vehicles in five (dt, logic period) groups.  Both sides
are double, -ffp-contract=off, the same libm and the same libstdc++ generator: everything is compared bit for bit, the
IMU floats and their minstd_rand0 noise included.  The one Eigen operation of the path, inertiaMatrix.inverse()
(Quadcopter_T.cpp:20), is injected into the probe from ora_params_init and judged here against the exact inverse.  CPU only."""
import importlib.util
import os
import re
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = ("pos", "vel", "att", "ang_vel", "motor_speed")


def _generator():
    spec = importlib.util.spec_from_file_location("make_rigid_body_reference", os.path.join(ROOT, "tests", "golden", "make_rigid_body_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ref():
    mod = _generator()
    return mod, mod.load_fixture()


def test_fixture_holds_the_cases(ref):
    mod, fx = ref
    assert len(fx["group"]) == 96 and fx["ref_pos"].shape == (96, 4, 3)
    mod.check_coverage(fx)      # every line of Run() reached, |w| dt <= 0.5 rad everywhere, the fp32 cap on pos.z
    assert np.array_equal(fx["fp32_ok"], mod.fp32_ok(fx)) and fx["fp32_ok"].all()     # no case is excluded from any comparison
    pairs = {(int(d), float(p)) for d, p in zip(fx["group_dt_us"], fx["group_period"])}
    assert {(1000, 1 / 500), (2000, 1 / 500), (250, 1 / 1000), (1000, 0.0033), (0, 1 / 500)} <= pairs
    assert (float(fx["sigma_gyro"]), float(fx["sigma_acc"])) == (0.1, 0.2)
    assert os.path.getsize(mod.FIXTURE) <= 128 * 1024


def _bits(a, dtype):
    return np.ascontiguousarray(a, dtype).tobytes()


def test_checker_steps_like_the_reference_bit_for_bit(ora, afa, ref):
    """ora_step_batch on every case, driven by the checker's own clock (ora_clock_run: dt and the logic gate): position,
    velocity, attitude, body rates, rotor speeds, the gyro and accelerometer floats with their noise, the commands in
    force and the tick count, at every checkpoint of every case; the tick pattern of every group, which is also
    afa.plan_ticks'.  The dt 0 group is Quadcopter_T.cpp:88-90's early return: the clock hands back 0 and nothing runs."""
    import ctypes as C
    mod, fx = ref
    compared = 0
    for gi in range(len(fx["group_dt_us"])):
        idx = mod.group_cases(fx, gi)
        dt_us, period, steps = int(fx["group_dt_us"][gi]), float(fx["group_period"][gi]), int(fx["group_steps"][gi])
        want_tick = mod.group_ticks(fx, gi)
        if dt_us > 0:
            np.testing.assert_array_equal(afa.plan_ticks(period, 0, dt_us, steps)[0], want_tick)
        table = [mod.oracle_params(ora, fx, i) for i in idx]
        for i, o in zip(idx, table):
            assert _bits(list(o.inertia_inv), np.float64) == _bits(fx["in_inverse"][i], np.float64)     # what the probe was handed
            assert (o.sigma_gyro, o.sigma_acc) == (0.1, 0.2) and list(o.R_imu_inv) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
        b = ora.Batch(len(idx), table, np.arange(len(idx)))
        for k in ("pos", "vel", "att", "ang_vel", "ext_force", "ext_torque"):
            getattr(b, k)[:] = fx["in_" + k][idx].T
        clock = ora.OraClock()
        ora.lib().ora_clock_init(C.byref(clock), period)
        rows = mod.script_rows(max(int(fx["group_ticks"][gi]), 1))
        b.motor_cmd[:] = fx["cmd_sets"][idx, 0].T
        runs, tick, cp = 0, C.c_int(0), mod.checkpoints(steps)
        for s in range(1, steps + 1):
            ora.lib().ora_clock_advance(C.byref(clock), dt_us)
            dt = ora.lib().ora_clock_run(C.byref(clock), C.byref(tick))
            assert tick.value == want_tick[s - 1], (gi, s)
            if dt > 0:
                b.step(dt, 1, ticks=[tick.value])
                if tick.value:        # Quadcopter_T.cpp:187-189: what the logic leaves takes effect at the next step
                    b.motor_cmd[:] = fx["cmd_sets"][idx, rows[runs]].T
                    runs += 1
            else:
                assert dt_us == 0
            if s in cp:
                c = cp.index(s)
                where = "group %d, after step %d" % (gi, s)
                np.testing.assert_array_equal(fx["ref_step"][idx, c], s)
                np.testing.assert_array_equal(fx["ref_ticks"][idx, c], runs, err_msg=where)
                for k in STATE:
                    got, want = getattr(b, k).T, fx["ref_" + k][idx, c]
                    bad = [int(idx[j]) for j in range(len(idx)) if _bits(got[j], np.float64) != _bits(want[j], np.float64)]
                    assert not bad, (where, k, bad[:8])
                for k, got in (("gyro", b.gyro), ("acc", b.acc), ("cmd", b.motor_cmd)):
                    want = fx["ref_" + k][idx, c]
                    bad = [int(idx[j]) for j in range(len(idx)) if _bits(got.T[j], np.float32) != _bits(want[j], np.float32)]
                    assert not bad, (where, k, bad[:8])
                compared += len(idx)
    assert compared == 96 * 4


def test_closed_loop_checker_equals_the_reference_headers_in_the_loop(ora, afa, ref):
    """tests/golden/rigid_body_closed_loop.npz: Quadcopter_T::Run with the reference's own LowPassFilterSecondOrder,
    QuadcopterAngularVelocityController and QuadcopterMixer headers in the loop (parameters from QuadcopterConstants), 12
    vehicles of the four shipped types, 150 steps, idle for 7 steps, then rates commands that change twice and reach the
    total-thrust cap and both per-propeller clamps.  ora.ClosedLoopBatch (ora_step_batch + ora_logic_tick) must equal the
    recording bit for bit at every checkpoint: state, rotor speeds, IMU floats, motor-speed commands and motor forces.
    What this pins: the restated controller, mixer, low-pass on a Vec3f and the type constants.  What it does not: the glue
    between them (first IMU call initialises only; thrust_norm * mass; idle until a rates command arrives), which is the
    probe's own reading of QuadcopterLogic.cpp / KalmanFilter6DOF.cpp, the same reading as the checker's."""
    mod, _ = ref
    fx = mod.load_fixture(mod.CL_FIXTURE)
    mod.check_closed_loop_coverage(fx, ora)
    n, dt_us, period = len(fx["type_id"]), int(fx["dt_us"]), float(fx["period"])
    np.testing.assert_array_equal(afa.plan_ticks(period, 0, dt_us, int(fx["steps"]))[0], fx["tick"])
    table = [mod.oracle_params(ora, fx, i) for i in range(n)]
    for i, o in enumerate(table):       # the probe's body is the shipped type's
        t = ora.params_from_type(int(fx["type_id"][i]))
        assert bytes(o) == bytes(t), i
    b = ora.Batch(n, table, np.arange(n))
    for k in ("pos", "vel", "att", "ang_vel", "ext_force", "ext_torque"):
        getattr(b, k)[:] = fx["in_" + k][:].T
    cl = ora.ClosedLoopBatch(b, [ora.logic_params_from_type(int(t), period) for t in fx["type_id"]], period)
    for a, e, row, c in mod.closed_loop_segments(fx):
        if row >= 0:
            cl.set_rates_cmd(fx["rows"][:, row, 1], fx["rows"][:, row, 2:5].T)
        cl.step(dt_us * 1e-6, fx["tick"][a:e])
        if c < 0:
            continue
        where = "after step %d" % e
        assert np.all(fx["ref_step"][:, c] == e) and np.all(fx["ref_ticks"][:, c] == fx["tick"][:e].sum())
        for k in STATE:
            assert _bits(getattr(b, k).T, np.float64) == _bits(fx["ref_" + k][:, c], np.float64), (where, k)
        force = np.array([list(s.motor_force_cmd) for s in cl.states], np.float32)
        for k, got in (("gyro", b.gyro.T), ("acc", b.acc.T), ("cmd", b.motor_cmd.T), ("force", force)):
            bad = [i for i in range(n) if _bits(got[i], np.float32) != _bits(fx["ref_" + k][i, c], np.float32)]
            assert not bad, (where, k, bad)


# ---- the injected inverse ---------------------------------------------------------------------------------------------
U = Fraction(1, 2 ** 53)          # unit roundoff of a double


def _exact_inverse(I):
    a = [Fraction(float(x)) for x in I]
    cof = lambda p, q, r, s: a[p] * a[q] - a[r] * a[s]
    terms = [(4, 8, 5, 7), (2, 7, 1, 8), (1, 5, 2, 4), (5, 6, 3, 8), (0, 8, 2, 6), (2, 3, 0, 5), (3, 7, 4, 6), (1, 6, 0, 7), (0, 4, 1, 3)]
    c = [cof(*t) for t in terms]
    c_abs = [abs(a[p] * a[q]) + abs(a[r] * a[s]) for p, q, r, s in terms]
    det = a[0] * c[0] + a[1] * c[3] + a[2] * c[6]
    det_abs = abs(a[0]) * c_abs[0] + abs(a[1]) * c_abs[3] + abs(a[2]) * c_abs[6]
    return [x / det for x in c], c_abs, det, det_abs


def test_injected_inverse_against_the_exact_one(ora, ref):
    """The nine numbers the probe was handed (ora_params_init: cofactors times 1 / det) against the exact inverse of the
    same doubles, in rationals.  The bounds count roundings (u = 2^-53 each, standard model), they are not fitted:

    A, power-of-two diagonal: every product, the reciprocal and the last product are exact -> the inverse is exact.
    B, diagonal: o_kk = (a_ii a_jj) * (1 / (a_kk * (a_ii a_jj))), four roundings on the path (the cofactor's product, the
       determinant's product, the reciprocal, the final product; the subtractions and additions meet exact zeros), so
       |o_kk - 1 / a_kk| <= ((1 + u)^4 - 1) / a_kk; off the diagonal 0 * x - 0 * y times anything is exactly 0.
    C, full: the longest path has nine roundings -- cofactor 2 (a product and the subtraction), determinant 5 (a cofactor,
       the product with a_0j, two additions), reciprocal 1, final product 1.  A cofactor's error is at most 2u C~_ij with
       C~_ij = |ab| + |cd|, the determinant's at most 5u D~ with D~ = sum |a_0j| C~_0j, so to first order
       |o_ij - exact| <= (2u C~_ij + |c_ij| (5u D~ / |det| + 2u)) / |det| <= 9u (C~_ij / |det|) (D~ / |det|).
       D~ / |det| >= 1 is the condition number of the determinant's sum and is required below 1e3 here, which keeps the
       second-order terms (at most (9u D~ / |det|)^2 relative) under the factor 1 + 1e-6.
    Observed: B at most 0.68 u relative, C at most 0.45 of its bound."""
    mod, fx = ref
    worst_b, worst_c, cond = Fraction(0), Fraction(0), Fraction(0)
    for i in range(len(fx["group"])):
        got = [Fraction(float(x)) for x in fx["in_inverse"][i]]
        exact, c_abs, det, det_abs = _exact_inverse(fx["in_inertia"][i])
        cls = int(fx["inertia_class"][i])
        if cls == 0:
            assert got == exact, i
        elif cls == 1:
            for k in range(9):
                if k in (0, 4, 8):
                    rel = abs(got[k] - exact[k]) / abs(exact[k])
                    assert rel <= (1 + U) ** 4 - 1, (i, k, float(rel / U))
                    worst_b = max(worst_b, rel / U)
                else:
                    assert got[k] == 0 and exact[k] == 0
        else:
            assert det > 0 and det_abs / det < 1000
            cond = max(cond, det_abs / det)
            for k in range(9):
                bound = 9 * U * (c_abs[k] / det) * (det_abs / det) * (1 + Fraction(1, 10 ** 6))
                assert abs(got[k] - exact[k]) <= bound, (i, k, float(abs(got[k] - exact[k]) / bound))
                worst_c = max(worst_c, abs(got[k] - exact[k]) / bound)
    print("inverse: class B worst %.3f u relative; class C worst %.3f of its bound, D~/|det| up to %.3f" % (float(worst_b), float(worst_c), float(cond)))


def test_fixture_is_what_the_probe_writes_now(ref):
    """staleness: the generator run again (needs oracle/_ref/rigid_body_probe, built where the reference is present).  The
    generator runs the probe twice on every request and requires identical bytes."""
    mod, fx = ref
    if not os.path.exists(mod.PROBE):
        pytest.skip("oracle/_ref/rigid_body_probe not built (the reference sources are not on this machine)")
    for fresh, old in ((mod.make_rigid_body_reference(mod.PROBE), fx), (mod.make_closed_loop_reference(mod.PROBE), mod.load_fixture(mod.CL_FIXTURE))):
        assert sorted(fresh) == sorted(old)
        for k in old:
            a, b = np.asarray(fresh[k]), old[k]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


# ---- the storage-only Eigen -------------------------------------------------------------------------------------------
STORE = os.path.join(ROOT, "oracle", "eigen_store")


def _gxx(args, text):
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        with open(src, "w") as f:
            f.write(text)
        return subprocess.run(["g++", "-std=c++11", "-I" + STORE] + args + [src], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_eigen_store_refuses_arithmetic_and_an_undefined_inverse():
    """oracle/eigen_store holds storage and constants: element access compiles and links; a product of two matrices is a
    COMPILE error; inverse() on a <float, 3, 3>, which no probe defines, compiles and fails to LINK."""
    ok = _gxx(["-o", "t"], "#include <Eigen/Dense>\nint main() { Eigen::Matrix<double, 3, 3> a = Eigen::Matrix<double, 3, 3>::Identity(); "
                           "a(1, 2) = 3; return a(1, 2) == 3 && a(4) == 1 && Eigen::Matrix<float, 2, 2>::Zero()(1, 1) == 0 ? 0 : 1; }\n")
    assert ok.returncode == 0, ok.stdout
    mul = _gxx(["-fsyntax-only"], "#include <Eigen/Dense>\nEigen::Matrix<double, 3, 3> a, b;\nint main() { a = a * b; }\n")
    assert mul.returncode != 0 and "operator*" in mul.stdout, mul.stdout
    inv = "#include <Eigen/Dense>\nEigen::Matrix<float, 3, 3> a;\nint main() { a = a.inverse(); }\n"
    assert _gxx(["-fsyntax-only"], inv).returncode == 0
    link = _gxx(["-o", "t"], inv)
    assert link.returncode != 0 and "undefined reference" in link.stdout and "inverse" in link.stdout, link.stdout
    with open(os.path.join(STORE, "Eigen", "Dense")) as f:
        code = [l for l in f if not l.lstrip().startswith("//")]
    assert not any("operator*" in l or "operator+" in l or "operator-" in l or "operator<<" in l for l in code)
    assert sum("inverse" in l for l in code) == 1          # the declaration, no definition


def test_probe_recipe_uses_the_storage_only_header():
    """the probe's include path names oracle/eigen_store and never tests/shim, Motor.cpp is compiled where it lies and
    Quadcopter_T.cpp is included from there; the flags are the checker's; built by `make ref`, i.e. by build()"""
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        mk = f.read()
    inc = re.search(r"^RIGID_INC\s*:=(.*)$", mk, re.M).group(1)
    src = re.search(r"^RIGID_SRC\s*:=(.*)$", mk, re.M).group(1)
    link = re.search(r"^RIGID_LINK\s*:=(.*)$", mk, re.M).group(1)
    recipe = re.search(r"^_ref/rigid_body_probe:.*\n((?:\t.*\n)+)", mk, re.M).group(1)
    assert all(v in recipe for v in ("$(RIGID_INC)", "$(RIGID_SRC)", "$(RIGID_LINK)")) and "-Ieigen_store" in inc.split()
    assert not any("shim" in t or "eigen_decl" in t for t in (inc, src, recipe))
    assert link.split() == ["-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections"]
    for flag in ("-ffp-contract=off", "-fno-fast-math", "-O2", "-std=c++11"):
        assert flag in recipe
    assert re.search(r"\$\(REF\)/\S*Motor\.cpp", src)
    assert "_ref/rigid_body_probe" in mk.split("\nref:")[1].split("\n\n")[0]
    with open(os.path.join(ROOT, "oracle", "ref_rigid_body_probe.cpp")) as f:
        probe = f.read()
    assert '#include "Components/Simulation/Quadcopter_T.cpp"' in probe and "Matrix<double, 3, 3>::inverse()" in probe
