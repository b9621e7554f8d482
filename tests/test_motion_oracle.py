"""The oracle's rotation math and rotor model (oracle/agrifly_oracle.c ora_rot_* and ora_motor_run, rows a4 / a5 of
DESIGN.md section 4) pinned BIT FOR BIT to the reference's own Rotation.hpp and Motor.cpp: tests/golden/motion_kat.json is
what oracle/_ref/motion_probe printed, the reference compiled in place against a declaration-only <Eigen/Dense>
(oracle/eigen_decl).  Both sides are double, -ffp-contract=off, the same libm.  CPU only."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "oracle", "_ref", "motion_probe")


@pytest.fixture(scope="module")
def kat(golden_dir):
    with open(os.path.join(golden_dir, "motion_kat.json")) as f:
        return json.load(f)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _call(fn, *ins, n_out):
    args = [np.ascontiguousarray(a, np.float64) for a in ins]
    out = np.zeros(n_out)
    fn(*[_dp(a) for a in args], _dp(out))
    return out


def motor_run(ora, case):
    """ora_motor_run over a case's schedule with the reference's clock: Timer::GetSeconds<double>() of the microseconds
    since the last Run() that did not return early (Motor.cpp:40-44), the outputs of the last effective Run() kept"""
    p = ora.params_from_type(case["type"])
    p.motor_min_speed, p.motor_max_speed = case["min_speed"], case["max_speed"]
    p.k_thrust, p.k_torque = case["k_thrust"], case["k_torque"]
    p.motor_time_const, p.motor_inertia = case["time_const"], case["inertia"]
    m = case["motor"]
    assert list(p.motor_pos[m]) == case["position"] and list(p.motor_rot_axis[m]) == case["rot_axis"]
    speed, since_us = 0.0, 0
    th, tq, L = np.zeros(3), np.zeros(3), np.zeros(3)
    rec = dict(speed=[], thrust=[], torque=[], ang_mom=[])
    for dt_us, cmd in zip(case["dt_us"], case["cmd"]):
        since_us += dt_us
        dt = since_us * 1e-6
        if not dt < 1e-6:
            since_us = 0
            pw = C.c_double(0)
            speed = ora.lib().ora_motor_run(C.byref(p), m, speed, cmd, dt, _dp(th), _dp(tq), _dp(L), C.byref(pw))
        rec["speed"].append(speed)
        rec["thrust"].append(th.tolist())
        rec["torque"].append(tq.tolist())
        rec["ang_mom"].append(L.tolist())
    return rec


def test_fixture_covers_the_edges(kat):
    """the cases the issue asks for are there: both neighbouring doubles of MIN_ANGLE, angles up to 2 pi + and past
    100 rad, every motor edge"""
    ma = kat["min_angle"]
    th = [np.linalg.norm(c["r"]) for c in kat["rotvec"]]
    assert np.nextafter(ma, 0) in th and np.nextafter(ma, 1) in th and ma in th and 0.0 in th
    steps = [np.linalg.norm(np.asarray(c["ang_vel"]) * c["dt"]) for c in kat["step"]]
    assert min(steps) == 0 and max(steps) > 900 and sum(abs(t - 2 * np.pi) < 2e-6 for t in steps) >= 6
    for c in kat["step"]:   # float32 values held in doubles: one fixture for both engines
        for k in ("att", "ang_vel"):
            assert np.array_equal(np.float32(c[k]).astype(np.float64), c[k])
    mot = kat["motor"]
    assert any(c["time_const"] > 0 and c["inertia"] > 0 for c in mot)
    assert any(c["min_speed"] > 0 for c in mot) and any(0 in c["dt_us"] for c in mot)
    assert any(x < 0 for c in mot for x in c["cmd"]) and any(x > c["max_speed"] for c in mot for x in c["cmd"])
    assert {c["schedule"] for c in mot} == {"1ms", "4ms", "mixed"}


def test_rotation_math_is_the_reference_bit_for_bit(ora, kat):
    L = ora.lib()
    for c in kat["rotvec"]:
        np.testing.assert_array_equal(_call(L.ora_rot_from_rotvec, c["r"], n_out=4), c["q"], err_msg=str(c["r"]))
    for c in kat["step"]:
        dq = _call(L.ora_rot_from_rotvec, [c["dt"] * w for w in c["ang_vel"]], n_out=4)   # angVel * dt, Quadcopter_T.cpp:142
        np.testing.assert_array_equal(_call(L.ora_rot_mul, c["att"], dq, n_out=4), c["q"], err_msg=str(c))
    for c in kat["mul"]:
        np.testing.assert_array_equal(_call(L.ora_rot_mul, c["a"], c["b"], n_out=4), c["q"])
    for c in kat["rotate"]:
        np.testing.assert_array_equal(_call(L.ora_rotate, c["q"], c["v"], n_out=3), c["fwd"])
        np.testing.assert_array_equal(_call(L.ora_rotate_inv, c["q"], c["v"], n_out=3), c["inv"])
    for c in kat["euler"]:
        out = np.zeros(4)
        L.ora_rot_from_euler_ypr(*c["ypr"], _dp(out))
        np.testing.assert_array_equal(out, c["q"])
    for c in kat["to_euler"]:
        np.testing.assert_array_equal(_call(L.ora_rot_to_euler_ypr, c["q"], n_out=3), c["ypr"])
        np.testing.assert_array_equal(_call(L.ora_rot_matrix, c["q"], n_out=9), c["R"])


def test_imu_mount_matrix_is_the_reference_float_instance(ora, kat):
    """Rotationf::FromEulerYPR(yaw, pitch, roll).Inverse().GetRotationMatrix() (Quadcopter_T.cpp:78-80) in
    ora_params_init's R_imu_inv"""
    for c in kat["imu_mount"]:
        p = ora.params_init(0.1, np.diag([1e-5, 1e-5, 2e-5]), 0.05, [0, 0, 0], 0.0, 1000.0, 1e-8, 1e-10, 0.0, 0.0,
                            [0, 0, 0], imu_ypr=c["ypr"])
        np.testing.assert_array_equal(np.asarray(list(p.R_imu_inv), np.float32), np.float32(c["R"]), err_msg=str(c["ypr"]))


def test_motor_is_the_reference_bit_for_bit(ora, kat):
    for c in kat["motor"]:
        got = motor_run(ora, c)
        for k in ("speed", "thrust", "torque", "ang_mom"):
            np.testing.assert_array_equal(got[k], c[k], err_msg="%s: type %d motor %d %s" % (k, c["type"], c["motor"], c["schedule"]))


def test_fixture_is_what_the_probe_prints_now():
    """staleness: rerun the probe on the fixture's own inputs (needs oracle/_ref/motion_probe, built where the reference
    is present)"""
    if not os.path.exists(PROBE):
        pytest.skip("oracle/_ref/motion_probe not built (the reference sources are not on this machine)")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    fresh = mg.make_motion_kat(PROBE)
    with open(os.path.join(ROOT, "tests", "golden", "motion_kat.json")) as f:
        assert json.load(f) == json.loads(json.dumps(fresh))


def test_probe_recipe_uses_the_declaration_only_eigen():
    """the probe's include path names oracle/eigen_decl and never tests/shim (a working matrix that must not feed a pin),
    and that header defines nothing"""
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        mk = f.read()
    inc = re.search(r"^MOTION_INC\s*:=(.*)$", mk, re.M).group(1)
    recipe = re.search(r"^_ref/motion_probe:.*\n((?:\t.*\n)+)", mk, re.M).group(1)
    assert "$(MOTION_INC)" in recipe and "-Ieigen_decl" in inc.split()
    assert "shim" not in inc and "shim" not in recipe
    assert "_ref/motion_probe" in mk.split("\nref:")[1].split("\n\n")[0]   # built by `make ref`, i.e. by build()
    with open(os.path.join(ROOT, "oracle", "eigen_decl", "Eigen", "Dense")) as f:
        code = [l for l in f if l.strip() and not l.lstrip().startswith(("//", "#pragma"))]
    assert code == ["namespace Eigen { template <typename T, int R, int C> class Matrix; }\n"]
    if os.path.exists(PROBE):   # the product of that recipe, where the reference was present
        out = subprocess.run([PROBE], input=b"R 0x1p-1 0 0\n", capture_output=True, check=True).stdout
        assert json.loads(out)["op"] == "R"
