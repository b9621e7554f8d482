"""The step kernels (afe_kernels.hip) against what the REFERENCE's own Quadcopter_T::Run computed: tests/golden/
rigid_body_reference.npz, recorded by oracle/_ref/rigid_body_probe from Quadcopter_T.cpp and Motor.cpp compiled in place
(tests/golden/make_rigid_body_reference.py; tests/test_rigid_body_reference.py holds the CPU checker to the same file bit
for bit, which is why the tolerances here are the project's existing engine-against-checker ones).  96 vehicles in five
(dt, logic period) groups: lagged rotors, rotor inertia, CoM error, drag, world-frame wrench, full inertia tensors, commands
outside the rotor's range that change at ticks, every kind of ground contact, both sides of the small-angle branch, dt 0.
Reads the committed fixture only.  The engine inverts the inertia tensor itself (afe_params.cpp invert3; the ABI has no
getter for the nine numbers): the fp64 comparison after ONE step at 1e-12 is what holds them to the recorded run.
Needs an MI355X."""
import importlib.util
import os

import numpy as np
import pytest

from tests.scenarios import FLOORS, afa, record_parity, rel_err, rel_err_vec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_GROUPS = 5
STATE = ("pos", "vel", "att", "ang_vel", "motor_speed")


@pytest.fixture(scope="module")
def ref():
    spec = importlib.util.spec_from_file_location("make_rigid_body_reference", os.path.join(ROOT, "tests", "golden", "make_rigid_body_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fx = mod.load_fixture()
    assert len(fx["group_dt_us"]) == N_GROUPS and fx["fp32_ok"].all()
    return mod, fx


_SEEN = {}


def _ledger(test, precision, field, got, want):
    """one ledger entry per kernel path, horizon and motor model: the worst vehicle over every group and checkpoint seen so far"""
    a, b = _SEEN.setdefault((test, precision, field), ([], []))
    a.append(np.asarray(got, np.float64))
    b.append(np.asarray(want, np.float64))
    record_parity(test, precision, field, np.concatenate(a, axis=1), np.concatenate(b, axis=1))


def _params(fx, i):
    p = afa.params_from_type(int(fx["type_id"][i]))
    assert (p.imu_yaw, p.imu_pitch, p.imu_roll) == (0, 0, 0)       # every shipped type: the IMU mount stays outside the pin
    p.mass, p.arm_length = float(fx["in_mass"][i]), float(fx["in_arm"][i])
    for k in range(9):
        p.inertia[k] = float(fx["in_inertia"][i, k])
    for k in range(3):
        p.com_error[k], p.lin_drag_coeff_b[k] = float(fx["in_com"][i, k]), float(fx["in_drag"][i, k])
    p.motor_min_speed, p.motor_max_speed = float(fx["in_min_speed"][i]), float(fx["in_max_speed"][i])
    p.prop_thrust_from_speed_sqr, p.prop_torque_from_speed_sqr = float(fx["in_k_thrust"][i]), float(fx["in_k_torque"][i])
    p.motor_time_const, p.motor_inertia = float(fx["in_tau"][i]), float(fx["in_J"][i])
    return p


def _run(mod, fx, gi, cases, table, types, precision, what):
    """vehicle j flies case cases[j] on record types[j]; compared with the recorded values at every checkpoint"""
    n = len(cases)
    dt_us = int(fx["group_dt_us"][gi])
    lagged = ((fx["in_tau"] > 0) | (fx["in_J"] > 0))[cases]
    with afa.Ensemble(n, precision=precision) as e:
        e.set_type_table(table)
        e.set_vehicle_types(types)
        e.set_logic_period(float(fx["group_period"][gi]))
        e.set_imu_noise(True, float(fx["sigma_gyro"]), float(fx["sigma_acc"]), afa.AFE_SEED_REFERENCE)
        e.set_state(fx["in_pos"][cases].T, fx["in_vel"][cases].T, fx["in_att"][cases].T, fx["in_ang_vel"][cases].T, np.zeros((4, n)))
        e.set_external_force(fx["in_ext_force"][cases].T)
        e.set_external_torque(fx["in_ext_torque"][cases].T)
        n_checked = 0
        for a, b, held, c in mod.segments(fx, gi):
            e.set_motor_cmds(fx["cmd_sets"][cases, held].T)
            e.step(dt_us, b - a)
            if c < 0:
                continue
            st = e.get_state()
            gyro, acc = e.get_imu()
            ticks = fx["ref_ticks"][cases, c]
            assert e.logic_ticks == int(ticks[0]) and np.all(ticks == ticks[0]), (what, b)
            assert e.time_us == dt_us * b
            got = dict(st)
            if ticks[0] > 0:          # before the first tick the reference has handed its logic no sample
                got.update(gyro=gyro, acc=acc)
            # fp64: 1e-12 after one step, 1e-11 over the rollout; fp32: 1e-5 with the reference's motor model (tau = J = 0),
            # 5e-5 with a lagged rotor (the speed itself is fp32 state, tests/campaigns/step_campaign.py)
            subsets = [("", np.ones(n, bool), 1e-12 if b == 1 else 1e-11)] if precision == afa.AFE_F64 else \
                      [(", reference motor", ~lagged, 1e-5), (", lagged rotor", lagged, 5e-5)]
            for tag, m, tol in subsets:
                if not m.any():
                    continue
                for k, v in got.items():
                    want = fx["ref_" + k][cases[m], c].T
                    err = rel_err_vec(v[:, m], want, FLOORS[k])
                    _ledger("reference rigid body, %s kernel, %s%s" % (what.split()[2], "one step" if b == 1 else "rollout", tag), precision, k, v[:, m], want)
                    t = max(tol, 1e-6) if k in ("gyro", "acc") else tol       # tests/test_gpu_parity.py _cmp_state
                    print("%s after step %3d%s %-11s %.3g (bound %.0e)" % (what, b, tag, k, err, t))
                    assert err <= t, "%s after step %d%s, %s: rel err %.3g > %.1g (floor %g)" % (what, b, tag, k, err, t, FLOORS[k])
            n_checked += 1
        assert n_checked == 4


@pytest.mark.parametrize("precision", [afa.AFE_F64, afa.AFE_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("gi", range(N_GROUPS))
def test_type_table_kernel_flies_the_recorded_cases(ref, gi, precision):
    """one Ensemble per (dt, period) group, one type-table record per case, the vehicles in shuffled order so that records
    mix within a wave; group 0 holds 68 vehicles, a ragged second wave"""
    mod, fx = ref
    idx = mod.group_cases(fx, gi)
    perm = np.random.Generator(np.random.PCG64(7 + gi)).permutation(len(idx))
    _run(mod, fx, gi, idx[perm], [_params(fx, i) for i in idx], perm.astype(np.uint8), precision, "group %d table" % gi)


@pytest.mark.parametrize("precision", [afa.AFE_F64, afa.AFE_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("gi", range(N_GROUPS))
def test_uniform_kernel_flies_the_recorded_cases(ref, gi, precision):
    """the single-record path: one vehicle flying the group's first case, and 65 flying its last (under the reference's
    seeding every vehicle draws the same noise, so all 65 must land on the one recording)"""
    mod, fx = ref
    idx = mod.group_cases(fx, gi)
    for n, i in ((1, idx[0]), (65, idx[-1])):
        _run(mod, fx, gi, np.full(n, i), [_params(fx, i)], np.zeros(n, np.uint8), precision, "group %d uniform n=%d" % (gi, n))


@pytest.mark.parametrize("precision,tol", [(afa.AFE_F64, 1e-9), (afa.AFE_F32, 1e-5)], ids=["f64", "f32"])
def test_on_device_rates_logic_flies_the_recorded_closed_loop(ref, precision, tol):
    """tests/golden/rigid_body_closed_loop.npz: the reference's rigid body with the reference's own low-pass, rate controller
    and mixer headers in the loop (12 vehicles, four types, 150 steps, rates commands that change twice and saturate).  The
    engine with set_rates_logic against the RECORDED values at every checkpoint, at tests/test_gpu_logic.py's tolerances:
    1e-9 (fp64) and 1e-5 (fp32) on the state, the float motor commands never below 1e-6."""
    mod, _ = ref
    fx = mod.load_fixture(mod.CL_FIXTURE)
    n, dt_us = len(fx["type_id"]), int(fx["dt_us"])
    ids = sorted(set(int(t) for t in fx["type_id"]))
    table = [afa.params_from_type(t) for t in ids]
    for i in range(n):                  # the recorded body is the shipped type's, field for field
        p = table[ids.index(int(fx["type_id"][i]))]
        assert (p.mass, list(p.inertia), p.arm_length, p.motor_max_speed) == (fx["in_mass"][i], list(fx["in_inertia"][i]), fx["in_arm"][i], fx["in_max_speed"][i])
    with afa.Ensemble(n, precision=precision) as e:
        e.set_type_table(table)
        e.set_vehicle_types(np.array([ids.index(int(t)) for t in fx["type_id"]], np.uint8))
        e.set_logic_period(float(fx["period"]))
        e.set_imu_noise(True, float(fx["sigma_gyro"]), float(fx["sigma_acc"]), afa.AFE_SEED_REFERENCE)
        e.set_state(fx["in_pos"].T, fx["in_vel"].T, fx["in_att"].T, fx["in_ang_vel"].T, np.zeros((4, n)))
        e.set_motor_cmds(np.zeros((4, n), np.float32))
        e.set_external_force(fx["in_ext_force"].T)
        e.set_rates_logic([afa.rates_logic_params_from_type(t) for t in ids])
        for a, b, row, c in mod.closed_loop_segments(fx):
            if row >= 0:
                e.set_rates_commands(fx["rows"][:, row, 1], fx["rows"][:, row, 2:5].T)
            e.step(dt_us, b - a)
            if c < 0:
                continue
            st, cmds = e.get_state(), e.get_motor_cmds()
            assert e.logic_ticks == int(fx["ref_ticks"][0, c])
            for k in STATE:
                err = rel_err_vec(st[k], fx["ref_" + k][:, c].T, FLOORS[k])
                _ledger("reference closed loop with the on-device rates logic", precision, k, st[k], fx["ref_" + k][:, c].T)
                print("closed loop after step %3d %-11s %.3g (bound %.0e)" % (b, k, err, tol))
                assert err <= tol, "closed loop after step %d, %s: rel err %.3g > %.1g" % (b, k, err, tol)
            err = rel_err(cmds, fx["ref_cmd"][:, c].T, 1.0)
            print("closed loop after step %3d motor_cmd   %.3g (bound %.0e)" % (b, err, max(tol, 1e-6)))
            assert err <= max(tol, 1e-6), (b, err)
