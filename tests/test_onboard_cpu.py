"""The onboard flight computer's definition on the CPU: the two restatements (tests/onboard_reference.py scalar and line by line,
tests/onboard_checker.py numpy) against each other, the script's branch coverage, the parts that have pins, the discrete fields
under two math libraries, and the physical sense of the attitude estimate on a flight of the CPU oracle.  No GPU."""
import ctypes as C
import importlib

import numpy as np
import pytest

from tests import gps_imu_reference as gref
from tests import onboard_checker as oc
from tests import onboard_flight as of

afa = importlib.import_module("agri-fly_amd")
F = np.float32

# measured on tests/onboard_truth_flight.py fly_oracle("rates") (0.6 s, tilts up to 0.413 rad, IMU noise on): the worst
# |estimated tilt - true tilt|; recorded in DESIGN.md section 4m.  The GPU truth flight is held to twice this.
TRUTH_TILT_ERR = 0.06992            # measured: 0.0699101 (true tilts up to 0.413 rad)


@pytest.fixture(scope="module")
def rec():
    return of.synthetic_record(afa)


@pytest.fixture(scope="module")
def glibc_run(rec):
    return of.replay(afa, rec, oc.glibc_math)


def test_the_two_restatements_agree_bit_for_bit(rec, glibc_run):
    """every field and command of every vehicle after every tick of the script (1 200 ticks, 130 vehicles)"""
    fields, cmds, _, _, _ = glibc_run
    rows = of.replay_scalar(afa, rec, oc.glibc_math)
    assert len(rows) == len(fields) == of.TICKS
    for k, row in enumerate(rows):
        assert len(row) == of.N
        for i, r in row.items():
            for name, v in r.items():
                w = cmds[k][:, i] if name == "motor_cmd" else fields[k][name][..., i]
                assert oc.same_bits(np.asarray(v, np.asarray(w).dtype), np.asarray(w)), (k + 1, i, name, v, w)


def test_the_script_takes_every_live_branch(glibc_run):
    count = glibc_run[4].count
    assert set(count) == set(oc.BRANCHES)
    for name, live in oc.BRANCHES.items():
        assert (count[name] > 0) == live, (name, count[name])


def test_the_script_ends_where_it_says(rec, glibc_run):
    """each group's story: state, first panic reason, and who is left alone"""
    fields = glibc_run[0]
    g, last = of.groups(of.N), glibc_run[0][-1]
    want = dict(turn=(oc.PANIC, oc.UPSIDE_DOWN), turn_suppressed=(oc.RATES, 0), silent=(oc.PANIC, oc.RADIO_TIMEOUT), flat=(oc.PANIC, oc.LOW_BATTERY),
                kill=(oc.KILLED, oc.KILLED_EXTERNALLY), idle=(oc.IDLE, 0), acc_hover=(oc.ACCELERATION, 0), acc_general=(oc.ACCELERATION, 0),
                acc_cut=(oc.ACCELERATION, 0), both_turned=(oc.PANIC, oc.RADIO_TIMEOUT), both_flat=(oc.PANIC, oc.LOW_BATTERY), chatty=(oc.RATES, 0),
                long=(oc.RATES, 0), late=(oc.RATES, 0))
    special = np.concatenate([v for v in g.values()])
    for name, (state, reason) in want.items():
        assert (last["flight_state"][g[name]] == state).all() and (last["panic_reason"][g[name]] == reason).all(), name
    others = np.setdiff1d(np.arange(of.N), special)
    assert (last["flight_state"][others] == oc.RATES).all() and (last["panic_reason"][others] == 0).all()
    # sticky: once PANIC or KILLED, for good, with the motors off from that tick on
    state = np.stack([f["flight_state"] for f in fields])
    sunk = (state == oc.PANIC) | (state == oc.KILLED)
    assert (sunk[1:] >= sunk[:-1]).all()
    cmds = np.stack(glibc_run[1])
    assert (cmds.transpose(0, 2, 1)[sunk] == 0).all()
    # the silent ones: PANIC at the first tick more than 1.5 s after their last message
    i = int(g["silent"][0])
    t_last = int(last["last_radio_us"][i])
    ticks_T = [tk[1] for tk in rec["ticks"]]
    expect = next(k for k, T in enumerate(ticks_T, 1) if T - t_last > 1500000)
    assert of.first_tick_in_state(fields, i, oc.PANIC) == expect


def test_discrete_fields_are_the_same_under_glibc_and_numpy(rec, glibc_run):
    """state, reason and warnings after every tick, and the counters: what licenses asserting them exactly on the GPU"""
    fields_n, _, counts_n, _, _ = of.replay(afa, rec, oc.numpy_math)
    for k, (a, b) in enumerate(zip(glibc_run[0], fields_n)):
        for name in ("flight_state", "panic_reason", "warnings", "motors_running", "cycle_counter", "last_radio_us"):
            assert np.array_equal(a[name], b[name]), (k + 1, name)
    assert all(np.array_equal(a, b) for a, b in zip(glibc_run[2], counts_n))


# ---- the pinned parts ------------------------------------------------------------------------------------------------------------
def test_lowpass_is_the_oracle_librarys():
    from oracle import oracle_py as ora
    L = ora.logic_lib()
    rng = np.random.default_rng(1)
    for cutoff, init in ((100.0, 0.0), (float(F(0.5) * F(2 * np.pi)), 7.2), (200.0, 0.0)):
        f = ora.OraLpf2()
        L.ora_lpf2_init(C.byref(f), float(F(of.PERIOD)), cutoff, init)
        k = gref.lowpass_coefficients(of.PERIOD, cutoff)
        assert [F(f.a1), F(f.a2), F(f.b0), F(f.b1), F(f.b2)] == list(k)
        state = [np.full(1, init, F) for _ in range(4)]
        for x in rng.normal(5, 3, 200).astype(F):
            want = F(L.ora_lpf2_apply(C.byref(f), float(x)))
            got = oc.lp2_apply(k, state, np.array([x], F))[0]
            assert oc.same_bits(got, want)


def test_rates_command_is_the_oracles_logic_tick(rec, glibc_run):
    """the command of a vehicle in the rates state against ora_logic_tick fed the same samples and commands (type 5 vehicles with
    the untilted mount, which the oracle's type record has)"""
    from oracle import oracle_py as ora
    L = ora.logic_lib()
    lp = ora.logic_params_from_type(5, of.PERIOD)
    plain = [int(i) for i in np.flatnonzero(rec["types"] == 0)[:6]]
    states = {}
    for i in plain:
        states[i] = ora.OraLogicState()
        L.ora_logic_init(C.byref(lp), C.byref(states[i]))
    fields, cmds = glibc_run[0], glibc_run[1]
    checked = 0
    for k, (now, T, after, gyro, acc) in enumerate(rec["ticks"][:120], start=1):
        for event in rec["events"].get(k, []):
            if event[0] == "rates":
                for j in range(len(event[2])):
                    if event[1] + j in states:
                        L.ora_logic_set_rates_cmd(C.byref(states[event[1] + j]), float(event[2][j]), (C.c_float * 3)(*[float(x) for x in event[3][:, j]]))
        for i, s in states.items():
            L.ora_logic_tick(C.byref(lp), C.byref(s), (C.c_float * 3)(*[float(x) for x in gyro[:, i]]))
            if fields[k - 1]["flight_state"][i] == oc.RATES:
                assert oc.same_bits(np.array(list(s.motor_speed_cmd), F), cmds[k - 1][:, i]), (k, i)
                assert oc.same_bits(np.array(list(s.motor_force_cmd), F), fields[k - 1]["motor_forces"][:, i]), (k, i)
                checked += 1
    assert checked > 500


def test_telemetry_bytes_are_the_hosts_encoder(rec, glibc_run):
    """both packets of every vehicle, rebuilt from the checker's fields with afe_telemetry_encode"""
    L = afa.library()
    fields, _, _, telemetry, ck = glibc_run
    assert len(telemetry) == 3
    for (k, first, count), got in telemetry.items():
        f = fields[k - 1]
        for j in range(count):
            i = first + j
            pk = afa.TelemetryPacket()
            raw = np.zeros((2, 30), np.uint8)
            pk.type, pk.packet_number = 0, int(got[j, 0, 1])
            for c in range(3):
                pk.accel[c] = f["acc_filtered"][c, i]
                pk.gyro[c] = f["gyro_filtered"][c, i]
                pk.position[c] = 0.0
            for c in range(4):
                pk.motor_forces[c] = f["motor_forces"][c, i]
            pk.batt_voltage = f["volts"][i]
            assert L.afe_telemetry_encode(C.byref(pk), raw[0].ctypes.data) == 0
            assert np.array_equal(raw[0], got[j, 0]), (k, i)
            pk.type = 1
            q = f["est_att"][:, i]
            for c in range(3):
                pk.velocity[c] = 0.0
                pk.attitude[c] = q[1 + c] if q[0] > 0 else -q[1 + c]
            for c in range(6):
                pk.debug_vals[c] = 0.0
            pk.debug_vals[0] = f["temp_filtered"][i]
            pk.panic_reason, pk.warnings = int(got[j, 1, 26]), int(got[j, 1, 28])
            assert L.afe_telemetry_encode(C.byref(pk), raw[1].ctypes.data) == 0
            assert np.array_equal(raw[1], got[j, 1]), (k, i)
    # the counter and the warnings: advanced and cleared in the range alone (63..65 at tick 200, everyone at 400 and at the end)
    assert (ck.packet[63:66] == 3).all() and (np.delete(ck.packet, [63, 64, 65]) == 2).all()
    assert (ck.warnings == 0).all()


def test_the_attitude_controller_is_the_pinned_one():
    """nothing restated: tests/onboard_checker.py calls tests/stages_checker.desired_angular_velocity and the quaternion functions
    of tests/follower_checker.py, which tests/golden/offboard_reference.npz pins"""
    from tests import follower_checker as fc
    from tests import stages_checker as sc
    assert oc.q_mul is fc.q_mul and oc.q_matrix is fc.q_matrix and oc.m_rotate is fc.m_rotate and oc.sc.desired_angular_velocity is sc.desired_angular_velocity


def test_guard_and_codec_edges():
    m = oc.glibc_math
    got = oc.guarded_acos(np.array([1.0, -1.0, 1.0000001, -1.0000001, 2.0, -2.0, np.nan], F), m)
    assert got[0] == 0 and got[1] == oc.PI_F and got[2] == 0 and got[3] == oc.PI_F and got[4] == 0 and got[5] == oc.PI_F and np.isnan(got[6])
    assert oc.telemetry_code(np.array([np.nan, 31.0, -31.0, 0.0, 30.0, -30.0], F), -30, 30).tolist() == [0, 0, 0, 32768, 65535, 1]


def test_estimated_tilt_follows_the_oracles_true_tilt():
    """0.6 s of the CPU oracle under swinging rates commands with IMU noise, tests/onboard_checker.py as the firmware: the worst
    distance of the estimated tilt from the true tilt is what was measured and written down, and the vehicles do tilt"""
    from oracle import oracle_py as ora
    from tests import onboard_truth_flight as tf
    out = tf.fly_oracle(ora, afa, "rates")
    print("tilt_err", out["tilt_err"], "tilt_max", out["tilt_max"])
    assert (out["states"] == oc.RATES).all()
    assert out["tilt_max"] > 0.1
    assert out["tilt_err"] <= TRUTH_TILT_ERR
