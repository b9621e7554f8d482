"""The type constants, pinned to the reference's own header.

tests/golden/vehicle_constants.json is what Onboard::QuadcopterConstants(t), t = 0..5, holds after its constructor
(Components/Components/Logic/QuadcopterConstants.hpp compiled in place by oracle/_ref/constants_probe) and what
GetVehicleTypeFromID answers for ids 0..31.  The engine's table (csrc/afe_params.cpp) and the checker's (oracle/
agrifly_oracle.c, agrifly_oracle_logic.c) restate that header independently; here both are held against the recording,
BIT FOR BIT, through the widening the simulator's main does (Simulator/Rappids_Simulator/main.cpp:152-164, 203-209:
float members to double, propTorqueFromSpeedSqr a float product, inertia_yy = inertia_xx) and through
QuadcopterLogic::Initialise / QuadcopterMixer::SetParameters (QuadcopterLogic.cpp:111-150, QuadcopterMixer.hpp:36-52).
No GPU."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

F = np.float32
TYPES = (1, 2, 4, 5)


@pytest.fixture(scope="module")
def consts(golden_dir):
    fx = json.load(open(os.path.join(golden_dir, "vehicle_constants.json")))

    def member(t, name):
        return np.array(fx["types"][str(t)]["bits"][name], np.uint32).view(F)[()]
    fx["f"] = member
    return fx


def _bits32(v):
    return int(np.asarray(v, F).view(np.uint32))


def _bits64(v):
    return int(np.asarray(v, np.float64).view(np.uint64))


def _same64(got, want, what):
    """a double of the engine / checker against a double built from the recording: the same 64 bits"""
    assert _bits64(got) == _bits64(want), "%s: got %r (%#x), the reference's header gives %r (%#x)" % (what, got, _bits64(got), want, _bits64(want))


def _same32(got, want, what):
    assert _bits32(got) == _bits32(want), "%s: got %r (%#x), the reference's header gives %r (%#x)" % (what, got, _bits32(got), want, _bits32(want))


def _widened(consts, t):
    """main.cpp:152-164, 203-209 applied to the recording: name -> (double, the line it follows)"""
    f = lambda name: consts["f"](t, name)   # noqa: E731
    ixx, izz = np.float64(f("inertia_xx")), np.float64(f("inertia_zz"))
    return dict(
        mass=(np.float64(f("mass")), "main.cpp:152"),
        inertia=([ixx, 0, 0, 0, ixx, 0, 0, 0, izz], "main.cpp:153-155 (inertia_yy = inertia_xx, :154), 203-204"),
        arm_length=(np.float64(f("armLength")), "main.cpp:156"),
        prop_thrust_from_speed_sqr=(np.float64(f("propellerThrustFromSpeedSqr")), "main.cpp:157"),
        # a float times a float, rounded to float, THEN widened
        prop_torque_from_speed_sqr=(np.float64(F(f("propellerTorqueFromThrust") * f("propellerThrustFromSpeedSqr"))), "main.cpp:158-159"),
        motor_time_const=(np.float64(f("motorTimeConst")), "main.cpp:161"),
        motor_inertia=(np.float64(f("motorInertia")), "main.cpp:162"),
        motor_min_speed=(np.float64(f("motorMinSpeed")), "main.cpp:163"),
        motor_max_speed=(np.float64(f("motorMaxSpeed")), "main.cpp:164"),
        lin_drag=([np.float64(f("linDragCoeffB" + a)) for a in "xyz"], "main.cpp:207-209"),
        com_error=([0.0, 0.0, 0.0], "main.cpp:171"))


def test_fixture_covers_every_type_and_says_which_are_valid(consts):
    assert sorted(consts["types"]) == [str(t) for t in range(6)] and len(consts["type_from_id"]) == 32
    assert [consts["types"][str(t)]["ints"]["valid"] for t in range(6)] == [0, 1, 1, 0, 1, 1]
    for t in range(6):   # the header's own identity: inertiaMatrix = diag(xx, xx, zz), QuadcopterConstants.hpp:269-271
        got = [consts["types"][str(t)]["bits"]["inertiaMatrix_%d_%d" % (i, j)] for i in range(3) for j in range(3)]
        xx, zz = (consts["types"][str(t)]["bits"][k] for k in ("inertia_xx", "inertia_zz"))
        assert got == [xx, 0, 0, 0, xx, 0, 0, 0, zz], t
    for t in TYPES:      # every shipped type mounts its IMU straight and spins propeller 0 upwards
        assert [_bits32(consts["f"](t, "IMU_" + a)) for a in ("yaw", "pitch", "roll")] == [0, 0, 0]
        assert consts["types"][str(t)]["ints"]["prop0SpinDir"] == 1


@pytest.mark.parametrize("t", TYPES)
def test_engine_vehicle_params_are_the_headers(afa, consts, t):
    p, w = afa.params_from_type(t), _widened(consts, t)
    for name in ("mass", "arm_length", "prop_thrust_from_speed_sqr", "prop_torque_from_speed_sqr", "motor_time_const",
                 "motor_inertia", "motor_min_speed", "motor_max_speed"):
        _same64(getattr(p, name), w[name][0], "type %d afe_vehicle_params.%s (%s)" % (t, name, w[name][1]))
    for k in range(9):
        _same64(p.inertia[k], w["inertia"][0][k], "type %d afe_vehicle_params.inertia[%d] (%s)" % (t, k, w["inertia"][1]))
    for k in range(3):
        _same64(p.lin_drag_coeff_b[k], w["lin_drag"][0][k], "type %d afe_vehicle_params.lin_drag_coeff_b[%d] (%s)" % (t, k, w["lin_drag"][1]))
        _same64(p.com_error[k], 0.0, "type %d afe_vehicle_params.com_error[%d] (%s)" % (t, k, w["com_error"][1]))
    for a in ("yaw", "pitch", "roll"):   # Quadcopter_T.cpp:75-77
        _same32(getattr(p, "imu_" + a), consts["f"](t, "IMU_" + a), "type %d afe_vehicle_params.imu_%s (Quadcopter_T.cpp:75-77)" % (t, a))


@pytest.mark.parametrize("t", TYPES)
def test_engine_logic_params_are_the_headers(afa, consts, t):
    """QuadcopterLogic::Initialise's reads (QuadcopterLogic.cpp:111-150).  Type 4 leaves maxCmdTotalThrust at -1 (the
    constructor's default, QuadcopterConstants.hpp:48: "computed in the mixer"), and the engine's record must carry that
    -1, not a number of its own."""
    g, f = afa.rates_logic_params_from_type(t), lambda name: consts["f"](t, name)   # noqa: E731
    _same32(g.mass, f("mass"), "mass (QuadcopterLogic.cpp:111)")
    for k in range(9):
        _same32(g.inertia[k], f("inertiaMatrix_%d_%d" % (k // 3, k % 3)), "inertia[%d] (QuadcopterLogic.cpp:142-144)" % k)
    _same32(g.ang_vel_time_const_xy, f("angVelControl_timeConst_xy"), "angVelControl_timeConst_xy (QuadcopterLogic.cpp:142)")
    _same32(g.ang_vel_time_const_z, f("angVelControl_timeConst_z"), "angVelControl_timeConst_z (QuadcopterLogic.cpp:143)")
    _same32(g.arm_length, f("armLength"), "armLength (QuadcopterLogic.cpp:122)")
    _same32(g.prop_thrust_from_speed_sqr, f("propellerThrustFromSpeedSqr"), "propellerThrustFromSpeedSqr (QuadcopterLogic.cpp:123)")
    _same32(g.prop_torque_from_thrust, f("propellerTorqueFromThrust"), "propellerTorqueFromThrust (QuadcopterLogic.cpp:124)")
    assert g.prop0_spin_dir == consts["types"][str(t)]["ints"]["prop0SpinDir"]          # :125
    _same32(g.max_thrust_per_propeller, f("maxThrustPerPropeller"), "maxThrustPerPropeller (QuadcopterLogic.cpp:147)")
    _same32(g.min_thrust_per_propeller, f("minThrustPerPropeller"), "minThrustPerPropeller (QuadcopterLogic.cpp:148)")
    _same32(g.max_cmd_total_thrust, f("maxCmdTotalThrust"), "maxCmdTotalThrust (QuadcopterLogic.cpp:148)")
    if t == 4:
        assert g.max_cmd_total_thrust == -1.0 and f("maxCmdTotalThrust") == F(-1)       # the mixer-default case
    else:
        assert g.max_cmd_total_thrust > 0
    for a in ("yaw", "pitch", "roll"):
        _same32(getattr(g, "imu_" + a), f("IMU_" + a), "imu_%s (QuadcopterLogic.cpp:113-115)" % a)
    _same32(g.gyro_lowpass_cutoff, F(200.0), "gyro cutoff (QuadcopterLogic.cpp:103)")


@pytest.mark.parametrize("t", TYPES)
def test_checker_vehicle_params_are_the_headers(ora, consts, t):
    p, w = ora.params_from_type(t), _widened(consts, t)
    for mine, theirs in (("mass", "mass"), ("k_thrust", "prop_thrust_from_speed_sqr"), ("k_torque", "prop_torque_from_speed_sqr"),
                         ("motor_time_const", "motor_time_const"), ("motor_inertia", "motor_inertia"),
                         ("motor_min_speed", "motor_min_speed"), ("motor_max_speed", "motor_max_speed")):
        _same64(getattr(p, mine), w[theirs][0], "type %d ora_params.%s (%s)" % (t, mine, w[theirs][1]))
    for k in range(9):
        _same64(p.inertia[k], w["inertia"][0][k], "type %d ora_params.inertia[%d] (%s)" % (t, k, w["inertia"][1]))
    for k in range(3):
        _same64(p.lin_drag[k], w["lin_drag"][0][k], "type %d ora_params.lin_drag[%d] (%s)" % (t, k, w["lin_drag"][1]))
    # the arm length has no field of its own there: it is in the motor positions, armLength / sqrt(2) * (+-1, +-1, 0) +
    # centreOfMassError in double (Quadcopter_T.cpp:45-65; FR, RR, RL, FL)
    a = w["arm_length"][0] / np.sqrt(np.float64(2))
    for m, (sx, sy) in enumerate(((+1, -1), (-1, -1), (-1, +1), (+1, +1))):
        for k, want in enumerate((a * sx + 0.0, a * sy + 0.0, a * 0.0 + 0.0)):
            _same64(p.motor_pos[m][k], want, "type %d ora_params.motor_pos[%d][%d] (main.cpp:156, Quadcopter_T.cpp:45-65)" % (t, m, k))
    # zero mount angles: the inverse mount matrix is the identity, Quadcopter_T.cpp:75-80
    assert [float(x) for x in p.R_imu_inv] == [1, 0, 0, 0, 1, 0, 0, 0, 1]   # (a -0.0 off the diagonal is no rotation either)


@pytest.mark.parametrize("t", TYPES)
def test_checker_logic_params_are_the_headers(ora, consts, t):
    """ora_logic_params holds what QuadcopterMixer::SetParameters makes of the header's members (QuadcopterMixer.hpp:
    41-51), in float: _d = armLength / sqrtf(2.0f), _kt = prop0SpinDir * propellerTorqueFromThrust, and the default
    4 * maxThrustPerPropeller * 0.8f where maxCmdTotalThrust < 0 (type 4)."""
    period = F(1.0 / 500.0)
    g, f = ora.logic_params_from_type(t, period), lambda name: consts["f"](t, name)   # noqa: E731
    _same32(g.mass, f("mass"), "mass (QuadcopterLogic.cpp:111)")
    for k in range(9):
        _same32(g.inertia[k], f("inertiaMatrix_%d_%d" % (k // 3, k % 3)), "inertia[%d] (QuadcopterLogic.cpp:142-144)" % k)
    _same32(g.tc_xy, f("angVelControl_timeConst_xy"), "tc_xy (QuadcopterLogic.cpp:142)")
    _same32(g.tc_z, f("angVelControl_timeConst_z"), "tc_z (QuadcopterLogic.cpp:143)")
    _same32(g.d, f("armLength") / np.sqrt(F(2.0)), "d (QuadcopterMixer.hpp:41)")
    _same32(g.kt, F(consts["types"][str(t)]["ints"]["prop0SpinDir"]) * f("propellerTorqueFromThrust"), "kt (QuadcopterMixer.hpp:42)")
    _same32(g.kf, f("propellerThrustFromSpeedSqr"), "kf (QuadcopterMixer.hpp:43)")
    _same32(g.max_thrust, f("maxThrustPerPropeller"), "max_thrust (QuadcopterMixer.hpp:44)")
    _same32(g.min_thrust, f("minThrustPerPropeller"), "min_thrust (QuadcopterMixer.hpp:45)")
    given = f("maxCmdTotalThrust")
    want = F(F(F(4) * f("maxThrustPerPropeller")) * F(0.8)) if given < 0 else given
    assert (given < 0) == (t == 4)
    _same32(g.max_cmd_total_thrust, want, "max_cmd_total_thrust (QuadcopterMixer.hpp:46-51)")
    assert [float(x) for x in g.R] == [1, 0, 0, 0, 1, 0, 0, 0, 1]                        # QuadcopterLogic.cpp:113-117
    _same32(g.onboard_period, period, "onboard_period")
    _same32(g.gyro_cutoff, F(200.0), "gyro cutoff (QuadcopterLogic.cpp:103)")


def test_type_from_id_is_the_headers(afa, ora, consts):
    want = consts["type_from_id"]
    assert [afa.type_from_id(i) for i in range(32)] == want                              # QuadcopterConstants.hpp:297-332
    assert [ora.lib().ora_type_from_id(i) for i in range(32)] == want
    assert set(want) == {0, 1, 2, 4, 5}


@pytest.mark.parametrize("t", (0, 3))
def test_types_the_header_calls_invalid_are_refused(afa, ora, consts, t):
    assert consts["types"][str(t)]["ints"]["valid"] == 0
    with pytest.raises(afa.AfeError) as ei:
        afa.params_from_type(t)
    assert ei.value.status == 1
    with pytest.raises(afa.AfeError) as ei:
        afa.rates_logic_params_from_type(t)
    assert ei.value.status == 1
    with pytest.raises(ValueError):
        ora.params_from_type(t)
    with pytest.raises(ValueError):
        ora.logic_params_from_type(t, 0.002)


def test_low_battery_threshold_is_the_headers(afa, consts):
    """afe_low_battery_threshold_from_type answers for EVERY type of the enum, the refused ones included (the reference's
    constructor reads the member whatever `valid` says, Quadcopter_T.cpp:71-72)"""
    L = afa.library()
    for t in range(6):
        _same32(afa.low_battery_threshold_from_type(t), consts["f"](t, "lowBatteryThreshold"), "type %d lowBatteryThreshold" % t)
    assert [float(afa.low_battery_threshold_from_type(t)) for t in range(6)] == [0.0, 3.0, 3.0, 3.0, 9.0, 6.0]
    v = C.c_float(-7.0)
    for t in (-1, 6, 255, 2 ** 31 - 1, -2 ** 31):
        assert L.afe_low_battery_threshold_from_type(t, C.byref(v)) == 1 and v.value == -7.0, t   # AFE_ERR_INVALID_ARG, output untouched
    for t in range(6):
        assert L.afe_low_battery_threshold_from_type(t, None) == 1


def test_fixture_is_what_the_probe_writes_now(golden_dir):
    """staleness (needs oracle/_ref/constants_probe, built where the reference is present): byte for byte"""
    spec = importlib.util.spec_from_file_location("make_vehicle_constants", os.path.join(golden_dir, "make_vehicle_constants.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if not os.path.exists(mod.PROBE):
        pytest.skip("oracle/_ref/constants_probe not built (the reference sources are not on this machine)")
    with open(mod.FIXTURE) as f:
        assert f.read() == mod.dumps(mod.make_vehicle_constants())
