"""agrifly::Fleet<logicType> with more than one vehicle, and the on-device rates logic judged on every vehicle.

tests/cpp/test_fleet.cpp does the flying and the comparing and prints one JSON object per case; this file runs it once
per case, each child under a time limit, and asserts.  Needs an MI355X.

  record   C1: 130 vehicles of the four shipped types, shuffled, decorrelated IMU noise, a recording logicType: the call
           order of Quadcopter_T.cpp:163-189, battery 1.2f x threshold(type of i) and current -1, temperature 25, the IMU
           sample bit for bit what afe_get_imu returns, commands unique to (vehicle, motor, tick) in vehicle i's slots,
           acting from the next step (rotor speeds of the zero-time-constant types), per-index accessors at 0, 63, 64, 129.
  single   C1: the single-vehicle Quadcopter_T through the reference's own fifteen-argument call is handed 1.2f x 3, 3, 9
           and 6 V for types 1, 2, 4 and 5; an explicit trailing threshold (0 included) wins.
  equal    C2: engine A is Fleet<OraLogic> -- the checker's ora_logic_tick as a host logicType, handed the engine's own IMU
           sample by the Fleet -- and engine B runs the device logic (afe_set_rates_logic) on the identical float sample, so
           motor commands, position, velocity, attitude, body rate, rotor speeds and the IMU sample of A and B are equal
           BIT FOR BIT after every step for every vehicle, no mask.  Six type records (types 1, 2, 4, 5, a tilted IMU
           mount, a full inertia tensor with a rotor lag); idle ticks, a command for all, one for [17, 101), thrust beyond
           the cap with rate steps into both propeller clamps and F <= 0; one vehicle's body rate set to NaN mid-run on
           both engines -- that vehicle alone is compared value-wise (NaN equal to NaN, non-finite in the same slots).
           The host logic tallies its branches per type; every reachable one is taken at least 10 times (the script
           flown on the CPU reaches them hundreds of times: tests/test_fleet_script.py).
  arena    C3: N = 16 384 (host-visible arena) and 16 385 (device arena), one type, three logic ticks, A against B."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_fleet")
CLOCKS = [(1000, 1.0 / 500.0), (2000, 1.0 / 500.0), (500, 0.0005)]   # the second: the strict > of the gate
BRANCHES = ("idle", "first_imu", "cap", "lower", "upper")


def run_case(*args, timeout=120):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.dirname(EXE), "test_fleet"])
    out = subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    res = json.loads(out.stdout)
    print(json.dumps({k: v for k, v in res.items() if k != "first_mismatch"}))
    return res


def assert_no_mismatch(res):
    assert res["total_mismatches"] == 0 and all(v == 0 for v in res["mismatches"].values()), \
        "%s\nfirst: %s" % (res["mismatches"], res["first_mismatch"])


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_fleet_hands_every_vehicle_its_own_sample_battery_and_slots(precision):
    res = run_case("record", precision)
    assert res["vehicles"] == 130 and res["ticks"] >= 5 and res["steps"] > res["ticks"]
    assert set(res["mismatches"]) >= {"call_order", "battery", "current", "temperature", "gyro", "acc", "cmd_slots", "rotor_speed",
                                      "noise_distinct", "accessor_get", "accessor_neighbour", "type_mix"}
    assert_no_mismatch(res)


def test_the_references_fifteen_argument_call_hands_the_logic_the_types_battery_voltage():
    res = run_case("single")
    assert_no_mismatch(res)
    import numpy as np
    f = np.float32
    want = {"1": f(1.2) * f(3), "2": f(1.2) * f(3), "4": f(1.2) * f(9), "5": f(1.2) * f(6)}     # float products
    assert {k: f(v) for k, v in res["handed_volts"].items()} == want
    assert f(res["override_5V"]) == f(1.2) * f(5) and res["override_0V"] == 0.0


def assert_equal_case(res, n, nanv):
    assert res["vehicles"] == n and res["steps"] == 200 and res["nonfinite_vehicle"] == nanv
    assert set(res["mismatches"]) == {"motor_cmds", "pos", "vel", "att", "ang_vel", "rotor_speed", "gyro", "acc", "logic_ticks"}
    assert_no_mismatch(res)
    # the run did something: in the linear range every vehicle's commands are non-zero and differ from its neighbour's, and
    # the NaN vehicle really was non-finite
    assert res["vehicles_with_nonzero_cmd"] == n and res["neighbours_with_distinct_cmd"] == n - 1
    assert res["nonfinite_slots_seen"] > 100
    for name, t in res["tallies"].items():
        for b in BRANCHES:
            assert t[b] >= 10, (name, b, t)
        if t["f_le0_reachable"]:
            assert t["f_le0"] >= 10, (name, t)
        else:
            assert t["f_le0"] == 0, (name, t)      # min_thrust > 0: the lower clamp keeps F above 0


@pytest.mark.parametrize("dt_us,period", CLOCKS)
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_device_logic_equals_host_logic_on_every_vehicle_mixed_types(precision, dt_us, period):
    res = run_case("equal", precision, 130, "mixed", "default", dt_us, repr(period))
    assert sorted(res["tallies"]) == sorted(["type1", "type2", "type4", "type5", "tilted_mount", "full_inertia"])
    assert res["record_path"] == 2                      # types mixed within a run of 64: the LDS-staged table
    assert_equal_case(res, 130, 77)


@pytest.mark.parametrize("dt_us,period", CLOCKS)
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_device_logic_equals_host_logic_one_type_in_kernel_arguments(precision, dt_us, period):
    """65 vehicles on one record: the parameters travel as kernel arguments (scalar registers).  The record is the full
    inertia tensor with the rotor lag."""
    res = run_case("equal", precision, 65, "one5", "default", dt_us, repr(period))
    assert res["record_path"] == 0 and list(res["tallies"]) == ["full_inertia"]
    assert_equal_case(res, 65, 40)


@pytest.mark.parametrize("dt_us,period", CLOCKS)
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_device_logic_equals_host_logic_with_the_device_engine_persistent(precision, dt_us, period):
    """B in AFE_STEP_PERSISTENT.  130 vehicles on one record (the tilted mount) so that the ensemble qualifies for the
    resident grid; how many of B's steps a resident grid served is printed, not asserted (the engine may decline)."""
    res = run_case("equal", precision, 130, "one4", "persistent", dt_us, repr(period))
    assert list(res["tallies"]) == ["tilted_mount"]
    assert_equal_case(res, 130, 77)


@pytest.mark.parametrize("n", [16384, 16385])
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_host_and_device_logic_agree_either_side_of_the_arena_switch(precision, n):
    """the Fleet keeps up to 16 384 vehicles in a host-visible arena and more in a device arena; vehicles 0, 16 383 and
    16 384 are named in the failure message when one of them is the first to differ"""
    res = run_case("arena", precision, n)
    assert res["vehicles"] == n and res["logic_ticks"] == 3
    assert_no_mismatch(res)
    assert res["vehicles_with_nonzero_cmd"] == n and res["neighbours_with_distinct_cmd"] == n - 1
