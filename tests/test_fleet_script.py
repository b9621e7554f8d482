"""The script of tests/test_gpu_fleet.py's host-against-device comparison, flown on the CPU by the checker alone
(`tests/cpp/test_fleet script`: ora_step_batch + ora_logic_tick, the loop of oracle_py.ClosedLoopBatch): it has to reach
every branch of the rates logic -- idle, the first IMU call, the total-thrust cap, both propeller clamps and F <= 0 --
for every type record, with room to spare over the 10 the GPU test requires.  No GPU: no engine is created."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_fleet")
ROOM = 10          # times the GPU test's floor of 10


@pytest.mark.parametrize("dt_us,period", [(1000, 1.0 / 500.0), (2000, 1.0 / 500.0), (500, 0.0005)])
@pytest.mark.parametrize("n,types,names", [(130, "mixed", ["type1", "type2", "type4", "type5", "tilted_mount", "full_inertia"]),
                                           (65, "one5", ["full_inertia"]), (130, "one4", ["tilted_mount"])])
def test_script_reaches_every_branch_of_the_rates_logic(n, types, names, dt_us, period):
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.dirname(EXE), "test_fleet"])
    out = subprocess.run([EXE, "script", str(n), types, str(dt_us), repr(period)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-1000:])
    res = json.loads(out.stdout)
    print(out.stdout.strip())
    assert sorted(res["tallies"]) == sorted(names) and res["steps"] == 200 and res["logic_ticks"] >= 99
    for name, t in res["tallies"].items():
        for b in ("idle", "cap", "lower", "upper"):
            assert t[b] >= 10 * ROOM, (name, b, t)
        assert t["first_imu"] >= 20                      # once per vehicle: 21 or 22 vehicles per record of the mixed fleet
        # F <= 0 needs min_thrust <= 0: types 1, 2, 4 and the full-inertia record (type 2's mixer); type 5's lower clamp is 0.03 N
        assert t["f_le0_reachable"] == (0 if name in ("type5", "tilted_mount") else 1)
        assert t["f_le0"] >= 10 * ROOM if t["f_le0_reachable"] else t["f_le0"] == 0, (name, t)
