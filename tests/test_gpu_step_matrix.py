"""Every compiled step kernel, flown once on purpose and judged against the double-precision oracle of the same
configuration (tests/step_matrix.py states the matrix; tests/test_step_matrix_cpu.py shows it to be the code object's).

One item per (family, precision); inside it every cell of the family is flown on two type tables -- the shipped types
(stateless motors, identity mount) and a modified table (lagged rotors with inertia, full inertia tensors, tilted IMU
mounts, CoM error, drag): motor_stateless is a run-time, wave-uniform branch inside every variant -- at the smallest
shapes at which these kernels can go wrong (step_matrix.N_SMALL, N_XCD, FIRST_GLOBAL).  Every failing cell is collected
before the item asserts, so one report names them all.  Oracle runs are shared between the cells they serve."""
import collections
import importlib
import time

import numpy as np
import pytest

from oracle import oracle_py as ora
from tests import step_matrix as sm
from tests.scenarios import FLOORS, MEASUREMENTS, record_parity, rel_err_vec

afa = importlib.import_module("agri-fly_amd")
pytestmark = pytest.mark.gpu

# ---- tolerances: each from what the project already asserts ------------------------------------------------------------
TOL_F64 = 2e-11              # fp64 state: tests/campaigns/step_campaign.py run_campaign
TOL_F64_LOGIC = 1e-9         # fp64 with logic, state and commands: step_campaign.py run_logic_campaign
TOL_F32 = 1e-5               # fp32 state: run_campaign (the reference's motor model) and run_logic_campaign
TOL_F32_LAGGED = 5e-5        # fp32 state where the table has a lagged rotor: run_campaign -- the rotor speed itself is fp32 state
#                              there, its rounding enters the body torque through differences of four nearly equal thrusts
TOL_FLOAT_SAMPLE = 1e-6      # gyro, acc, motor_cmd are float arithmetic on float-narrowed inputs in every build: never below
#                              max(tol, 1e-6) (run_campaign, run_logic_campaign)
TOL_COUNTER_IMU = {"f32": 1e-5, "f64": 1e-6}     # counter policy, gyro and acc: tests/test_gpu_counter.py (rollout against the checker)
# fp64 + counter + logic, state and commands: no precedent.  A device normal within 1e-13 of the checker's can narrow to a
# neighbouring float, and the float logic carries that ulp into the commands.  Measured on an MI355X over the 42 such cells
# x 2 tables (the parity ledger's step_matrix/... entries): worst 4.27e-13 (ang_vel, args_fused F1T1N2L1B1 on the modified
# table; 2.1e-15 on the shipped types) -- no sample of these flights narrowed to a neighbouring float, every gyro and
# accelerometer sample of the fp64 engine equals the checker's bit for bit.  Asserted at 4 x the measured worst, rounded up
# to one significant digit (the 4 x allows for cells and seeds not sampled); never above the project's fp32 bar.  A float
# ulp in one sample would show as ~1e-7 here: that is then a finding about the device's normals, not a bound to widen.
TOL_F64_COUNTER_LOGIC = 2e-12
assert TOL_F64_COUNTER_LOGIC <= TOL_F32

STATE = ("pos", "vel", "att", "ang_vel", "motor_speed")


def tolerances(c, d):
    if c.precision == "f32":
        state = TOL_F32_LAGGED if d.lagged else TOL_F32
    elif c.logic:
        state = TOL_F64_COUNTER_LOGIC if c.noise == 2 else TOL_F64_LOGIC
    else:
        state = TOL_F64
    sample = max(state, TOL_FLOAT_SAMPLE)
    imu = max(sample, TOL_COUNTER_IMU[c.precision]) if c.noise == 2 else sample
    tol = {k: state for k in STATE}
    tol["gyro"] = tol["acc"] = imu
    if c.logic:
        tol["motor_cmd"] = state if (c.precision == "f64" and c.noise == 2) else sample
    return tol


_data, _oracle = {}, {}


def data_of(c, table):
    k = (table, sm.layout_of(c), sm.n_of(c))
    if k not in _data:
        _data[k] = sm.flight_data(afa, ora, *k)
    return _data[k]


def oracle_of(c, d, rng0):
    """one oracle run per (fext, text, noise, logic, layout, table, shape, where the commands fall), left unchanged"""
    k = sm.oracle_key(c, d)
    if k not in _oracle:
        b = sm.oracle_run(ora, c, d, rng0)
        for a in (b.pos, b.vel, b.att, b.ang_vel, b.motor_speed, b.motor_cmd, b.gyro, b.acc, b.rng):
            a.flags.writeable = False
        _oracle[k] = (b, rng0.copy())
    b, seeded = _oracle[k]
    assert np.array_equal(seeded, rng0), "the engine's initial noise words differ between two flights of one configuration"
    return b


def judge(c, table, export_view=False):
    """fly one cell on one table -> ({field: relative error}, [what failed])"""
    d = data_of(c, table)
    got = sm.fly(afa, c, d, export_view=export_view)
    b = oracle_of(c, d, got["rng0"])
    errs = {k: rel_err_vec(got[k], getattr(b, k), FLOORS[k]) for k in STATE}
    if d.ticks.any():
        errs["gyro"] = rel_err_vec(got["gyro"], b.gyro, FLOORS["gyro"])
        errs["acc"] = rel_err_vec(got["acc"], b.acc, FLOORS["acc"])
    if c.logic:
        errs["motor_cmd"] = rel_err_vec(got["motor_cmd"], b.motor_cmd, 1.0)
    tol = tolerances(c, d)
    bad = ["%s %.2e > %.0e" % (k, v, tol[k]) for k, v in errs.items() if not v <= tol[k]]
    if c.noise == 1 and not np.array_equal(got["rng"], b.rng):
        bad.append("rng words")
    if got["logic_ticks"] != int(d.ticks.sum()):
        bad.append("logic_ticks %d != %d" % (got["logic_ticks"], int(d.ticks.sum())))
    if got["time_us"] != sm.STEPS * sm.DT_US:
        bad.append("time_us %d" % got["time_us"])
    if c.precision == "f64" and c.noise == 2 and c.logic:        # the cells whose bound is a measurement: into the parity ledger
        for k in STATE + ("motor_cmd",):
            record_parity("step_matrix/%s/%s" % (sm.key(c), table), afa.AFE_F64, k, got[k], getattr(b, k), floor=1.0 if k == "motor_cmd" else None)
    return errs, bad


@pytest.mark.parametrize("precision", sm.PRECISIONS)
@pytest.mark.parametrize("family", sm.FAMILIES)
def test_every_step_kernel_against_the_oracle(family, precision):
    t0 = time.perf_counter()
    mine = [c for c in sm.cells() if c.family == family and c.precision == precision]
    assert mine
    ledger = MEASUREMENTS.setdefault("step_matrix", {})
    failures, flights = [], 0
    worst = collections.defaultdict(float)
    for c in mine:
        if c in sm.UNREACHABLE:
            continue
        # an fp32 one-step grid with a force stream and no logic keeps commands and force in LDS (afe_engine.cpp
        # persist_holds_inputs): flown once more with the device view exported first, which makes it read them from memory
        held = family == "grid" and precision == "f32" and c.fext and not c.logic and not c.resident
        for table in sm.TABLES:
            for export_view in ((False, True) if held else (False,)):
                name = "%s/%s%s" % (sm.key(c), table, "/view" if export_view else "")
                try:
                    errs, bad = judge(c, table, export_view)
                except AssertionError as ex:                      # e.g. a cell that was not reached (configure / fly say which)
                    errs, bad = {}, ["assertion: %s" % (str(ex).splitlines() or ["(no message)"])[0]]
                flights += 1
                if errs:
                    k = max(errs, key=errs.get)
                    ledger[name] = {"worst_field": k, "rel_err": errs[k]}
                    group = "f64 counter logic" if (precision == "f64" and c.noise == 2 and c.logic) else "other"
                    for f, v in errs.items():
                        if f in STATE or f == "motor_cmd":
                            worst[group + ", state and commands"] = max(worst[group + ", state and commands"], v)
                        else:
                            worst[group + ", gyro and acc"] = max(worst[group + ", gyro and acc"], v)
                if bad:
                    failures.append("%s: %s" % (name, "; ".join(bad)))
    seconds = time.perf_counter() - t0
    MEASUREMENTS.setdefault("step_matrix_items", {})["%s/%s" % (family, precision)] = dict(
        cells=len(mine), flights=flights, seconds=seconds, oracle_runs_so_far=len(_oracle), worst=dict(worst))
    print("step matrix %s/%s: %d cells, %d flights, %.1f s, worst %s" % (family, precision, len(mine), flights, seconds,
                                                                         ", ".join("%s %.2e" % kv for kv in sorted(worst.items()))))
    assert not failures, "%d of %d flights failed:\n%s" % (len(failures), flights, "\n".join(failures))
