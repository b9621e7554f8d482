"""Generator of tests/golden/onboard_reference.npz and profiles/onboard_reference.json: the scripted flight of
tests/onboard_flight.py (synthetic_record: 130 vehicles, 1 200 ticks, every event) through the REFERENCE's own
Onboard::QuadcopterLogic -- oracle/_ref/onboard_probe, QuadcopterLogic.cpp and KalmanFilter6DOF.cpp compiled where they lie
against oracle/eigen_trap -- call for call what tests/onboard_reference.py is given (tests/onboard_probe.py writes the mapping
down).  Runs only where the probe exists; imports the restatements, never the reverse.

ASSERTED HERE, WITHOUT A TOLERANCE (a NaN equals any NaN):
  * tests/onboard_checker.py and tests/onboard_reference.py under glibc_math equal the probe bit for bit in every printed field
    of every vehicle after every one of the 1 200 ticks and in every telemetry byte (two fleets: the mixed type table of the
    launch tests and the one tilted record of the resident grid; the scalar restatement flies the whole mixed fleet when this
    file is run, and the recorded subset when tests/test_onboard_reference.py runs it again);
  * the position and velocity estimates are 0 throughout; the probe reached no trap (it would have died by name);
  * the lines of the probe's vehicle mode -- Simulation::Quadcopter_T<Onboard::QuadcopterLogic> -- equal the restated feed's.

THE FIXTURE (numbers and bytes only, at most 128 KiB; a raw dump of the flight is 30 MB).  Per fleet ("mix_", "one_"):
  a) *_state, _reason, _warnings, _running, _cycle, _radio_delta    the discrete fields of every vehicle after every tick (the
                                                                   radio timer's reset time as its difference from tick to tick)
  b) *_batt_*, _main_dt_*, _cmd_dt_*                                floats that depend on clocks and events alone, in full
                                                                   (the distinct columns and who has which)
     mix_digest [ticks, 8]                                          one digest per tick over all libm-free floats (below)
  c) *_sub_vehicle, _sub_tick, _sub_values [pairs, 25]              every float field in full on a subset: the first and last vehicle of
                                                                   every group of onboard_flight.groups, one plain vehicle of
                                                                   every type record, NAN_FIRST and the first of every telemetry read, every 100th tick, the last, and the tick
                                                                   before and after every change of state of that vehicle
  d) *_tel_<tick>                                                   all telemetry bytes of the three reads
  e) veh_lines                                                      the vehicle-mode lines
  f) *_inputs_sha256                                                a digest of the bytes the probe was fed
  g) expf_coefficients, libm_fingerprint, tick_clock_delta             the two first-order coefficients; a digest per function of
                                                                   the recording machine's sinf, cosf, acosf, asinf, atan2f on
                                                                   256 fixed arguments each; (now, T, after) of every tick
LIBM-FREE means: no libm call besides sqrtf lies between the inputs and the value.  For the untilted records that is the three
low-pass outputs, the filtered voltage, both lpDt, the angular-velocity estimate, and commands and forces outside the
acceleration state (zeroed in the digest where the state is ACCELERATION).  The tilted record's _R comes from sinf and cosf:
every float field of its vehicles counts as libm-dependent, and so do the attitude estimate and the acceleration-mode commands
of everyone.

profiles/onboard_reference.json: per field, TWICE the largest difference between the checker under glibc_math and under
numpy_math on this script -- two independent libms standing in for "another machine's"; what tests/test_onboard_reference.py
holds the libm-dependent fields to where the test machine's libm is not the recorded one."""
import hashlib
import importlib
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import onboard_checker as oc        # noqa: E402
from tests import onboard_flight as of         # noqa: E402
from tests import onboard_probe as op          # noqa: E402

FIXTURE = os.path.join(HERE, "onboard_reference.npz")
PROFILE = os.path.join(ROOT, "profiles", "onboard_reference.json")
PROBE = op.PROBE
SIZE_LIMIT = 128 * 1024
F = np.float32
FLEETS = (("mix_", False), ("one_", True))
FLOAT_NAMES = tuple(n for n, _ in op.FLOATS if n not in ("est_pos", "est_vel"))          # 25 floats in all
CLOCK_ONLY = (("batt", "batt_filtered"), ("main_dt", "main_loop_dt"), ("cmd_dt", "cmd_dt"))
DISCRETE = (("state", "flight_state"), ("reason", "panic_reason"), ("warnings", "warnings"), ("running", "motors_running"), ("cycle", "cycle_counter"))
LIBM_FREE = ("acc_filtered", "gyro_filtered", "temp_filtered", "batt_filtered", "main_loop_dt", "cmd_dt", "est_ang_vel", "motor_cmd", "motor_forces")
LIBM_DEPENDENT = ("est_att", "motor_cmd", "motor_forces")            # for everyone; for the tilted record every float
ATTITUDE_GROUPS = ("turn", "turn_suppressed", "both_turned", "long")  # whose discrete story runs through the attitude estimate
SPREAD = 100


def afa_package():
    return importlib.import_module("agri-fly_amd")


def same(a, b):
    """bit for bit, a NaN equal to any NaN -> bool array"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    eq = a.view(u) == b.view(u)
    if a.dtype.kind == "f":
        eq |= np.isnan(a) & np.isnan(b)
    return eq


def stack(fields, cmds=None):
    """per-tick dicts -> name -> [ticks, (components,) vehicles]; cmds: the checker's motor commands per tick"""
    names = set(fields[0]) | ({"motor_cmd"} if cmds is not None else set())
    out = {}
    for name in names:
        if name == "motor_cmd" and cmds is not None:
            out[name] = np.stack(cmds)
        else:
            out[name] = np.stack([np.asarray(f[name]) for f in fields])
    return out


def stack_scalar(rows, who):
    """tests/onboard_flight.replay_scalar's rows -> the same shape, vehicles in the order of `who`"""
    out = {}
    for name in rows[0][who[0]]:
        out[name] = np.stack([np.stack([np.asarray(r[i][name]) for i in who], axis=-1) for r in rows])
    for name, dt in op.DISCRETE_DTYPES.items():
        out[name] = out[name].astype(dt)
    return out


def tilted_vehicles(rec):
    """bool [n]: whose type record has a placed mount (TILTED)"""
    tilted = np.array([tuple(float(F(x)) for x in (r.imu_yaw, r.imu_pitch, r.imu_roll)) == tuple(float(F(x)) for x in of.TILTED) for r in rec["llist"]])
    return tilted[np.asarray(rec["types"], int)]


def digest_per_tick(S, plain):
    """[ticks, 8] uint8: blake2b over the libm-free floats of the vehicles `plain` (NaNs made one NaN; commands and forces zeroed
    where the state is ACCELERATION)"""
    ticks = S["flight_state"].shape[0]
    acc_state = S["flight_state"][:, plain] == oc.ACCELERATION
    out = np.zeros((ticks, 8), np.uint8)
    for k in range(ticks):
        h = hashlib.blake2b(digest_size=8)
        for name in LIBM_FREE:
            a = np.array(S[name][k][..., plain], F)
            if name in ("motor_cmd", "motor_forces"):
                a[..., acc_state[k]] = 0
            a[np.isnan(a)] = np.nan
            h.update(np.ascontiguousarray(a).tobytes())
        out[k] = np.frombuffer(h.digest(), np.uint8)
    return out


def subset_vehicles(rec):
    g = of.groups(rec["n"])
    special = np.concatenate(list(g.values())).astype(int)
    who = [int(v[k]) for v in g.values() if len(v) for k in (0, -1)]
    for ty in range(len(rec["llist"])):
        who.append(int(next(i for i in range(rec["n"]) if rec["types"][i] == ty and i not in special and i != of.NAN_FIRST)))
    who.append(of.NAN_FIRST)
    who += [int(e[1]) for events in rec["events"].values() for e in events if e[0] == "telemetry"]      # the first vehicle of every read
    return sorted(set(who))


def subset_pairs(state, who):
    """(vehicle, tick) pairs, ticks 1-based: the spread, the last tick, and the ticks on both sides of every change of state"""
    ticks = state.shape[0]
    pairs = []
    for i in who:
        ts = set(range(1, ticks + 1, SPREAD)) | {ticks}
        for k in np.flatnonzero(state[1:, i] != state[:-1, i]):
            ts |= {int(k) + 1, int(k) + 2}
        pairs += [(i, t) for t in sorted(ts)]
    return np.array(pairs, np.int32)


def values_at(S, pairs, column=None):
    """[pairs, 25] float32 in FLOAT_NAMES' order; column(i): where vehicle i stands on the arrays' last axis"""
    out = []
    for i, t in pairs:
        c = i if column is None else column(int(i))
        out.append(np.concatenate([np.atleast_1d(np.asarray(S[name][t - 1][..., c], F)) for name in FLOAT_NAMES]))
    return np.array(out, F)


def float_columns():
    cols, c = {}, 0
    for name, comps in op.FLOATS:
        if name in FLOAT_NAMES:
            cols[name] = slice(c, c + comps)
            c += comps
    return cols


def libm_fingerprint(math=oc.glibc_math):
    """[5, 8] uint8: a digest per function of its values on 256 fixed arguments (edges included)"""
    rng = np.random.default_rng(20)
    edges = np.array([0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 1e-6, -1e-6, 0.99999994, -0.99999994], F)
    out = np.zeros((5, 8), np.uint8)
    for op_ in range(5):
        scale = 3.2 if op_ < 2 else 1.0
        x = np.concatenate([edges, rng.uniform(-scale, scale, 246).astype(F)])
        y = math(op_, x, np.roll(x, 7)) if op_ == 4 else math(op_, x)
        out[op_] = np.frombuffer(hashlib.blake2b(np.ascontiguousarray(y, F).tobytes(), digest_size=8).digest(), np.uint8)
    return out


def compare_all(got, want, where, names=None):
    """every field bit for bit; fails naming the first tick"""
    for name in (names or sorted(want)):
        if name not in got:
            continue
        eq = same(np.asarray(got[name], np.asarray(want[name]).dtype), want[name])
        if not eq.all():
            bad = np.argwhere(~eq)[0]
            raise AssertionError("%s: %s differs from the reference first at tick %d, index %r: %r against %r (%d values differ)" % (
                where, name, bad[0] + 1, bad[1:].tolist(), np.asarray(got[name])[tuple(bad)], want[name][tuple(bad)], int((~eq).sum())))


def scalar_telemetry(tel, key, who):
    return np.stack([np.stack([np.frombuffer(p, np.uint8) for p in tel[key][i]]) for i in who])


def make_onboard_reference(probe=PROBE, scalar="all", verbose=False):
    afa = afa_package()
    fx, measured = {}, {}
    say = print if verbose else (lambda *a: None)
    for prefix, single in FLEETS:
        rec = of.synthetic_record(afa, single=single)
        fields, telemetry, sha = op.fly_reference(afa, rec, probe)
        R = stack(fields)
        assert len(fields) == of.TICKS and R["flight_state"].shape == (of.TICKS, of.N)
        assert not R["est_pos"].any() and not R["est_vel"].any(), "the position and velocity estimates are 0 without UWB"
        # the numpy checker, every vehicle
        cf, cc, _, ctel, ck = of.replay(afa, rec, oc.glibc_math)
        C = stack(cf, cc)
        compare_all(C, R, prefix + "tests/onboard_checker.py")
        assert set(ctel) == set(telemetry) and len(telemetry) == 3
        for key in telemetry:
            assert np.array_equal(ctel[key], telemetry[key]), (prefix, "checker telemetry", key, np.argwhere(ctel[key] != telemetry[key])[:4].tolist())
        # the scalar restatement
        sub = subset_vehicles(rec)
        who = list(range(of.N)) if (scalar == "all" and not single) else sub
        rows, stel = of.replay_scalar(afa, rec, oc.glibc_math, vehicles=who, with_telemetry=True)
        Sc = stack_scalar(rows, who)
        compare_all(Sc, {k: v[..., who] for k, v in R.items()}, prefix + "tests/onboard_reference.py")
        for key in telemetry:
            inside = [i for i in who if key[1] <= i < key[1] + key[2]]
            if inside:
                want = telemetry[key][[i - key[1] for i in inside]]
                assert np.array_equal(scalar_telemetry(stel, key, inside), want), (prefix, "scalar telemetry", key)
        say(prefix, "checker: %d vehicles, scalar: %d vehicles, %d ticks, all equal the reference bit for bit" % (of.N, len(who), of.TICKS))
        if not single:
            for name, live in oc.BRANCHES.items():
                assert (ck.count[name] > 0) == live, (name, ck.count[name])
            measured = measure_bounds(afa, rec, C)
        # the fixture
        for short, name in DISCRETE:
            fx[prefix + short] = R[name]
        radio = R["last_radio_us"].astype(np.int64)
        fx[prefix + "radio_delta"] = np.diff(radio, axis=0, prepend=np.zeros((1, of.N), np.int64)).astype(np.int32)
        for short, name in CLOCK_ONLY:
            fx[prefix + short + "_columns"], fx[prefix + short + "_index"] = pack_columns(R[name])
        if not single:
            fx[prefix + "digest"] = digest_per_tick(R, ~tilted_vehicles(rec))
        pairs = subset_pairs(R["flight_state"], sub)
        fx[prefix + "sub_vehicle"], fx[prefix + "sub_tick"] = pairs[:, 0].astype(np.uint8), pairs[:, 1].astype(np.uint16)
        fx[prefix + "sub_values"] = values_at(R, pairs)
        for key, got in telemetry.items():
            fx[prefix + "tel_%d" % key[0]] = got
        fx[prefix + "inputs_sha256"] = np.frombuffer(bytes.fromhex(sha), np.uint8)
        fx[prefix + "types"] = np.asarray(rec["types"], np.uint8)
        clocks = np.array([(now, T, after) for now, T, after, _, _ in rec["ticks"]], np.int64)
        delta = np.diff(clocks, axis=0, prepend=np.zeros((1, 3), np.int64)).astype(np.int32)
        if "tick_clock_delta" in fx:
            assert np.array_equal(fx["tick_clock_delta"], delta)
        fx["tick_clock_delta"] = delta
    lines, restated = op.vehicle_lines(afa, probe), op.restated_vehicle_lines(afa)
    for t in op.VEHICLE_TYPES:
        assert lines[t].tobytes() == restated[t].tobytes(), ("vehicle mode, type %d" % t, lines[t], restated[t])
    fx["veh_lines"] = np.stack([lines[t] for t in op.VEHICLE_TYPES])
    fx["veh_types"] = np.array(op.VEHICLE_TYPES, np.int32)
    fx["expf_coefficients"] = np.array([oc.lp1_coefficient(of.PERIOD, 50.0), oc.lp1_coefficient(0.02, 1.0)], F)
    fx["libm_fingerprint"] = libm_fingerprint()
    return fx, measured


def measure_bounds(afa, rec, C):
    """per float field: twice the largest |glibc - numpy| of the checker over the script; and the telemetry codes apart"""
    nf, nc, _, ntel, _ = of.replay(afa, rec, oc.numpy_math)
    N = stack(nf, nc)
    out = {"fields": {}, "what": "2 x the largest difference between tests/onboard_checker.py under glibc_math and under numpy_math on the "
                                 "script of tests/onboard_flight.synthetic_record (130 vehicles, 1 200 ticks); 0 for a field no libm call reaches"}
    with np.errstate(all="ignore"):
        for name in FLOAT_NAMES:
            d = np.abs(C[name].astype(np.float64) - N[name].astype(np.float64))
            d = d[np.isfinite(d)]
            out["fields"][name] = 2.0 * float(d.max()) if d.size else 0.0
    return out


def write_fixture(fx, path=FIXTURE):
    """an .npz whose bytes depend on its arrays alone (np.savez stamps the time of day into the archive)"""
    with zipfile.ZipFile(path, "w") as z:
        for name in sorted(fx):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(fx[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def load_fixture(path=FIXTURE):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def pack_columns(a):
    """float32 [ticks, n] -> (the distinct columns [ticks, u], which one each vehicle has [n]): most vehicles share a story"""
    bits = np.ascontiguousarray(a, F).view(np.uint32)
    cols, index = np.unique(bits, axis=1, return_inverse=True)
    return cols.view(F), np.asarray(index).reshape(-1).astype(np.uint8)


def clock_only(fx, prefix, short):
    """the recorded [ticks, n] of "batt", "main_dt" or "cmd_dt" """
    return fx[prefix + short + "_columns"][:, fx[prefix + short + "_index"]]


def tick_clocks(fx):
    return np.cumsum(fx["tick_clock_delta"].astype(np.int64), axis=0)


def radio_us(fx, prefix):
    return np.cumsum(fx[prefix + "radio_delta"].astype(np.int64), axis=0).astype(np.uint64)


if __name__ == "__main__":
    if not os.path.exists(PROBE):
        sys.exit("oracle/_ref/onboard_probe is not built (make -C oracle ref, where the reference sources are present)")
    fixture, bounds = make_onboard_reference(verbose=True)
    write_fixture(fixture)
    size = os.path.getsize(FIXTURE)
    print("written", FIXTURE, size, "bytes")
    assert size <= SIZE_LIMIT, "larger than 128 KiB"
    with open(PROFILE, "w") as f:
        json.dump(bounds, f, indent=1, sort_keys=True)
        f.write("\n")
    print("written", PROFILE, bounds["fields"])
