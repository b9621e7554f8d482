"""The two restatements of the onboard flight computer (tests/onboard_checker.py numpy, tests/onboard_reference.py scalar) against
what the REFERENCE's own Onboard::QuadcopterLogic computed: tests/golden/onboard_reference.npz is what oracle/_ref/onboard_probe
recorded -- QuadcopterLogic.cpp and KalmanFilter6DOF.cpp compiled where they lie, against oracle/eigen_trap -- when it was given,
call for call, the scripted flight of tests/onboard_flight.synthetic_record (tests/golden/make_onboard_reference.py).

Discrete fields, libm-free floats (digests and values), the telemetry bytes that hold no libm-dependent value and the vehicle-mode
lines are compared bit for bit, unconditionally.  The libm-dependent fields (the attitude estimate, the acceleration-mode
commands, every float of the tilted record) are compared bit for bit where this machine's sinf, cosf, acosf, asinf and atan2f
reproduce the recorded fingerprint -- where the probe is built they must -- and elsewhere held per field to
profiles/onboard_reference.json (twice the largest difference between two independent libms on the same script), telemetry
codes to the cap of tests/test_gpu_onboard.py: one code, at most 1 % of the values.  The numpy checker flies every vehicle; the
scalar restatement flies the recorded subset (tests/test_onboard_cpu.py holds the two to each other on every vehicle, and the
generator holds the scalar one to the reference on every vehicle when it writes the fixture).  CPU only."""
import importlib
import importlib.util
import json
import os
import re

import numpy as np
import pytest

from tests import onboard_checker as oc
from tests import onboard_flight as of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
afa = importlib.import_module("agri-fly_amd")
F = np.float32
TELEMETRY_SHARE = 0.01          # tests/test_gpu_onboard.py test_glibc_functions_change_nothing_discrete: one code, at most 1 %


def _generator():
    spec = importlib.util.spec_from_file_location("make_onboard_reference", os.path.join(ROOT, "tests", "golden", "make_onboard_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ref():
    mod = _generator()
    return mod, mod.load_fixture()


@pytest.fixture(scope="module")
def bounds():
    with open(os.path.join(ROOT, "profiles", "onboard_reference.json")) as f:
        return json.load(f)["fields"]


@pytest.fixture(scope="module")
def exact(ref):
    """does this machine's libm reproduce the recorded fingerprint?"""
    mod, fx = ref
    here = mod.libm_fingerprint()
    is_same = bool((here == fx["libm_fingerprint"]).all())
    names = [n for n, row_h, row_f in zip(("sinf", "cosf", "acosf", "asinf", "atan2f"), here, fx["libm_fingerprint"]) if (row_h != row_f).any()]
    print("libm-dependent fields are compared", "BIT FOR BIT: this machine's libm is the recorded one" if is_same else
          "WITHIN profiles/onboard_reference.json: this machine's %s differ from the recorded ones" % ", ".join(names))
    if os.path.exists(mod.PROBE):
        assert is_same, "the probe is built here, so this is a recording machine: its libm must be the recorded one (%s differ)" % names
    return is_same


@pytest.fixture(scope="module")
def flown(ref):
    """per fleet: the record, the checker's fields of every vehicle, its telemetry, its branch counts"""
    mod, _ = ref
    out = {}
    for prefix, single in mod.FLEETS:
        rec = of.synthetic_record(afa, single=single)
        fields, cmds, _, telemetry, ck = of.replay(afa, rec, oc.glibc_math)
        out[prefix] = (rec, mod.stack(fields, cmds), telemetry, ck)
    return out


def _first_bad(eq):
    bad = np.argwhere(~eq)[0]
    return "first at tick %d, index %r (%d values differ)" % (bad[0] + 1, bad[1:].tolist(), int((~eq).sum()))


def hold_discrete_and_clock_fields(mod, fx, prefix, S, who, column=None, names=None):
    """S[name][ticks, ..., columns]: state, reason, warnings, motors-running, cycle counter, radio reset time, filtered voltage and
    both lpDt (or `names` among them) equal the reference's recorded values at every tick, for the vehicles `who` (standing at
    column(i) of S)"""
    cols = list(who) if column is None else [column(i) for i in who]
    want = {name: fx[prefix + short] for short, name in mod.DISCRETE}
    want["last_radio_us"] = mod.radio_us(fx, prefix)
    for short, name in mod.CLOCK_ONLY:
        want[name] = mod.clock_only(fx, prefix, short)
    assert names is None or set(names) <= set(want)
    for name, w in want.items():
        if names is not None and name not in names:
            continue
        got = np.asarray(S[name])[:, cols]
        eq = mod.same(got.astype(w.dtype), w[:len(got), list(who)])
        assert eq.all(), "%s%s differs from the reference's recorded value %s" % (prefix, name, _first_bad(eq))


def hold_subset_values(mod, fx, prefix, S, exact, bounds, tilted, column=None, who=None):
    """every float field at the recorded (vehicle, tick) pairs: libm-free ones bit for bit, the others bit for bit or within bounds"""
    cols = mod.float_columns()
    pairs = np.stack([fx[prefix + "sub_vehicle"].astype(int), fx[prefix + "sub_tick"].astype(int)], axis=1)
    keep = np.ones(len(pairs), bool) if who is None else np.isin(pairs[:, 0], list(who))
    got, want = mod.values_at(S, pairs[keep], column), fx[prefix + "sub_values"][keep]
    state = fx[prefix + "state"]
    compared = dict(exact=0, bounded=0)
    for r, (i, t) in enumerate(pairs[keep]):
        for name, sl in cols.items():
            dependent = tilted[i] or name == "est_att" or (name in ("motor_cmd", "motor_forces") and state[t - 1, i] == oc.ACCELERATION)
            if exact or not dependent:
                assert mod.same(got[r, sl], want[r, sl]).all(), "%s%s of vehicle %d at tick %d: %r, the reference has %r" % (
                    prefix, name, i, t, got[r, sl], want[r, sl])
                compared["exact"] += 1
            else:
                with np.errstate(all="ignore"):
                    d = np.abs(got[r, sl].astype(np.float64) - want[r, sl])
                ok = (d <= bounds[name]) | (np.isnan(got[r, sl]) & np.isnan(want[r, sl])) | (got[r, sl] == want[r, sl])
                assert ok.all(), "%s%s of vehicle %d at tick %d: %r, the reference has %r (bound %g)" % (prefix, name, i, t, got[r, sl], want[r, sl], bounds[name])
                compared["bounded"] += 1
    return compared


def telemetry_free_mask(fx, prefix, key, tilted):
    """bool [count, 2, 30]: the bytes no libm-dependent value reaches (header, position, velocity, raw voltage, debug 1..5, reason and
    warnings of everyone; of the untilted records also the low-pass outputs, and the forces outside the acceleration state)"""
    k, first, count = key
    mask = np.ones((count, 2, 30), bool)
    for j in range(count):
        i = first + j
        mask[j, 1, 8:14] = False                                       # the attitude
        if tilted[i]:
            mask[j, 0, 2:22] = False                                   # accelerometer, gyro, forces
            mask[j, 1, 14:16] = False                                  # debug 0: the temperature low-pass (a float of the tilted record)
        elif fx[prefix + "state"][k - 1, i] == oc.ACCELERATION:
            mask[j, 0, 14:22] = False
    return mask


def hold_telemetry(fx, prefix, telemetry, exact, tilted, rows=None):
    """telemetry[(tick, first, count)] uint8 [count, 2, 30] (rows: which vehicles of the range are present)"""
    assert sorted(k[0] for k in telemetry) == [200, 400, 1200] and all(len(v) for v in telemetry.values())
    values = apart = 0
    for key, got in telemetry.items():
        want, free = fx[prefix + "tel_%d" % key[0]], telemetry_free_mask(fx, prefix, key, tilted)
        if rows is not None:
            want, free = want[rows[key]], free[rows[key]]
        assert got.shape == want.shape
        if exact:
            assert np.array_equal(got, want), (prefix, key, np.argwhere(got != want)[:4].tolist())
            continue
        assert np.array_equal(got[free], want[free]), (prefix, key, "libm-free bytes", np.argwhere((got != want) & free)[:4].tolist())
        a = got[:, :, 2:].copy().view(np.uint16).astype(np.int64)[:, :, :12]          # (the last two words of part 2 are bytes, and libm-free)
        b = want[:, :, 2:].copy().view(np.uint16).astype(np.int64)[:, :, :12]
        assert (np.abs(a - b) <= 1).all(), (prefix, key)
        values += a.size
        apart += int((a != b).sum())
    assert apart <= TELEMETRY_SHARE * values, (apart, values)


# ---- the numpy checker, every vehicle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", ["mix_", "one_"])
def test_checker_equals_the_reference_in_every_discrete_and_clock_field(ref, flown, prefix):
    """all 130 vehicles after every one of the 1 200 ticks.  This is also the CPU half of tests/test_gpu_onboard_reference.py's
    condition: the synthetic flight (another IMU than the device's) keeps these fields on the reference's recorded values."""
    mod, fx = ref
    rec, S, _, _ = flown[prefix]
    assert np.array_equal(np.array([(now, T, after) for now, T, after, _, _ in rec["ticks"]], np.int64), mod.tick_clocks(fx))
    assert np.array_equal(fx[prefix + "types"], rec["types"])
    hold_discrete_and_clock_fields(mod, fx, prefix, S, range(of.N))


def test_checker_equals_the_reference_in_the_libm_free_digest_of_every_tick(ref, flown):
    mod, fx = ref
    rec, S, _, _ = flown["mix_"]
    plain = ~mod.tilted_vehicles(rec)
    assert plain.sum() >= 2 * of.N // 3
    got = mod.digest_per_tick(S, plain)
    eq = (got == fx["mix_digest"]).all(axis=1)
    assert eq.all(), "the libm-free floats of the untilted vehicles differ from the reference's first at tick %d (%d ticks differ)" % (
        int(np.flatnonzero(~eq)[0]) + 1, int((~eq).sum()))


@pytest.mark.parametrize("prefix", ["mix_", "one_"])
def test_checker_equals_the_reference_on_the_recorded_subset_and_in_the_telemetry(ref, flown, exact, bounds, prefix):
    mod, fx = ref
    rec, S, telemetry, _ = flown[prefix]
    tilted = mod.tilted_vehicles(rec)
    compared = hold_subset_values(mod, fx, prefix, S, exact, bounds, tilted)
    print(prefix, "pairs", len(fx[prefix + "sub_tick"]), compared)
    hold_telemetry(fx, prefix, telemetry, exact, tilted)
    assert np.array_equal(np.array([oc.lp1_coefficient(of.PERIOD, 50.0), oc.lp1_coefficient(0.02, 1.0)], F).view(np.uint32),
                          fx["expf_coefficients"].view(np.uint32))


def test_another_library_stays_inside_the_recorded_bounds(ref, bounds):
    """the branch a machine with another libm takes, taken here with numpy's functions standing in for it: the discrete and
    libm-free comparisons stay exact, the others stay inside profiles/onboard_reference.json and the telemetry cap"""
    mod, fx = ref
    rec = of.synthetic_record(afa)
    fields, cmds, _, telemetry, _ = of.replay(afa, rec, oc.numpy_math)
    S, tilted = mod.stack(fields, cmds), mod.tilted_vehicles(rec)
    hold_discrete_and_clock_fields(mod, fx, "mix_", S, range(of.N))
    assert (mod.digest_per_tick(S, ~tilted) == fx["mix_digest"]).all()
    compared = hold_subset_values(mod, fx, "mix_", S, False, bounds, tilted)
    assert compared["bounded"] > 500 and compared["exact"] > 500
    hold_telemetry(fx, "mix_", telemetry, False, tilted)


# ---- the scalar restatement, the recorded subset -------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", ["mix_", "one_"])
def test_scalar_restatement_equals_the_reference_on_the_recorded_subset(ref, exact, bounds, prefix):
    mod, fx = ref
    rec = of.synthetic_record(afa, single=prefix == "one_")
    who = sorted(set(int(i) for i in fx[prefix + "sub_vehicle"]))
    assert who == mod.subset_vehicles(rec)
    rows, stel = of.replay_scalar(afa, rec, oc.glibc_math, vehicles=who, with_telemetry=True)
    S, tilted = mod.stack_scalar(rows, who), mod.tilted_vehicles(rec)
    hold_discrete_and_clock_fields(mod, fx, prefix, S, who, column=who.index)
    hold_subset_values(mod, fx, prefix, S, exact, bounds, tilted, column=who.index)
    telemetry, present = {}, {}
    for key in stel:
        inside = [i for i in who if key[1] <= i < key[1] + key[2]]
        if inside:
            telemetry[key], present[key] = mod.scalar_telemetry(stel, key, inside), [i - key[1] for i in inside]
    hold_telemetry(fx, prefix, telemetry, exact, tilted, rows=present)


def test_the_restated_feed_equals_the_vehicle_mode_lines(ref, flown):
    """Quadcopter_T<Onboard::QuadcopterLogic> of types 1, 2, 4, 5 for 20 logic ticks: the clock of a tick, the call counts, the 25
    degrees, the battery value float(1.2 * threshold) where the filter starts at threshold * 1.2f"""
    from tests import onboard_probe as op
    mod, fx = ref
    assert list(fx["veh_types"]) == list(op.VEHICLE_TYPES) and fx["veh_lines"].shape == (4, op.VEHICLE_TICKS)
    restated = op.restated_vehicle_lines(afa)
    for row, t in zip(fx["veh_lines"], op.VEHICLE_TYPES):
        assert restated[t].tobytes() == row.tobytes(), (t, restated[t], row)
    # the quirk is in the record: the first filtered voltage is not the raw one wherever the two roundings differ
    raw, filt = fx["veh_lines"]["voltage_raw"][:, 0], fx["veh_lines"]["voltage_filtered"][:, 0]
    assert (fx["veh_lines"]["temp_raw"] == 25).all() and (raw != filt).any()
    assert (fx["veh_lines"]["cycle"] == fx["veh_lines"]["batt_count"]).all() and (fx["veh_lines"]["cycle"][:, -1] == op.VEHICLE_TICKS).all()
    # the numpy checker hands over the same battery value (its filter hides a last-place difference of the input: the value itself is held)
    for prefix, _ in mod.FLEETS:
        rec, S, _, _ = flown[prefix]
        ids = np.array(op.type_ids(rec))[np.asarray(rec["types"], int)]
        want = np.array([raw[op.VEHICLE_TYPES.index(int(t))] for t in ids], F)
        assert mod.same(S["volts"][0], want).all(), (prefix, np.flatnonzero(~mod.same(S["volts"][0], want))[:5])


# ---- what the recorded flight covers -------------------------------------------------------------------------------------------------
def test_recorded_flight_takes_every_live_branch_and_no_dead_one(ref, flown):
    """the checker equals the reference in every discrete field of every tick (above), so its branch counts are the reference's;
    the dead branches are dead in the recorded values themselves: nobody is ever FULLY_AUTONOMOUS or UNINITIALIZED, and no first
    panic reason is ESTIMATE_CRAZY, UWB_TIMEOUT or KILLED_INTERNALLY"""
    mod, fx = ref
    count = flown["mix_"][3].count
    assert set(count) == set(oc.BRANCHES)
    for name, live in oc.BRANCHES.items():
        assert (count[name] > 0) == live, (name, count[name])
    for prefix, _ in mod.FLEETS:
        assert set(np.unique(fx[prefix + "state"])) == {oc.IDLE, oc.PANIC, oc.KILLED, oc.ACCELERATION, oc.RATES}
        assert set(np.unique(fx[prefix + "reason"])) == {oc.NO_PANIC, oc.UPSIDE_DOWN, oc.RADIO_TIMEOUT, oc.LOW_BATTERY, oc.KILLED_EXTERNALLY}
        assert set(np.unique(fx[prefix + "warnings"])) <= set(range(32)) and np.bitwise_or.reduce(fx[prefix + "warnings"], axis=None) == 0x1f
    # the subset: the first and last of every group, one plain vehicle of every type record, the NaN one; both sides of every change of state
    rec = flown["mix_"][0]
    sub = set(int(i) for i in fx["mix_sub_vehicle"])
    g = of.groups(of.N)
    assert all({int(v[0]), int(v[-1])} <= sub for v in g.values()) and of.NAN_FIRST in sub
    special = set(int(i) for v in g.values() for i in v)
    assert {int(rec["types"][i]) for i in sub - special} == {0, 1, 2}
    state = fx["mix_state"]
    for i in sub:
        have = set(int(t) for v, t in zip(fx["mix_sub_vehicle"], fx["mix_sub_tick"]) if v == i)
        for k in np.flatnonzero(state[1:, i] != state[:-1, i]):
            assert {int(k) + 1, int(k) + 2} <= have, (i, k)
    nan_rows = fx["mix_sub_values"][fx["mix_sub_vehicle"] == of.NAN_FIRST]
    assert np.isnan(nan_rows[:, mod.float_columns()["est_att"]]).all()      # acosf of a NaN cosine sets no errno: the NaN stays


# ---- staleness, recipe, size ----------------------------------------------------------------------------------------------------------
def test_fixture_is_what_the_probe_writes_now(ref):
    """staleness: the generator run again (needs oracle/_ref/onboard_probe, built where the reference is present), the scalar
    restatement on the recorded subset.  The generator asserts that both restatements equal the probe bit for bit."""
    mod, fx = ref
    if not os.path.exists(mod.PROBE):
        pytest.skip("oracle/_ref/onboard_probe not built (the reference sources are not on this machine)")
    fresh, measured = mod.make_onboard_reference(mod.PROBE, scalar="subset")
    assert sorted(fresh) == sorted(fx)
    for k in fx:
        a, b = np.asarray(fresh[k]), fx[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
    with open(mod.PROFILE) as f:
        assert json.load(f) == json.loads(json.dumps(measured))


def test_fixture_is_small_and_holds_numbers_only(ref):
    mod, fx = ref
    assert os.path.getsize(mod.FIXTURE) <= 128 * 1024 == mod.SIZE_LIMIT
    for k, a in fx.items():
        assert a.dtype.kind in "uif" or (a.dtype.names and all(a.dtype[n].kind in "uif" for n in a.dtype.names)), (k, a.dtype)
    assert fx["mix_inputs_sha256"].shape == (32,) and fx["one_inputs_sha256"].shape == (32,)


def test_probe_recipe_compiles_the_two_sources_in_place_against_the_trap_header():
    """eigen_trap on the include path and none of the other three Eigen headers; QuadcopterLogic.cpp and KalmanFilter6DOF.cpp named
    where they lie; the checkers' flags, and math-errno left on; built by `make ref`, i.e. by build()"""
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        mk = f.read()
    inc = re.search(r"^ONBOARD_INC\s*:=(.*)$", mk, re.M).group(1)
    src = re.search(r"^ONBOARD_SRC\s*:=((?:.*\\\n)*.*)$", mk, re.M).group(1)
    recipe = re.search(r"^_ref/onboard_probe:.*\n((?:\t.*\n)+)", mk, re.M).group(1)
    assert all(v in recipe for v in ("$(ONBOARD_INC)", "$(ONBOARD_SRC)")) and "-Ieigen_trap" in inc.split()
    assert not any("shim" in t or "eigen_decl" in t or "eigen_store" in t for t in (inc, src, recipe))
    for flag in ("-ffp-contract=off", "-fno-fast-math", "-O2", "-std=c++11"):
        assert flag in recipe
    assert "-fno-math-errno" not in recipe and "-ffast-math" not in recipe
    assert re.search(r"\$\(REF\)/\S*Logic/QuadcopterLogic\.cpp", src) and re.search(r"\$\(REF\)/\S*Logic/KalmanFilter6DOF\.cpp", src)
    assert "_ref/onboard_probe" in mk.split("\nref:")[1].split("\n\n")[0]
    assert "onboard_probe" in mk.split("\nREF ?=")[0]                                   # the header comment's list
    with open(os.path.join(ROOT, "oracle", "ref_onboard_probe.cpp")) as f:
        probe = f.read()
    assert '#include "Components/Logic/QuadcopterLogic.hpp"' in probe and "#define private public" in probe
    with open(os.path.join(ROOT, "oracle", "eigen_trap", "Eigen", "Dense")) as f:
        trap = f.read()
    assert "abort()" in trap and re.search(r"Matrix inverse\(\) const;", trap) and "inverse() const {" not in trap
    with open(os.path.join(ROOT, ".gitignore")) as f:
        assert "oracle/_ref/" in f.read().split()
