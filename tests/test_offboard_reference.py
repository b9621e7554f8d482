"""The restatements of the offboard controller, the safety net and the prediction pipe against what the REFERENCE's own
code computed: tests/golden/offboard_reference.npz is what oracle/_ref/offboard_probe recorded -- QuadcopterController.cpp,
SafetyNet.hpp and PredictionPipe.hpp compiled where they lie -- on the populations of tests/golden/make_offboard_reference.py.
Everything is compared bit for bit (a NaN equals any NaN).  The reference's outputs carry the recording machine's sinf, cosf,
asinf, acosf and acos; those values travel with the fixture, and the restatements are judged with a table_math that looks
each argument up by its bits and fails by name on one that is not there.  CPU only."""
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from tests import estimator_checker as ec
from tests import follower_checker as fc
from tests import offboard_reference as oref
from tests import offboard_stub
from tests import stage_machine_reference as smr
from tests import stages_checker as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, F = np.float64, np.float32


def _generator():
    spec = importlib.util.spec_from_file_location("make_offboard_reference", os.path.join(ROOT, "tests", "golden", "make_offboard_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ref():
    mod = _generator()
    fx = mod.load_fixture()
    return mod, fx, mod.Table(fx)


def _trk(fx):
    return tuple(fx[k].astype(D) for k in ("trk_pos", "trk_vel", "trk_att"))


def _run(fx):
    return {k: fx["run_" + k] for k in ("pos", "vel", "att", "des_pos", "des_vel", "des_acc", "yaw")}


def test_fixture_holds_the_populations_and_reaches_every_live_branch(ref):
    mod, fx, _ = ref
    assert fx["trk_pos"].shape == (3, 162) and fx["run_pos"].shape == (3, 130) and int(fx["n_sphere"]) == 130 and int(fx["n_level"]) == 32
    mod.check_coverage(fx)
    trk, run = mod.branch_counts(fx, "trk"), mod.branch_counts(fx, "run")
    print(trk, run)
    for k in fc.BRANCHES:
        assert trk[k] > 0, "no recorded vehicle takes the RunTracking branch %r" % k
    for k in ("sat_norm", "z_floor", "thrust_floor", "yaw_nonzero", "cos_ge_1", "n_tiny"):
        assert sc.BRANCHES[k] and run[k] > 0, "no recorded vehicle takes the Run branch %r" % k
    assert not sc.BRANCHES["cos_le_m1"] and run["cos_le_m1"] == 0
    assert os.path.getsize(mod.FIXTURE) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "rigid_body_reference.npz"))
    # the fp32 engines hold these very numbers
    for k in ("trk_pos", "trk_vel", "trk_att", "net_pos", "net_att", "net_since"):
        assert fx[k].dtype == np.float32
    # the hand-placed edges of the Run population are where the generator says
    p = _run(fx)
    g = F(9.81)
    with np.errstate(all="ignore"):
        norms = np.array([np.sqrt(F(p["des_acc"][0, i]) * F(p["des_acc"][0, i]) + F(0) + g * g) for i in range(12, 17)], F)
        zs = np.array([F(p["des_acc"][2, i]) + g for i in range(17, 22)], F)
    ulp20, half = np.spacing(F(20)), F(0.5 * 9.81)
    assert norms[2] == F(20) and np.all(np.diff(norms) > 0) and norms[0] >= F(20) - 2 * ulp20 and norms[4] <= F(20) + 2 * ulp20
    assert zs[2] == half and np.all(np.diff(zs) > 0) and abs(float(zs[0]) - float(half)) <= 2 * np.spacing(half)
    assert fx["run_thrust"][22] > F(-1) and fx["run_thrust"][22] < F(-1) + F(1e-5) and fx["run_thrust"][23] == F(-1)
    assert list(p["att"][:, 24]) == [0, 1, 0, 0]
    assert list(p["yaw"][25:30]) == [0.0, np.pi, -np.pi, 4.0, -7.0]


def test_the_tracking_reference_is_the_plans_of_the_recorded_seed(ref):
    """the plans are not stored: make_plans with the recorded seed must arrive at the recorded ref14 (rows 10..12 through the
    table's acos), or every comparison behind this one reads "inputs differ" """
    mod, fx, table = ref
    pos, vel, att = _trk(fx)
    plans = fc.make_plans(pos, int(fx["seed"]), int(fx["now_us"]))
    ref14 = fc.reference(att, plans, fc.default_config(), int(fx["now_us"]), table.follower())
    for k in range(14):
        assert mod.same(ref14[k], fx["trk_ref14"][k]), k


def test_run_tracking_equals_the_reference(ref):
    mod, fx, table = ref
    pos, vel, att = _trk(fx)
    info = {}
    thrust, rates = fc.run_tracking(pos, vel, att, fx["trk_ref14"], fc.default_config(), table.follower(), info)
    bad = np.flatnonzero(thrust.view(np.uint64) != fx["trk_thrust"].view(np.uint64))
    assert mod.same(thrust, fx["trk_thrust"]), (bad[:8], thrust[bad[:8]], fx["trk_thrust"][bad[:8]])
    assert mod.same(rates, fx["trk_rates"])
    names = fc.BRANCHES + ("theta_small",)
    recorded = np.unpackbits(fx["trk_branch"], axis=1)[:, :162].astype(bool)
    for k in ("cos_ge_1", "cos_le_m1", "n_tiny", "w_le_0", "rot_small", "theta_small"):
        assert np.array_equal(info[k], recorded[names.index(k)]) and info[k].any(), k


def test_run_position_equals_the_reference(ref):
    mod, fx, table = ref
    p = _run(fx)
    info = {}
    thrust, rates = sc.run_position(p["pos"], p["vel"], p["att"], p["des_pos"], p["des_vel"], p["des_acc"], p["yaw"], sc.default_config(),
                                    table.stages(), info)
    assert mod.same(thrust, fx["run_thrust"].astype(D)) and mod.same(rates, fx["run_rates"].astype(D))
    recorded = np.unpackbits(fx["run_branch"], axis=1)[:, :130].astype(bool)
    for i, k in enumerate(mod.RUN_BRANCHES):
        assert np.array_equal(info[k], recorded[i]), k


def test_the_scalar_controller_equals_the_reference_on_every_vehicle(ref):
    mod, fx, table = ref
    p = _run(fx)
    cfg = sc.default_config()
    ctrl = smr.QuadcopterController(cfg["nat_freq"], cfg["damping"], cfg["tc_xy"], cfg["tc_z"])
    recorded = np.unpackbits(fx["run_branch"], axis=1)[:, :130].astype(bool)
    for i in range(130):
        with np.errstate(all="ignore"):
            thrust, w = ctrl.run(p["pos"][:, i], p["vel"][:, i], p["att"][:, i], p["des_pos"][:, i], p["des_vel"][:, i], p["des_acc"][:, i],
                                 p["yaw"][i], table.stages())
        got = np.array([thrust, w[0], w[1], w[2]], D)
        want = np.concatenate([[fx["run_thrust"][i]], fx["run_rates"][:, i]]).astype(D)
        assert mod.same(got, want), (i, got, want)
        for b, k in enumerate(mod.RUN_BRANCHES):
            assert ctrl.seen[k] == bool(recorded[b, i]), (i, k)


def test_the_hover_stub_equals_the_reference_where_it_can_express_the_request(ref, monkeypatch):
    """OffboardHover.controller: desired velocity and acceleration 0, yaw 0.  It evaluates its functions on every lane before it
    selects (acosf of a clipped cosine where the reference never calls acosf): an argument the table lacks answers NaN,
    which reaches the output exactly where the value is used."""
    mod, fx, table = ref
    p = _run(fx)
    monkeypatch.setattr(offboard_stub, "_tr", lambda name, np_fn, x: table.call(name, x, missing_is_nan=True))
    who = np.flatnonzero(mod.run_expressible_by_hover(p))
    assert who.size >= 30 and 0 in who and 24 in who and set(range(30, 35)) <= set(who)
    for i in who:
        stub = offboard_stub.OffboardHover(1, des_pos=p["des_pos"][:, i])
        with np.errstate(all="ignore"):
            thrust, w = stub.controller(p["pos"][:, i].reshape(3, 1), p["vel"][:, i].reshape(3, 1), p["att"][:, i].reshape(4, 1))
        assert thrust.dtype == np.float32 and w.dtype == np.float32
        assert mod.same(thrust[0], fx["run_thrust"][i]) and mod.same(w[:, 0], fx["run_rates"][:, i]), (i, thrust, w[:, 0], fx["run_rates"][:, i])


def test_the_mission_forms_the_inputs_the_reference_was_given(ref):
    """the teacher-forced mission of the GPU test on the CPU: stages_checker.tick forms the inputs of Run (no function of libm
    stands in front of them with traj_id 5), their bytes hash to what the generator fed the reference, and the thrust -- which
    has no function of libm in it either -- equals the reference's bit for bit"""
    mod, fx, _ = ref
    pos, vel, att = _trk(fx)
    flown = mod.fly_mission(pos, vel, att, sc.numpy_math)
    assert len(flown) == len(fx["msn_dt_us"]) <= 12
    for k, tick in enumerate(flown):
        assert (tick["stage_before"] == mod.MISSION_STAGE_BEFORE[k]).all()
        assert np.array_equal(mod.inputs_digest(tick["inputs"]), fx["msn_digest"][k]), k
    assert {sc.TAKEOFF, sc.FLIGHT, sc.LANDING} == {mod.MISSION_STAGE_BEFORE[k] for k in fx["msn_recorded"]}
    for r, k in enumerate(fx["msn_recorded"]):
        assert mod.same(flown[k]["thrust"], fx["msn_thrust"][r].astype(D)), k
        assert (flown[k]["fields"]["cmd_yaw"] != 0).all() == (k >= 7)          # the yaw of Flight stays through Landing


# ---- the safety net ---------------------------------------------------------------------------------------------------------
def _user_unsafe(fx):
    user, out = 0, []
    for fresh, set_unsafe in zip(fx["net_fresh"], fx["net_set_unsafe"]):
        user = int(set_unsafe) | (0 if fresh else user)
        out.append(user)
    return np.array(out, np.uint8)


def test_both_safety_nets_equal_the_reference(ref):
    """faces, corners, the height rule at its edge, the timeout at its edge, NaNs and SetUnsafe: the four flags and GetIsSafe"""
    mod, fx, _ = ref
    pos, att, since, flags = fx["net_pos"].astype(D), fx["net_att"].astype(D), fx["net_since"].astype(D), fx["net_flags"]
    n = pos.shape[1]
    want = flags[:, 0] * sc.NOT_SEEN + flags[:, 1] * sc.UNSAFE_POSITION + flags[:, 2] * sc.UPSIDE_DOWN_AND_LOW + flags[:, 3] * sc.USER_UNSAFE
    assert np.array_equal(flags[:, 4] == 1, want == 0)
    # what the issue's author saw, as the reference has it
    nan_all = np.flatnonzero(np.isnan(pos).all(0) & np.isnan(since))
    assert nan_all.size == 1 and flags[nan_all[0], 4] == 1                      # NaN everywhere: every comparison is false, safe
    on_timeout = np.flatnonzero(since == 0.5)
    assert on_timeout.size == 1 and flags[on_timeout[0], 0] == 0                 # timeSince == 0.5 counts as seen
    cfg = sc.default_config()
    corners = np.flatnonzero((pos == cfg["min_corner"][:, None]).all(0) | (pos == cfg["max_corner"][:, None]).all(0))
    assert corners.size == 2 and (flags[corners, 1] == 0).all()                  # exactly on a corner is inside
    # stages_checker.tick
    st = sc.new_state(n, cfg)
    st["user_unsafe"] = _user_unsafe(fx)
    with np.errstate(all="ignore"):
        sc.tick(st, cfg, 100000, pos, np.zeros((3, n)), att, since, False, False, sc.numpy_math)
    assert np.array_equal(st["safety"], want), (st["safety"], want)
    # stage_machine_reference.SafetyNet
    net = None
    for i in range(n):
        if fx["net_fresh"][i] or net is None:
            net = smr.SafetyNet()
            net.set_safe_corners(cfg["min_corner"], cfg["max_corner"], cfg["min_normal_height"])
            assert net.not_seen_timeout == cfg["not_seen_timeout"]
        with np.errstate(all="ignore"):
            net.update_with_estimator(tuple(D(x) for x in pos[:, i]), tuple(D(x) for x in att[:, i]), D(since[i]))
        if fx["net_set_unsafe"][i]:
            net.set_unsafe()
        assert net.bits() == want[i] and net.is_safe() == bool(flags[i, 4]), (i, net.bits(), want[i])


# ---- the pipe -----------------------------------------------------------------------------------------------------------------
def _pipe_through(fx, mod, add, get, clear):
    """the recorded script through a restatement -> what it answered to every GetActiveMessage: (found, id, remaining)"""
    now_us, out = 0, []
    for op in fx["pipe_ops"]:
        if op["op"] == mod.ADD:
            add(now_us, int(op["id"]), int(op["ballistic"]))
        elif op["op"] == mod.ADVANCE:
            now_us += int(op["advance_us"])
        elif op["op"] == mod.GET:
            out.append(get(float(op["t"])))
        else:
            t_us = int(round(float(op["t"]) * 1e6))
            assert t_us * 1e-6 == float(op["t"])
            clear(t_us)
    return out


def _assert_pipe(mod, fx, got, answered=None):
    want = fx["pipe_out"][fx["pipe_ops"]["op"] == mod.GET]
    assert len(got) == len(want)
    compared = 0
    for k, (g, w) in enumerate(zip(got, want)):
        if answered is not None and not answered[k]:
            continue
        compared += 1
        assert g[0] == bool(w["found"]), (k, g, w)
        if w["found"]:
            assert g[1] == w["id"] and mod.same(D(g[2]), D(w["remaining"])), (k, g, w)
    return compared


def test_the_three_pipes_equal_the_reference(ref):
    mod, fx, _ = ref
    delay = float(fx["pipe_delay"])
    n_get = int((fx["pipe_ops"]["op"] == mod.GET).sum())
    # tests/offboard_reference.py
    clock = oref.Clock()
    pipe = oref.PredictionPipe(clock, delay)

    def add(now_us, i, ballistic):
        clock.us = now_us
        pipe.add((i, ballistic))

    def get(t):
        got = pipe.active(t)
        return (False, -1, np.nan) if got is None else (True, got[0][0], got[1])

    sizes = []
    got = _pipe_through(fx, mod, add, get, lambda t_us: (pipe.clear_expired(t_us * 1e-6), sizes.append(len(pipe.msgs))))
    assert _assert_pipe(mod, fx, got) == n_get
    assert sizes == list(fx["pipe_out"]["size"][fx["pipe_ops"]["op"] == mod.CLEAR])
    flags = [m for m in fx["pipe_out"][fx["pipe_ops"]["op"] == mod.GET] if m["found"]]
    assert all(m["ballistic"] == (1 if m["id"] == 2 else 0) for m in flags)       # the flag rides with its message

    # tests/estimator_checker.py: the deque as it is, and the mirror of csrc/afe_estimator_ring.h
    cfg = ec.default_config()
    assert cfg["command_delay_s"] == delay
    for kind in ("deque", "ring"):
        pipe_c = ec.Deque() if kind == "deque" else ec.Ring(ec.ring_slots(cfg))
        est = ec.Estimator(1, cfg, ec.numpy_math, pipe_c)
        need = [0]

        def add_c(now_us, i, ballistic):
            est.announce(now_us, np.zeros((3, 1)), np.full((3, 1), float(i)))

        def get_c(t):
            with np.errstate(all="ignore"):
                acc, _, free, span, _ = est._active(np.array([t]), np.array([True]))
            return (not bool(free[0]), int(acc[0, 0]), float(span[0])), t * 1e6 >= need[0]

        def clear_c(t_us):
            pipe_c.measured(t_us, np.array([t_us], np.uint64), np.array([False]))
            if kind == "ring":
                need[0] = pipe_c.need_us()

        both = _pipe_through(fx, mod, add_c, get_c, clear_c)
        answered = None if kind == "deque" else [a for _, a in both]
        compared = _assert_pipe(mod, fx, [g for g, _ in both], answered)
        print(kind, "compared", compared, "of", n_get)
        if kind == "deque":
            assert compared == n_get
        else:
            # the ring promises nothing before `need`, the ClearExpiredMessages before the last: counted from the script alone
            clears, promised = [0, 0], 0
            for op in fx["pipe_ops"]:
                if op["op"] == mod.CLEAR:
                    clears = [clears[1], float(op["t"])]
                elif op["op"] == mod.GET:
                    promised += float(op["t"]) >= clears[0]
            assert compared == promised and promised >= 0.75 * n_get, (compared, promised, n_get)


# ---- cli/hover_controller.hpp ----------------------------------------------------------------------------------------------------
def test_the_cpp_controller_equals_the_reference_where_libm_is_the_recorded_one(ref, tmp_path):
    """the driver tests/test_mocap_estimator.py compiles from the tree's own headers, fed the fixture's Run and RunTracking
    records.  HoverController calls this machine's libm: where that reproduces every entry of the recorded table the answers
    must be the reference's bit for bit; where it does not, the test has nothing to say and names the first entry."""
    from tests.test_mocap_estimator import CONTROLLER_DRIVER
    mod, fx, table = ref
    differs = table.first_entry_libm_misses()
    if differs is not None:
        pytest.skip("this machine's libm is not the recorded one: " + differs)
    src = tmp_path / "ctrl.cpp"
    src.write_text(CONTROLLER_DRIVER)
    exe = tmp_path / "ctrl"
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "agri-fly_amd", "cli"),
                           str(src), "-o", str(exe)])

    def ask(mode, records):
        text = "".join(" ".join(float(x).hex() for x in r) + "\n" for r in records)
        out = subprocess.run([str(exe), mode], input=text, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
        assert out.returncode == 0, out.stderr[-2000:]
        got = np.array([[float.fromhex(x) for x in line.split()] for line in out.stdout.strip().split("\n")], D)
        assert got.shape == (len(records), 4)
        return got

    p = _run(fx)
    records = np.concatenate([p["pos"], p["vel"], p["att"], p["des_pos"], p["des_vel"], p["des_acc"], p["yaw"][None]]).T
    got = ask("run", records)
    want = np.concatenate([fx["run_thrust"][None], fx["run_rates"]]).T.astype(D)
    bad = [i for i in range(len(want)) if not mod.same(got[i], want[i])]
    assert not bad, ("Run", bad[:8], got[bad[:4]], want[bad[:4]])
    pos, vel, att = _trk(fx)
    r14 = fx["trk_ref14"]
    records = np.concatenate([pos, vel, att, r14[0:9], np.zeros((1, 162)), r14[9:13]]).T
    got = ask("track", records)
    want = np.concatenate([fx["trk_thrust"][None], fx["trk_rates"]]).T
    bad = [i for i in range(len(want)) if not mod.same(got[i], want[i])]
    assert not bad, ("RunTracking", bad[:8], got[bad[:4]], want[bad[:4]])


# ---- the cap, with numpy standing in for the device ---------------------------------------------------------------------------------
def test_another_library_stays_inside_the_radio_code_cap(ref):
    """The GPU tests hold the device's sent codes to the reference's under the project's cap: at most 1 % of the values differ,
    each by one code (35 / 32768).  Here numpy's sinf, cosf, asinf and acosf stand in for the device's: the fixture's seed was
    chosen so that this passes.  The near-level groups are counted and not capped (near level the cap does not hold)."""
    mod, fx, _ = ref
    counts = mod.standin_counts(fx)
    for k, (differing, of, largest) in counts.items():
        print("%s: %d of %d codes differ, largest distance %d" % (k, differing, of, largest))
    assert set(mod.CAPPED) == {"RunTracking sphere", "Run sphere", "mission sphere"} and set(counts) - set(mod.CAPPED) == {
        "RunTracking near-level", "mission near-level"}
    for k in mod.CAPPED:
        differing, of, largest = counts[k]
        assert of >= 520 and differing <= 0.01 * of, (k, counts[k])
        assert largest <= 1, (k, counts[k])


# ---- staleness and recipe ----------------------------------------------------------------------------------------------------------
def test_fixture_is_what_the_probe_writes_now(ref):
    """staleness: the generator run again (needs oracle/_ref/offboard_probe, built where the reference is present).  The
    generator runs the probe twice on every request and requires identical bytes, and asserts that the checkers with the
    recording glibc_math equal the probe bit for bit."""
    mod, fx, _ = ref
    if not os.path.exists(mod.PROBE):
        pytest.skip("oracle/_ref/offboard_probe not built (the reference sources are not on this machine)")
    fresh = mod.make_offboard_reference(mod.PROBE)
    assert sorted(fresh) == sorted(fx)
    for k in fx:
        a, b = np.asarray(fresh[k]), fx[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_probe_recipe_compiles_the_three_pieces_in_place():
    """the probe's include path names oracle/eigen_store (SafetyNet.hpp pulls in MocapStateEstimator.hpp, whose 2x2 members need
    storage) and never tests/shim or eigen_decl; QuadcopterController.cpp is compiled where it lies, the two headers are
    included from there; the flags are the checkers'; built by `make ref`, i.e. by build()"""
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        mk = f.read()
    inc = re.search(r"^OFFBOARD_INC\s*:=(.*)$", mk, re.M).group(1)
    src = re.search(r"^OFFBOARD_SRC\s*:=(.*)$", mk, re.M).group(1)
    recipe = re.search(r"^_ref/offboard_probe:.*\n((?:\t.*\n)+)", mk, re.M).group(1)
    assert all(v in recipe for v in ("$(OFFBOARD_INC)", "$(OFFBOARD_SRC)")) and "-Ieigen_store" in inc.split()
    assert not any("shim" in t or "eigen_decl" in t for t in (inc, src, recipe))
    for flag in ("-ffp-contract=off", "-fno-fast-math", "-O2", "-std=c++11", "-include cassert", "-include sstream"):
        assert flag in recipe
    assert re.search(r"\$\(REF\)/\S*Offboard/QuadcopterController\.cpp", src) and "Estimator.cpp" not in src + recipe
    assert "_ref/offboard_probe" in mk.split("\nref:")[1].split("\n\n")[0]
    assert "offboard_probe" in mk.split("\nREF ?=")[0]                                  # the header comment's list
    with open(os.path.join(ROOT, "oracle", "ref_offboard_probe.cpp")) as f:
        probe = f.read()
    for header in ("Components/Offboard/PredictionPipe.hpp", "Components/Offboard/SafetyNet.hpp", "Components/Offboard/QuadcopterController.hpp"):
        assert '#include "%s"' % header in probe
    with open(os.path.join(ROOT, ".gitignore")) as f:
        assert "oracle/_ref/" in f.read().split()
