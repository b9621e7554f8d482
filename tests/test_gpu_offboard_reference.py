"""The follower's and the stage machine's kernels against what the REFERENCE's own QuadcopterController and SafetyNet computed
(tests/golden/offboard_reference.npz, recorded by oracle/_ref/offboard_probe; tests/test_offboard_reference.py holds the
checkers to the same file on the CPU).  The fixture alone is read: no probe runs here and the reference's sources are not
needed.  The judging rule:

  inputs      what the device holds is the fixture's, bit for bit (state, the tracking reference's rows without a library
              function in them, the stage machine's controller inputs): a mismatch there reads "inputs differ"
  thrust      has no sinf, cosf, asinf or acosf in it: the device's equals the reference's bit for bit
  sent codes  carry the device library's functions where the reference's carry glibc's: the project's cap -- at most 1 % of
              the sent values differ, each by one radio code (35 / 32768) -- on the vehicles with attitudes all over the
              sphere.  The 32 near-level vehicles are counted and recorded, not capped.

What was measured goes to tests.scenarios.MEASUREMENTS ("offboard_reference ..."; profiles/offboard_reference.json is a copy).
Needs an MI355X."""
import importlib.util
import os

import numpy as np
import pytest

from tests import follower_checker as fc
from tests import scenarios
from tests import stages_checker as sc
from tests.scenarios import afa

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, F = np.float64, np.float32
PRECISIONS = [pytest.param(afa.AFE_F32, id="f32"), pytest.param(afa.AFE_F64, id="f64")]
DT_US = 1000


def _name(precision):
    return "f32" if precision == afa.AFE_F32 else "f64"


@pytest.fixture(scope="module")
def ref():
    spec = importlib.util.spec_from_file_location("make_offboard_reference", os.path.join(ROOT, "tests", "golden", "make_offboard_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    fx = mod.load_fixture()
    trk = tuple(fx[k].astype(D) for k in ("trk_pos", "trk_vel", "trk_att"))
    return mod, fx, trk


def make_engine(n, precision):
    params = afa.params_from_type(5)
    e = afa.Ensemble(n, precision=precision)
    e.set_type_table([params])
    e.set_rates_logic([afa.rates_logic_params_from_type(5)])
    return e, afa.scenarios.hover_speed(params)


def put(e, w_hover, pos, vel, att):
    """the fixture's state into the engine (on an fp32 engine x and y become the anchor, as in tests/test_gpu_follower.py; z,
    velocity and attitude are float-representable) -> the state as the engine reports it"""
    n = pos.shape[1]
    e.set_state(pos, vel, att, np.zeros((3, n)), np.full((4, n), w_hover))
    return e.get_state()


def assert_state(mod, st, pos, vel, att, where):
    for name, want in (("pos", pos), ("vel", vel), ("att", att)):
        assert mod.same(st[name], want), ("inputs differ", where, name)


def capped(mod, got_sent, ref_sent, n_sphere):
    """-> (sphere: differing, of, largest), (near-level: the same)"""
    return mod.code_differences(got_sent[:, :n_sphere], ref_sent[:, :n_sphere]), mod.code_differences(got_sent[:, n_sphere:], ref_sent[:, n_sphere:])


def largest_difference(a, b):
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(a, D) - np.asarray(b, D))
        return float(np.nanmax(np.where(np.isfinite(d), d, 0.0)))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_follower_tick_equals_the_reference(ref, precision):
    """set_state, set_plans and set_hold from the fixture, one tick: RunTracking on 130 + 32 vehicles"""
    mod, fx, (pos, vel, att) = ref
    n, n_sphere, now = pos.shape[1], int(fx["n_sphere"]), int(fx["now_us"])
    e, w_hover = make_engine(n, precision)
    f = None
    try:
        put(e, w_hover, pos, vel, att)
        t_origin = e.time_us
        e.step(DT_US, now // DT_US)                              # the plans need a past to have been planned in
        assert e.time_us - t_origin == now
        st = put(e, w_hover, pos, vel, att)
        assert_state(mod, st, pos, vel, att, "follower")
        f = afa.Follower(e)
        cfg, want_cfg = fc.config_from(f.cfg), fc.default_config()
        for k in ("period_us", "delay_us", "lookahead", "omega_step", "hover_thrust", "nat_freq", "damping", "tc_xy", "tc_z"):
            assert cfg[k] == want_cfg[k], k
        plans = fc.make_plans(pos, int(fx["seed"]), e.time_us)
        f.set_plans(**{k: plans[k] for k in ("planned", "coeffs", "tf", "t_plan_us", "traj_att", "offset", "grav")})
        f.set_hold(plans["hold"])
        f.set_goal(plans["goal"])
        f.tick()
        ref14 = f.get_reference()
        computed, sent = f.get_command()
    finally:
        if f is not None:
            f.close()
        e.close()
    want14 = fx["trk_ref14"]
    for k in list(range(10)) + [13]:                             # arithmetic and sqrt only
        bad = np.flatnonzero(ref14[k].view(np.uint64) != want14[k].view(np.uint64))
        assert bad.size == 0, ("inputs differ", "ref14 row", k, bad[:8], ref14[k][bad[:8]], want14[k][bad[:8]])
    rates_in = largest_difference(ref14[10:13], want14[10:13])   # these carry the device's acos: recorded, not asserted
    # refThrust + accErr . (R e3): no library function
    with np.errstate(all="ignore"):
        want_thrust = fx["trk_thrust"].astype(F)
        ref_computed = np.concatenate([fx["trk_thrust"][None], fx["trk_rates"]]).astype(F)
    bad = np.flatnonzero(~(np.isnan(computed[0]) & np.isnan(want_thrust)) & (computed[0].view(np.uint32) != want_thrust.view(np.uint32)))
    assert bad.size == 0, ("thrust", bad[:8], computed[0][bad[:8]], want_thrust[bad[:8]])
    sphere, level = capped(mod, sent, mod.sent_of(fx["trk_thrust"], fx["trk_rates"]), n_sphere)
    before = largest_difference(computed[:, :n_sphere], ref_computed[:, :n_sphere])
    print("follower %s: sphere %r, near-level %r, largest difference before quantisation %.3g, reference rates in %.3g"
          % (_name(precision), sphere, level, before, rates_in))
    scenarios.MEASUREMENTS["offboard_reference follower[%s]" % _name(precision)] = {
        "sphere": dict(differing=sphere[0], of=sphere[1], largest=sphere[2]), "near_level": dict(differing=level[0], of=level[1], largest=level[2]),
        "largest_difference_before_quantisation": before, "near_level_largest_difference_before_quantisation":
            largest_difference(computed[:, n_sphere:], ref_computed[:, n_sphere:]), "reference_rates_rows_10_12_largest_difference": rates_in}
    assert sphere[2] <= 1, sphere
    assert sphere[0] <= 0.01 * sphere[1], sphere


def mission_stages(e, mod, n):
    cfg = afa.stages_default_config(5)
    want = mod.mission_config()
    cfg.traj_id = want["traj_id"]
    cfg.spool_up_time_s, cfg.takeoff_time_s, cfg.get_into_action_time_s = want["spool_up_time"], want["takeoff_time"], want["get_into_action_time"]
    s = afa.FlightStages(e, cfg=cfg)
    have = sc.config_from(cfg)
    for k, v in want.items():
        assert np.array_equal(have[k], v), ("the mission's configuration", k, have[k], v)
    return s


@pytest.mark.parametrize("precision", PRECISIONS)
def test_stage_machine_mission_equals_the_reference(ref, precision):
    """a teacher-forced mission through Take-off, Flight and Landing (traj_id 5: the desired point is held and the yaw is
    0.2 t, so no sin or cos stands in front of the controller): the fixture's states are put in before each of the ten ticks,
    the stage times are shortened through the configuration.  Run on 130 + 32 vehicles at the four recorded ticks."""
    mod, fx, (pos, vel, att) = ref
    n, n_sphere = pos.shape[1], int(fx["n_sphere"])
    flown = mod.fly_mission(pos, vel, att, sc.numpy_math)       # the controller's inputs: stages_checker's, no library function
    for k, tick in enumerate(flown):
        assert np.array_equal(mod.inputs_digest(tick["inputs"]), fx["msn_digest"][k]), ("not the inputs the reference was given", k)
    e, w_hover = make_engine(n, precision)
    s = None
    sphere_all, level_all, before = [0, 0, 0], [0, 0, 0], 0.0
    try:
        put(e, w_hover, pos, vel, att)
        s = mission_stages(e, mod, n)
        s.set_desired_position(mod.mission_desired(n))
        t_origin = e.time_us
        recorded = list(fx["msn_recorded"])
        for k, dt_us in enumerate(fx["msn_dt_us"]):
            e.step(DT_US, int(dt_us) // DT_US)
            assert e.time_us - t_origin == flown[k]["now_us"]
            st = put(e, w_hover, pos, vel, att)
            assert_state(mod, st, pos, vel, att, ("mission", k))
            s.tick(k in mod.MISSION_START, k in mod.MISSION_STOP)
            got = s.get()
            want = flown[k]["fields"]
            for name in ("stage", "last_stage", "init_pos", "desired_pos", "last_pos", "last_vel", "last_acc", "cmd_yaw", "msg_type"):
                assert mod.same(got[name], want[name]), ("inputs differ", k, name)
            assert np.array_equal(got["t0_us"] - np.uint64(t_origin), want["t0_us"]), ("inputs differ", k, "t0_us")
            assert not got["safety"].any()
            if k in recorded:
                r = recorded.index(k)
                want_thrust = fx["msn_thrust"][r]
                bad = np.flatnonzero(got["computed"][0].view(np.uint32) != want_thrust.view(np.uint32))
                assert bad.size == 0, ("thrust", k, bad[:8], got["computed"][0][bad[:8]], want_thrust[bad[:8]])
                ref_sent = mod.sent_of(fx["msn_thrust"][r], fx["msn_rates"][r])
                sphere, level = capped(mod, got["sent"], ref_sent, n_sphere)
                assert sphere[2] <= 1, (k, sphere)
                for acc, d in ((sphere_all, sphere), (level_all, level)):
                    acc[0], acc[1], acc[2] = acc[0] + d[0], acc[1] + d[1], max(acc[2], d[2])
                before = max(before, largest_difference(got["computed"][1:4, :n_sphere], fx["msn_rates"][r][:, :n_sphere]))
        assert (got["stage"] == sc.LANDING).all()
    finally:
        if s is not None:
            s.close()
        e.close()
    print("mission %s: sphere %r, near-level %r, largest difference before quantisation %.3g" % (_name(precision), sphere_all, level_all, before))
    scenarios.MEASUREMENTS["offboard_reference mission[%s]" % _name(precision)] = {
        "sphere": dict(differing=sphere_all[0], of=sphere_all[1], largest=sphere_all[2]),
        "near_level": dict(differing=level_all[0], of=level_all[1], largest=level_all[2]), "largest_difference_before_quantisation": before}
    assert sphere_all[1] == 4 * 4 * n_sphere
    assert sphere_all[0] <= 0.01 * sphere_all[1], sphere_all


@pytest.mark.parametrize("precision", PRECISIONS)
def test_safety_byte_equals_the_reference(ref, precision):
    """the SafetyNet population in Flight: faces, corners, the height rule at its edge, a NaN position and SetUnsafe.  The rows
    whose time since the last good measurement is not 0 need an estimator attached and are left to the CPU test: these are the
    rows the ABI reaches without one (net_gpu of the fixture)."""
    mod, fx, _ = ref
    rows = np.flatnonzero(fx["net_gpu"])
    assert rows.size >= 25
    n = 130
    idx = rows[np.arange(n) % rows.size]                         # the population, repeated to two waves and two lanes
    pos, att = fx["net_pos"].astype(D)[:, idx], fx["net_att"].astype(D)[:, idx]
    flags = fx["net_flags"][idx]
    want = flags[:, 0] * sc.NOT_SEEN + flags[:, 1] * sc.UNSAFE_POSITION + flags[:, 2] * sc.UPSIDE_DOWN_AND_LOW + flags[:, 3] * sc.USER_UNSAFE
    assert (want & sc.UNSAFE_POSITION).any() and (want & sc.UPSIDE_DOWN_AND_LOW).any() and (want & sc.USER_UNSAFE).any() and (want == 0).any()
    rest_pos = np.tile(np.array([[0.0], [0.0], [1.0]]), (1, n))
    rest_att = np.tile(np.array([[1.0], [0.0], [0.0], [0.0]]), (1, n))
    e, w_hover = make_engine(n, precision)
    s = None
    try:
        put(e, w_hover, rest_pos, np.zeros((3, n)), rest_att)
        s = mission_stages(e, mod, n)
        s.set_desired_position(rest_pos)
        for k in range(6):                                       # safe and at rest on the desired position until Flight
            e.step(DT_US, int(fx["msn_dt_us"][k]) // DT_US)
            put(e, w_hover, rest_pos, np.zeros((3, n)), rest_att)
            s.tick(k in mod.MISSION_START, False)
        before = s.get(fields=["stage", "safety"])
        assert (before["stage"] == sc.FLIGHT).all() and not before["safety"].any()
        e.step(DT_US, 20)
        st = put(e, w_hover, pos, np.zeros((3, n)), att)
        assert mod.same(st["pos"], pos) and mod.same(st["att"], att), "inputs differ"
        for i in np.flatnonzero(fx["net_set_unsafe"][idx]):
            s.set_unsafe(first=int(i), count=1)
        s.tick()
        got = s.get(fields=["stage", "last_stage", "safety"])
    finally:
        if s is not None:
            s.close()
        e.close()
    assert (got["last_stage"] == sc.FLIGHT).all()
    bad = np.flatnonzero(got["safety"] != want)
    assert bad.size == 0, (bad[:8], idx[bad[:8]], got["safety"][bad[:8]], want[bad[:8]])
    assert np.array_equal(got["stage"], np.where(flags[:, 4] == 1, sc.FLIGHT, sc.EMERGENCY))     # GetIsSafe() decides
    scenarios.MEASUREMENTS["offboard_reference safety[%s]" % _name(precision)] = {"rows": int(rows.size), "vehicles": n, "differing": int(bad.size)}
