"""The flight stage machine on the device (include/agrifly_engine.h, "flight stage machine") against its numpy
specification (tests/stages_checker.py).  The judging rule is the follower's: all arithmetic outside sin, cos, sinf, cosf,
asinf and acosf is IEEE and uncontracted on both sides, so with the device's own values of those six
(afe_stages_selftest_math) the checker equals the device BIT FOR BIT in every field, after every tick; with glibc's values
only their last bits differ, and the sent commands are then equal or one radio code (35 / 32768) apart, in at most 1 % of
the values.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

from tests import scenarios
from tests import stages_checker as sc
from tests.scenarios import afa

pytestmark = pytest.mark.gpu

FAR = (100, 30, 4000.0)      # on the fp32 engine this group stands 4 km out: the anchors matter
INVALID_ARG, HIP, OUT_OF_RANGE, NOT_CONFIGURED = 1, 3, 4, 5
F32, F64 = afa.AFE_F32, afa.AFE_F64
DT_US = 1000


def make_engine(n, precision, noise=False, mode=None):
    params = afa.params_from_type(5)
    e = afa.Ensemble(n, precision=precision)
    e.set_type_table([params])
    if noise:
        e.set_imu_noise(True, 0.1, 0.2, afa.AFE_SEED_DECORRELATED)
    e.set_rates_logic([afa.rates_logic_params_from_type(5)])
    if mode is not None:
        e.set_step_mode(mode)
    return e, afa.scenarios.hover_speed(params)


def make_stages(e, traj_id, far=None, **changes):
    cfg = afa.stages_default_config(5)
    cfg.traj_id = traj_id
    if far is not None:
        sc.far_box(cfg, far)
    for k, v in changes.items():
        setattr(cfg, k, v)
    return afa.FlightStages(e, cfg=cfg), sc.config_from(cfg)


@pytest.fixture(scope="module")
def dmath():
    return sc.device_math(afa)


def apply_step_device(s, step):
    if step["request"] is not None:
        idx, start, stop = step["request"]
        for v in idx:                                        # (runs of one vehicle: the ranges of the ABI)
            s.request(start, stop, first=int(v), count=1)
    for v in ([] if step["warnings"] is None else step["warnings"]):
        s.set_warnings(np.array([afa.AFE_WARN_LOW_BATT], np.uint8), first=int(v))
    for v in ([] if step["unsafe"] is None else step["unsafe"]):
        s.set_unsafe(first=int(v), count=1)


def assert_fields(got, st, where):
    for name in sc.GET_FIELDS:
        g, w = got[name], st[name]
        if not sc.same_bits(g, w):
            g2, w2 = np.atleast_2d(g), np.atleast_2d(w)
            diff = np.argwhere(g2 != w2)[:6]
            raise AssertionError((where, name, g.dtype, w.dtype, diff.tolist(), [(g2[tuple(d)], w2[tuple(d)]) for d in diff]))


def run_script(n, precision, traj_id, dmath, mode=None, with_estimator=False, glibc=False):
    """The scripted mission on the engine: before every tick the clock is advanced, the script's state PUT into the engine (or,
    with the estimator attached, into the estimate) and read back as the device holds it; the checker runs on what was read
    back.  Every field of afe_stages_get, the engine's rates commands and have bytes and the eight counters are compared after
    every tick.  -> what the last tick left, and the glibc comparison's figures"""
    far = FAR if (precision == F32 and not with_estimator) else None
    e, w_hover = make_engine(n, precision, noise=with_estimator, mode=mode)
    est = afa.GpsEstimator(e) if with_estimator else None
    s, cfg = make_stages(e, traj_id, far=far)
    if est is not None:
        s.attach_gps_estimator(est)
    st = sc.new_state(n, cfg)
    des, yaw, centre = sc.desired_for(n, far)
    s.set_desired_position(des)
    s.set_desired_yaw(yaw)
    s.set_centre(centre)
    st["desired_pos"], st["desired_yaw"], st["centre"] = des, yaw, centre
    line = sc.DelayLine(cfg["delay_us"])
    held = (np.zeros((4, n), np.float32), np.zeros(n, np.uint8))
    info, out = {}, {}
    gl = dict(st={k: v.copy() for k, v in st.items()}, differing=0, total=0, largest=0, flight_excess=0.0) if glibc else None
    try:
        first = s.get()
        assert_fields(first, st, "before the first tick")
        t_origin = e.time_us
        for k, step in enumerate(sc.script(n)):
            if est is None:
                e.step(DT_US, step["dt_us"] // DT_US)
            else:
                target = e.time_us + step["dt_us"]
                while e.time_us < target:
                    e.step(DT_US, e.steps_until_tick(DT_US))
                    est.imu()
                est.measure()
            now = e.time_us
            pos, vel, att, _ = sc.script_state(n, k, far)
            if est is None:
                e.set_state(pos, vel, att, np.zeros((3, n)), np.full((4, n), w_hover))
                seen_state = e.get_state()
                pos, vel, att, since = seen_state["pos"], seen_state["vel"], seen_state["att"], np.zeros(n)
            else:
                est.set_state(est=np.concatenate([pos, vel, att, np.zeros((3, n))]))
                back = est.state()
                pos, vel, att = back["est"][0:3], back["est"][3:6], back["est"][6:10]
                since = ((np.uint64(now - t_origin) - back["last_update_us"]).astype(np.float64)) * 1e-6
            apply_step_device(s, step)
            sc.apply_step(st, step)
            counts = s.tick(step["start"], step["stop"], count=True)
            msg = sc.tick(st, cfg, now, pos, vel, att, since, step["start"], step["stop"], dmath, info)
            held = sc.deliver(held, line.tick(now, msg), info)
            got = s.get()
            assert_fields(got, st, (k, "tick"))
            thrust, w, have = e.get_rates_commands()
            assert sc.same_bits(np.concatenate([thrust[None], w]), held[0]) and np.array_equal(have, held[1]), (k, "delivery")
            assert np.array_equal(counts, sc.counters(st)), (k, counts, sc.counters(st))
            assert s.info()["in_flight"] == len(line.queue) and s.info()["n_ticks"] == k + 1
            if gl is not None:
                sc.apply_step(gl["st"], step)
                sc.tick(gl["st"], cfg, now, pos, vel, att, since, step["start"], step["stop"], sc.glibc_math)
                assert np.array_equal(gl["st"]["stage"], st["stage"]) and np.array_equal(gl["st"]["msg_type"], st["msg_type"])
                dist = sc.code_distance(got["sent"], gl["st"]["sent"])
                gl["differing"] += int(np.count_nonzero(dist))
                gl["total"] += dist.size
                gl["largest"] = max(gl["largest"], int(dist.max()))
                fl = st["last_stage"] == sc.FLIGHT
                if fl.any() and traj_id in (1, 2, 3, 4):
                    # the Flight reference: radius * w^k times the largest device-glibc difference of sin / cos on those very
                    # arguments, plus one rounding of the value
                    radius, w_ = {1: (1.0, 0.5), 2: (1.0, 2.0), 3: (0.5, 1.0), 4: (0.5, 0.5)}[traj_id]
                    ts = (np.uint64(now) - st["t0_us"][fl]).astype(np.float64) * 1e-6
                    args = [w_ * ts] + ([(w_ * ts) * 4] if traj_id == 4 else [])
                    d = max(np.abs(dmath(op, a) - sc.glibc_math(op, a)).max() for a in args for op in (0, 1))
                    for name, power in (("last_pos", 0), ("last_vel", 1), ("last_acc", 2)):
                        a_, b_ = got[name][:, fl], gl["st"][name][:, fl]
                        allowed = radius * w_ ** power * d + np.spacing(np.abs(b_).max())
                        gl["flight_excess"] = max(gl["flight_excess"], float(np.abs(a_ - b_).max() - allowed))
        out = dict(got=got, rates=(thrust, w, have), counts=counts, info=info, glibc=gl, state=e.get_state())
    finally:
        s.close()
        if est is not None:
            est.close()
        e.close()
    return out


CASES = [pytest.param(130, F32, 3, id="130-f32-traj3"), pytest.param(130, F64, 4, id="130-f64-traj4"),
         pytest.param(600, F32, 1, id="600-f32-traj1"), pytest.param(600, F64, 2, id="600-f64-traj2"),
         pytest.param(130, F32, 0, id="130-f32-traj0"), pytest.param(130, F64, 5, id="130-f64-traj5")]


def test_device_functions_are_the_library_functions_to_an_ulp_or_two(dmath):
    """not the judging rule, its premise: the device's six functions are ordinary implementations of them"""
    rng = np.random.default_rng(0)
    xd = rng.uniform(-20, 20, 4096)
    for op in (0, 1):
        assert np.abs(dmath(op, xd) - sc.glibc_math(op, xd)).max() <= 4 * np.spacing(1.0)
    x = rng.uniform(-1, 1, 4096).astype(np.float32)
    for op, scale in ((2, 3.2), (3, 3.2), (4, 1.0), (5, 1.0)):
        xs = (x * np.float32(scale)).astype(np.float32)
        d, g = dmath(op, xs), sc.glibc_math(op, xs)
        assert d.dtype == np.float32 and np.abs(d.astype(np.float64) - g).max() <= 4 * np.spacing(np.float32(3.2))
    # the float helpers are the follower's very functions
    for op in (2, 3, 4, 5):
        assert sc.same_bits(dmath(op, x), afa.follower_selftest_math(op - 2, x))


@pytest.mark.parametrize("n,precision,traj_id", CASES)
def test_scripted_mission_is_bit_identical(n, precision, traj_id, dmath):
    out = run_script(n, precision, traj_id, dmath, glibc=True)
    counts = {k: out["info"].get(k, 0) for k, live in sc.BRANCHES.items() if live and not k.startswith("traj") and k != "not_seen"
              and (k != "yaw_nonzero" or traj_id in (1, 2, 4, 5))}
    print(counts)
    for k, v in counts.items():                              # (the truth is always seen: not_seen needs the estimator)
        assert v > 0, "no vehicle takes the branch %r on the engine: %r" % (k, counts)
    assert out["info"]["traj%d" % traj_id] > 0 and out["info"]["cos_le_m1"] == 0
    assert out["counts"][sc.COMPLETE] + out["counts"][sc.EMERGENCY] == n and out["counts"][7] == out["counts"][sc.COMPLETE]
    gl = out["glibc"]
    print("device against glibc: %d of %d codes differ, largest distance %d, flight reference excess %.3g"
          % (gl["differing"], gl["total"], gl["largest"], gl["flight_excess"]))
    scenarios.MEASUREMENTS["stages_device_vs_glibc_codes[%d-%s-traj%d]" % (n, "f32" if precision == F32 else "f64", traj_id)] = {
        "differing": gl["differing"], "of": gl["total"], "largest": gl["largest"]}
    assert gl["largest"] <= 1
    assert gl["differing"] <= 0.01 * gl["total"]
    assert gl["flight_excess"] <= 0.0


def test_scripted_mission_with_the_gps_estimator_is_bit_identical(dmath):
    out = run_script(130, F32, 3, dmath, with_estimator=True)
    assert out["info"]["flight_unsafe"] > 0 and out["info"]["ovr_takeoff_unsafe_to_flight"] > 0 and out["info"]["not_seen"] == 0
    assert out["counts"][sc.COMPLETE] + out["counts"][sc.EMERGENCY] == 130


def test_a_vehicle_the_estimator_has_not_seen_is_killed(dmath):
    """0.6 s of IMU messages without a GPS measurement: GetTimeSinceLastGoodMeasurement passes the timeout, every vehicle is
    in Emergency one tick later, and the checker fed with the estimator's own times says the same to the bit"""
    n = 130
    e, w_hover = make_engine(n, F32, noise=True)
    pos, vel, att, _ = sc.script_state(n, 1)
    e.set_state(pos, vel * 0, att, np.zeros((3, n)), np.full((4, n), w_hover))
    est = afa.GpsEstimator(e)
    s, cfg = make_stages(e, 3)
    s.attach_gps_estimator(est)
    st = sc.new_state(n, cfg)
    try:
        t_origin = e.time_us
        for k, (gap_us, measure) in enumerate(((20000, True), (20000, True), (600000, False), (20000, False))):
            target = e.time_us + gap_us
            while e.time_us < target:
                e.step(DT_US, e.steps_until_tick(DT_US))
                est.imu()
            if measure:
                est.measure()
            now = e.time_us
            back = est.state()
            since = ((np.uint64(now - t_origin) - back["last_update_us"]).astype(np.float64)) * 1e-6
            counts = s.tick(True, False, count=True)
            sc.tick(st, cfg, now, back["est"][0:3], back["est"][3:6], back["est"][6:10], since, True, False, dmath)
            assert_fields(s.get(), st, k)
            assert np.array_equal(counts, sc.counters(st))
        assert since.min() > 0.5 and (st["safety"] & sc.NOT_SEEN).all()
        assert counts[sc.EMERGENCY] == n
    finally:
        s.close()
        est.close()
        e.close()


def test_launches_and_the_resident_grid_give_the_same_bits(dmath):
    a = run_script(130, F32, 3, dmath, mode=afa.AFE_STEP_LAUNCH)
    b = run_script(130, F32, 3, dmath, mode=afa.AFE_STEP_RESIDENT)
    for name in sc.GET_FIELDS:
        assert sc.same_bits(a["got"][name], b["got"][name]), name
    for x, y in zip(a["rates"], b["rates"]):
        assert sc.same_bits(x, y)
    for name in a["state"]:
        assert sc.same_bits(a["state"][name], b["state"][name]), name


def test_two_writers_the_last_one_stands():
    """a follower and a stage machine on one engine both write the rates command: documented, not policed"""
    n = 130
    e, w_hover = make_engine(n, F32)
    pos, vel, att, _ = sc.script_state(n, 1)
    e.set_state(pos, vel, att, np.zeros((3, n)), np.full((4, n), w_hover))
    fcfg = afa.follower_default_config(5)
    fcfg.delay_us = 0
    f = afa.Follower(e, cfg=fcfg)
    s, _ = make_stages(e, 3, delay_us=0)
    try:
        s.tick(True, False)                                  # WaitForStart -> SpoolUp: a message of type 0, nothing written
        e.step(DT_US, 20)
        f.tick()
        s.tick()                                             # SpoolUp's command, delivered at once
        thrust, w, have = e.get_rates_commands()
        sent = s.get(fields=["sent"])["sent"]
        assert have.all() and sc.same_bits(thrust, sent[0]) and sc.same_bits(w, sent[1:4]) and not w.any()
        assert np.float32(thrust[0]) == sent[0, 0] and abs(float(thrust[0]) - 9.81 * 0.25) < 35 / 32768
        e.step(DT_US, 20)
        s.tick()
        f.tick()                                             # now the follower is the last writer
        thrust, w, have = e.get_rates_commands()
        fsent = f.get_command()[1]
        assert sc.same_bits(thrust, fsent[0]) and sc.same_bits(w, fsent[1:4]) and np.abs(w).max() > 0
    finally:
        s.close()
        f.close()
        e.close()


def test_idle_and_kill_packets_leave_what_a_delivery_leaves():
    """afe_set_commands_from_radio with an idle and a kill packet: zeros and have = 0, which is what the machine delivers for
    Complete and Emergency (the scripted mission compares every delivery with this rule)"""
    n = 130
    e, _ = make_engine(n, F32)
    L = afa.library()
    try:
        e.set_rates_commands(np.full(n, 9.81, np.float32), np.ones((3, n), np.float32))
        raw = np.zeros((2, afa.RADIO_PACKET_SIZE), np.uint8)
        assert L.afe_radio_create_simple_command(6, 0, raw[0].ctypes.data) == 0       # idleCommand
        assert L.afe_radio_create_simple_command(2, 0, raw[1].ctypes.data) == 0       # emergencyKill
        assert [afa.radio_decode(raw[i]).type for i in range(2)] == [6, 2]
        e.set_commands_from_radio(raw, first=3)
        thrust, w, have = e.get_rates_commands()
        held = sc.deliver((np.concatenate([np.full((1, 2), 9.81, np.float32), np.ones((3, 2), np.float32)]), np.ones(2, np.uint8)),
                          (np.array([sc.MSG_IDLE, sc.MSG_KILL], np.uint8), np.zeros((4, 2), np.float32)))
        assert sc.same_bits(np.concatenate([thrust[None, 3:5], w[:, 3:5]]), held[0]) and np.array_equal(have[3:5], held[1])
        assert have[:3].all() and have[5:].all() and not have[3:5].any()
    finally:
        e.close()


def test_refusals(dmath):
    L = afa.library()
    n = 130
    cfg = afa.stages_default_config(5)
    h = C.c_void_p()
    bare = afa.Ensemble(n, precision=F32)                    # no rates logic
    bare.set_type_table([afa.params_from_type(5)])
    try:
        assert L.afe_stages_create(bare.handle, C.byref(cfg), C.byref(h)) == NOT_CONFIGURED
    finally:
        bare.close()
    hv = afa.Ensemble(n, precision=F32, host_visible=True)   # a host-visible engine
    hv.set_type_table([afa.params_from_type(5)])
    hv.set_rates_logic([afa.rates_logic_params_from_type(5)])
    try:
        assert L.afe_stages_create(hv.handle, C.byref(cfg), C.byref(h)) == INVALID_ARG
    finally:
        hv.close()
    e, w_hover = make_engine(n, F32, noise=True)
    other, _ = make_engine(n, F32)
    try:
        for field, value in (("struct_bytes", C.sizeof(afa.StagesConfig) - 8), ("traj_id", 6), ("traj_id", -1), ("takeoff_time_s", 0.0)):
            bad = afa.StagesConfig.from_buffer_copy(bytes(cfg))
            setattr(bad, field, value)
            assert L.afe_stages_create(e.handle, C.byref(bad), C.byref(h)) == INVALID_ARG, field
        for axis in range(3):                                # a corner pair that is not ordered: the reference's assert
            bad = afa.StagesConfig.from_buffer_copy(bytes(cfg))
            bad.min_corner[axis] = bad.max_corner[axis]
            assert L.afe_stages_create(e.handle, C.byref(bad), C.byref(h)) == INVALID_ARG, axis
        bad = afa.StagesConfig.from_buffer_copy(bytes(cfg))
        bad.delay_us = 20000 * 15
        assert L.afe_stages_create(e.handle, C.byref(bad), C.byref(h)) == OUT_OF_RANGE
        assert L.afe_stages_create(e.handle, None, C.byref(h)) == INVALID_ARG
        assert L.afe_stages_create(e.handle, C.byref(cfg), None) == INVALID_ARG
        pos, vel, att, _ = sc.script_state(n, 1)
        e.set_state(pos, vel, att, np.zeros((3, n)), np.full((4, n), w_hover))
        est = afa.GpsEstimator(e)
        s = afa.FlightStages(e)
        sh = s._h
        d3 = np.zeros((3, n))
        b = np.zeros(n, np.uint8)
        fields = afa.StagesFields()
        fields.struct_bytes = C.sizeof(afa.StagesFields)
        fields.stage = b.ctypes.data
        # NULL arrays
        assert L.afe_stages_set_desired_position(sh, 0, n, None) == INVALID_ARG
        assert L.afe_stages_set_desired_yaw(sh, 0, n, None) == INVALID_ARG
        assert L.afe_stages_set_centre(sh, 0, n, None) == INVALID_ARG
        assert L.afe_stages_set_warnings(sh, 0, n, None) == INVALID_ARG
        assert L.afe_stages_get(sh, 0, n, None) == INVALID_ARG
        empty = afa.StagesFields()
        empty.struct_bytes = C.sizeof(afa.StagesFields)
        assert L.afe_stages_get(sh, 0, n, C.byref(empty)) == INVALID_ARG
        # a range past the end, negative ranges, sums that wrap
        big = 2 ** 63 - 1
        for first, count, want in ((-1, 1, INVALID_ARG), (0, -1, INVALID_ARG), (0, n + 1, OUT_OF_RANGE), (n + 1, 0, OUT_OF_RANGE),
                                   (n, 1, OUT_OF_RANGE), (big, big, OUT_OF_RANGE), (2, big, OUT_OF_RANGE)):
            assert L.afe_stages_set_desired_position(sh, first, count, d3.ctypes.data) == want, (first, count)
            assert L.afe_stages_set_unsafe(sh, first, count) == want, (first, count)
            assert L.afe_stages_request(sh, first, count, 1, 0) == want, (first, count)
            assert L.afe_stages_set_warnings(sh, first, count, b.ctypes.data) == want, (first, count)
            assert L.afe_stages_get(sh, first, count, C.byref(fields)) == want, (first, count)
        for first in (0, n):                                 # an empty range is answered without touching the engine
            assert L.afe_stages_set_desired_position(sh, first, 0, d3.ctypes.data) == 0
            assert L.afe_stages_get(sh, first, 0, C.byref(fields)) == 0
        assert not s.get(fields=["safety"])["safety"][0] & sc.USER_UNSAFE      # none of the refused calls did anything
        # an estimator on another engine; a tick without the estimator's _imu at the current logic tick
        est_other = afa.GpsEstimator(other)
        assert L.afe_stages_attach_gps_estimator(sh, est_other._h) == INVALID_ARG
        est_other.close()
        s.attach_gps_estimator(est)
        assert L.afe_stages_tick(sh, 0, 0, None) == NOT_CONFIGURED               # no _imu yet
        e.step(DT_US, e.steps_until_tick(DT_US))
        est.imu()
        s.tick()
        e.step(DT_US, e.steps_until_tick(DT_US))                               # a logic tick the estimator has not consumed
        assert L.afe_stages_tick(sh, 0, 0, None) == NOT_CONFIGURED
        assert s.info()["n_ticks"] == 1
        s.attach_gps_estimator(None)
        # ticks closer together than the ring allows: delay 30 ms / period 20 ms is three slots, two in flight and one written
        s.tick()
        s.tick()
        assert L.afe_stages_tick(sh, 0, 0, None) == OUT_OF_RANGE
        assert s.info() == {"n_vehicles": n, "slots": 3, "n_ticks": 3, "in_flight": 3}
        e.step(DT_US, 30)
        s.tick()
        assert s.info()["in_flight"] == 1
        # the rates logic switched off under a live machine
        e.set_rates_logic(None)
        assert L.afe_stages_tick(sh, 0, 0, None) == NOT_CONFIGURED
        # destroy order: stage machine, estimator, engine
        s.close()
        est.close()
    finally:
        e.close()
        other.close()
    assert L.afe_stages_destroy(None) == INVALID_ARG


# ---- a whole mission against the truth, and the safety case (tests/stages_flight.py) ----------------------------------------------
@pytest.fixture(scope="module")
def oracle_mission():
    """the CPU oracle's flight with the numpy checkers (about four seconds): the stages at every tick and the two figures"""
    from oracle import oracle_py as ora
    from tests import stages_flight as sf
    return sf.fly_oracle(ora, afa)


@pytest.mark.parametrize("precision", [pytest.param(F32, id="f32"), pytest.param(F64, id="f64")])
def test_a_whole_mission_against_the_truth(precision, oracle_mission):
    """24 vehicles at rest at ground level, IMU noise under the counter policy, GPS estimator attached; stage times shortened
    (spool-up 0.1 s, take-off 0.6 s, get-into-action 0.4 s, landing speed 1 m/s, 1.2 s of Flight).  The oracle's flight ends
    in Complete with nobody in Emergency; the engine's goes through the same stages at the same ticks and stays within twice
    the oracle's two figures (fp32 state against the oracle's double, the margin of tests/gps_truth_flight.py)."""
    from tests import stages_flight as sf
    want = oracle_mission
    assert (want["stages"][-1] == sc.COMPLETE).all() and not (want["stages"] == sc.EMERGENCY).any()
    assert np.isfinite(want["off_track"]) and np.isfinite(want["final_height"])
    got = sf.fly_engine(afa, precision)
    print("oracle: off track %.4f m, final height %.4f m; engine: %.4f m, %.4f m"
          % (want["off_track"], want["final_height"], got["off_track"], got["final_height"]))
    scenarios.MEASUREMENTS["stages_mission[%s]" % ("f32" if precision == F32 else "f64")] = {
        "oracle_off_track": want["off_track"], "oracle_final_height": want["final_height"], "engine_off_track": got["off_track"],
        "engine_final_height": got["final_height"]}
    assert np.array_equal(got["stages"], want["stages"])
    assert got["off_track"] <= 2 * want["off_track"]
    assert got["final_height"] <= 2 * want["final_height"]
    assert not got["safety"].any()


def test_a_vehicle_pushed_out_of_the_box_is_the_only_one_killed():
    """In Flight an external force of 40 m/s^2 times its mass drives vehicle 7 through the y face of a 12 m x 10 m box.  It is the
    only one in Emergency, and its motors are commanded off one radio delay later: the kill is sent at the first tick that
    enters with Emergency and, 30 ms on a 20 ms period, delivered two ticks after that one."""
    from tests import stages_flight as sf
    victim, from_tick = 7, 55
    force = np.array([0.0, 40.0 * afa.params_from_type(5).mass, 0.0])
    got = sf.fly_engine(afa, F32, box=((-6.0, -5.0, -2.0), (6.0, 5.0, 20.0)), push=(victim, force, from_tick))
    stages, have = got["stages"], got["have"]
    others = np.arange(sf.N) != victim
    assert (stages[-1, others] == sc.COMPLETE).all() and not (stages[:, others] == sc.EMERGENCY).any()
    k_em = int(np.flatnonzero(stages[:, victim] == sc.EMERGENCY)[0])          # index k - 1 of the tick after which it is in Emergency
    assert stages[k_em - 1, victim] == sc.FLIGHT and (stages[k_em:, victim] == sc.EMERGENCY).all() and k_em + 1 > from_tick
    assert got["safety"][k_em, victim] == sc.UNSAFE_POSITION
    assert have[k_em + 2, victim] == 1 and (have[k_em + 3:, victim] == 0).all()
    assert have[k_em + 3, others].all()
