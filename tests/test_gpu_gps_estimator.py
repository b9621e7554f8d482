"""The GPS + IMU state estimator on the device (include/agrifly_engine.h, "GPS + IMU state estimator") against its numpy
specification (tests/gps_estimator_checker.py).  The judging rule is the mocap estimator's: all arithmetic outside sin, cos
and acosf is IEEE and uncontracted on both sides, so with the device's own values of those three
(afe_gps_estimator_selftest_math) the checker equals the device BIT FOR BIT in every field after every call (a NaN equals
any NaN: gps_estimator_checker.differing says why).  The IMU samples the checker consumes are the raw ones afe_get_imu
reports; the checker runs the logic's mount and both low-passes itself, so the engine's filtered gyro the kernel reads is
judged too.  Needs an MI355X."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import follower_checker as fc
from tests import gps_estimator_checker as gc
from tests.gps_flight import fly_gps
from tests.scenarios import afa

pytestmark = pytest.mark.gpu

N = 130                      # two full waves and two lanes
INVALID_ARG, HIP, OUT_OF_RANGE, NOT_CONFIGURED = 1, 3, 4, 5
TYPE_IDS = (5, 1, 4)
TILTED = (0.3, -0.2, 0.25)   # the third record's IMU mount (yaw, pitch, roll)
DT_US = 1000


def make_engine(n, precision, mode=None, noise=False, seed=3):
    """Under launches: mixed type records, the third with a tilted IMU mount (and, type 4, with drag).  Under the resident
    grid, which takes homogeneous ensembles only, and for one vehicle: that third record alone.  The first half level and at
    rest, the others tilted and moving -- an accelerometer in flight reads thrust and drag alone, so it is the drag of the
    third record's moving vehicles that tilts a first sample --, two in three turning; motor commands at hover from the
    first step (before the first tick the logic has commanded nothing, and a vehicle in free fall measures rounding noise)
    under a rates command that holds the turn; the last vehicle at a NaN position.  IMU noise is ON in a new engine: it is
    switched off unless asked for, or no resting vehicle would measure a vertical acceleration or a zero rate."""
    plist = [afa.params_from_type(t) for t in TYPE_IDS]
    llist = [afa.rates_logic_params_from_type(t) for t in TYPE_IDS]
    for rec in (plist[2], llist[2]):
        rec.imu_yaw, rec.imu_pitch, rec.imu_roll = TILTED
    types = ((np.arange(n) + 2) % 3).astype(np.uint8)
    if mode == afa.AFE_STEP_RESIDENT or n == 1:
        plist, llist, types = [plist[2]], [llist[2]], np.zeros(n, np.uint8)
    e = afa.Ensemble(n, precision=precision)
    e.set_type_table(plist)
    e.set_vehicle_types(types)
    e.set_imu_noise(noise, 0.1, 0.2, afa.AFE_SEED_DECORRELATED)
    e.set_rates_logic(llist)
    if mode is not None:
        e.set_step_mode(mode)
    rng = np.random.default_rng(seed)
    level = np.arange(n) < max(1, n // 2)
    pos = rng.uniform(-5, 5, (3, n)) + np.array([[300.0], [-200.0], [40.0]])
    if n > 1:
        pos[:, n - 1] = np.nan
    att = np.where(level, np.array([[1.0], [0.0], [0.0], [0.0]]), afa.scenarios.random_attitudes(rng, n, max_tilt_deg=40.0))
    w = np.where((np.arange(n) % 3 == 0) | level, 0.0, rng.normal(0, 0.8, (3, n)))
    hover = np.array([p.hover_speed for p in plist])[types]
    vel = np.where(level, 0.0, rng.normal(0, 2.0, (3, n)))
    e.set_state(pos, vel, att, w, np.tile(hover, (4, 1)))
    e.set_motor_cmds(np.tile(hover, (4, 1)).astype(np.float32))
    e.set_rates_commands(np.full(n, 9.81, np.float32), w.astype(np.float32))
    mounts = [(p.imu_yaw, p.imu_pitch, p.imu_roll) for p in llist]
    sampler = gc.Sampler(n, 1.0 / 500.0, mounts, types, [p.gyro_lowpass_cutoff for p in llist])
    return e, sampler


@pytest.fixture(scope="module")
def dmath():
    return gc.device_math(afa)


def test_device_functions_are_the_library_functions_to_an_ulp_or_two(dmath):
    """not the judging rule, its premise"""
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, 4096)
    for op, scale in ((0, 3.2), (1, 3.2)):
        d, g = dmath(op, x * scale), gc.glibc_math(op, x * scale)
        assert (np.abs(d - g) <= 2 * np.spacing(np.abs(g))).all(), op
    d, g = dmath(2, x), gc.glibc_math(2, x)
    assert gc.same_bits(d, d.astype(np.float32).astype(np.float64))                 # a float, widened
    assert (np.abs(d - g) <= 2 * np.spacing(np.abs(g).astype(np.float32))).all()
    edge = dmath(2, np.array([1.0, -1.0, 1.0 + 1e-9, 1.5, np.nan]))
    assert edge[0] == 0.0 and abs(edge[1] - np.pi) < 1e-6 and edge[2] == 0.0 and np.isnan(edge[3]) and np.isnan(edge[4])


def _step_to_tick(e):
    e.step(DT_US, e.steps_until_tick(DT_US))


def _fly_script(e, est, script):
    """the script on the device -> (inputs for the checker, states after every event, singular counts, grid_was_running)"""
    inputs, states, singular, running = [], [], {}, []
    for k, ev in enumerate(script):
        if ev[0] == "imu":
            _step_to_tick(e)
            running.append(e.persistent_running)
            est.imu()
            gyro, acc = e.get_imu()
            inputs.append((e.time_us, acc, gyro))
        elif ev[0] == "measure":
            singular[k] = est.measure(count_reinitialised=True)
            inputs.append((e.time_us, e.get_state()["pos"]))
        elif ev[0] == "reset":
            est.reset(ev[1], ev[2])
            inputs.append(e.time_us)
        else:
            near = e.get_state()["pos"][:, ev[2]:ev[2] + ev[3]]
            e13, c81, k3 = gc.payload(ev[1], ev[3], near)
            est.set_state(e13, c81, k3, first=ev[2])
            inputs.append(near)
        states.append(est.state())
    return inputs, states, singular, running


def _assert_states_equal(got, want, where):
    for k in ("est", "cov", "last_predict_us", "last_update_us", "initialized", "num_resets"):
        bad = np.argwhere(np.atleast_2d(gc.differing(got[k], want[k])))
        if bad.size:
            a, b = np.atleast_2d(got[k]), np.atleast_2d(want[k])
            raise AssertionError("%s, %s: %d values differ, first at %r: device %r, checker %r"
                                 % (where, k, len(bad), bad[:4].tolist(), a[tuple(bad[0])], b[tuple(bad[0])]))


RUNS = [pytest.param((afa.AFE_F32, afa.AFE_STEP_LAUNCH, N), id="f32-launches"), pytest.param((afa.AFE_F64, afa.AFE_STEP_LAUNCH, N), id="f64-launches"),
        pytest.param((afa.AFE_F32, afa.AFE_STEP_RESIDENT, N), id="f32-resident"), pytest.param((afa.AFE_F64, afa.AFE_STEP_RESIDENT, N), id="f64-resident"),
        pytest.param((afa.AFE_F32, afa.AFE_STEP_LAUNCH, 1), id="f32-one-vehicle"), pytest.param((afa.AFE_F64, afa.AFE_STEP_RESIDENT, 1), id="f64-one-vehicle")]


_FLOWN = {}


@pytest.fixture(scope="module", params=RUNS)
def flown(request, dmath):
    if request.param not in _FLOWN:
        _FLOWN[request.param] = _flown(request.param, dmath)
    return _FLOWN[request.param]


@pytest.fixture(scope="module", params=RUNS[:4])
def flown_with_tick(request, dmath):
    """the runs of 130 vehicles: a follower ticks behind the script (its scripted plans need 24 vehicles)"""
    if request.param not in _FLOWN:
        _FLOWN[request.param] = _flown(request.param, dmath)
    return _FLOWN[request.param]


def _flown(param, dmath):
    """The scripted call list on the device and, fed what the engine reported, in the checker with the device's functions
    and with glibc's.  Behind the script a follower is attached and ticks once on the estimate."""
    precision, mode, n = param
    script = gc.make_script(n)
    e, sampler = make_engine(n, precision, mode)
    est = afa.GpsEstimator(e)
    tick = None
    try:
        assert est.info() == {"n_vehicles": n, "n_imu": 0, "n_measures": 0, "last_tick": 0}
        inputs, states, singular, running = _fly_script(e, est, script)
        info = est.info()
        if n >= 2 * fc.N_SPECIAL:
            f = afa.Follower(e)
            try:
                f.attach_gps_estimator(est)
                now = e.time_us
                plans = fc.make_plans(states[-1]["est"][0:3], 5, now)
                f.set_plans(**{k: plans[k] for k in ("planned", "coeffs", "tf", "t_plan_us", "traj_att", "offset", "grav")})
                f.set_hold(plans["hold"])
                f.set_goal(plans["goal"])
                f.tick()
                tick = dict(now=now, plans=plans, cfg=fc.config_from(f.cfg), ref14=f.get_reference())
                tick["computed"], tick["sent"] = f.get_command()
            finally:
                f.close()
    finally:
        est.close()
        e.close()
    runs = {}
    for name, math in (("device", dmath), ("glibc", gc.glibc_math)):
        sampler.gyro.reset(n)
        sampler.acc.reset(n)
        chk = gc.Estimator(n, gc.config_from(afa.gps_estimator_default_config()), math)
        st, sing = gc.run_script(script, chk, inputs, sampler)
        runs[name] = dict(states=st, singular=sing, count=chk.count)
    return dict(n=n, precision=precision, resident=mode == afa.AFE_STEP_RESIDENT, script=script, states=states, singular=singular,
                running=running, info=info, runs=runs, tick=tick)


def test_every_call_is_bit_identical_with_the_devices_functions(flown):
    want = flown["runs"]["device"]
    assert len(flown["states"]) == len(flown["script"])
    for k, (got, exp) in enumerate(zip(flown["states"], want["states"])):
        _assert_states_equal(got, exp, "event %d %r" % (k, flown["script"][k]))
    assert flown["singular"] == want["singular"]
    n_imu = sum(ev[0] == "imu" for ev in flown["script"])
    assert flown["info"]["n_imu"] == n_imu and flown["info"]["n_measures"] == sum(ev[0] == "measure" for ev in flown["script"])
    if flown["resident"]:
        assert all(flown["running"]), "the imu calls did not find the resident grid running"


def test_the_script_reaches_the_branches_on_the_engine(flown):
    counts = flown["runs"]["device"]["count"]
    print(counts)
    skip = ("measure_before_predict", "nan_position", "first_predict_tilted") if flown["n"] == 1 else ()
    for b in gc.SCRIPT_BRANCHES:
        if b not in skip:
            assert counts[b] > 0, "no vehicle takes the branch %r: %r" % (b, counts)
    last = flown["states"][-1]
    ok = slice(0, max(1, flown["n"] - 1))
    assert np.isfinite(last["est"][:, ok]).all() and np.isfinite(last["cov"][:, ok]).all()
    if flown["n"] > 1:
        assert np.isnan(last["est"][0:3, -1]).all()


def test_sent_codes_against_glibc_at_most_one_code_in_at_most_one_percent(flown_with_tick):
    """the follower's cap for the whole chain: the tick an attached follower makes behind the script, on the device, against
    glibc's estimator under glibc's follower.  With the device's functions in both the tick is bit-identical (the NaN
    vehicle left out: which NaN a float operation hands on is the hardware's business).  The cap is the follower tests',
    which state it for attitudes all over the sphere (follower_checker.make_state); near level the follower's own float
    acosf turns one float ulp of sinf / cosf into several codes, with or without an estimator (tests/test_gpu_estimator.py,
    the attached flight).  So the script ends with the estimate set to make_state's attitudes and velocities and one more
    offboard period (gps_estimator_checker.make_script).  On the flight's own estimate, half of it level, the device was
    3 to 5 of 516 codes from glibc, by up to 2 codes."""
    flown = flown_with_tick
    t = flown["tick"]
    assert t is not None
    n = flown["n"]
    ok = np.arange(n - 1)
    pd = flown["runs"]["device"]["states"][-1]["est"]
    assert gc.same_bits(flown["states"][-1]["est"], pd)
    same = fc.tick(pd[0:3], pd[3:6], pd[6:10], t["plans"], t["cfg"], t["now"], fc.device_math(afa))
    assert fc.same_bits(t["computed"][:, ok], same["computed"][:, ok]) and fc.same_bits(t["sent"][:, ok], same["sent"][:, ok])
    assert fc.same_bits(t["ref14"][:, ok], same["ref14"][:, ok])
    pg = flown["runs"]["glibc"]["states"][-1]["est"]
    want = fc.tick(pg[0:3], pg[3:6], pg[6:10], t["plans"], t["cfg"], t["now"], fc.glibc_math)
    dist = fc.code_distance(t["sent"][:, ok], want["sent"][:, ok])
    print("device against glibc throughout: %d of %d sent codes differ, largest distance %d" % (np.count_nonzero(dist), dist.size, dist.max()))
    assert dist.max() <= 1
    assert np.count_nonzero(dist) <= 0.01 * dist.size


# ---- the loop ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,mode", [(afa.AFE_F32, afa.AFE_STEP_RESIDENT), (afa.AFE_F64, afa.AFE_STEP_LAUNCH)], ids=["f32-resident", "f64-launches"])
def test_hundred_offboard_periods_bit_for_bit(dmath, precision, mode):
    """[step to the tick -> imu] x 5 -> measure, 100 times, with IMU noise; compared after every period"""
    e, sampler = make_engine(N, precision, mode, noise=True)
    est = afa.GpsEstimator(e)
    chk = gc.Estimator(N, gc.config_from(est.cfg), dmath)
    steps = set()
    try:
        for period in range(100):
            for _ in range(5):
                k = e.steps_until_tick(DT_US)
                steps.add(k)
                e.step(DT_US, k)
                est.imu()
                gyro, acc = e.get_imu()
                chk.imu(e.time_us, *sampler.sample(gyro, acc))
            est.measure()
            chk.measure(e.time_us, e.get_state()["pos"])
            if period % 10 == 9 or period < 3:
                _assert_states_equal(est.state(), chk.state(), "period %d" % period)
        assert est.info() == {"n_vehicles": N, "n_imu": 500, "n_measures": 100, "last_tick": 500}
    finally:
        est.close()
        e.close()
    print("steps per tick:", steps, chk.count)
    assert chk.count["update"] > 90 * (N - 1)


# ---- the follower, attached, in flight ----------------------------------------------------------------------------------------
def test_attached_follower_flight_is_bit_identical():
    """100 ticks of the field loop in the 6 x 10 orchard, 48 vehicles, at the follower flights' image size: the checker's
    estimator is fed the raw IMU samples and the positions the engine reported; at every tick the device's estimate, planner
    inputs, adopted trajAtt / trajOffset / gravity, reference and computed and sent command equal follower_checker run on
    the CHECKER'S estimate instead of the truth.  Nothing is announced."""
    n = 48
    dm, fm = gc.device_math(afa), fc.device_math(afa)
    lp = afa.rates_logic_params_from_type(5)
    sampler = gc.Sampler(n, 1.0 / 500.0, [(lp.imu_yaw, lp.imu_pitch, lp.imu_roll)], np.zeros(n, int), [lp.gyro_lowpass_cutoff])
    chk = gc.Estimator(n, gc.default_config(), dm)
    seen = {"ticks": 0, "adopted": 0}

    def on_create(e, fol, est, goal):
        seen["cfg"], seen["goal"] = fc.config_from(fol.cfg), goal
        seen["prev_thrust"] = np.full(n, seen["cfg"]["hover_thrust"])
        seen["hold"] = e.get_state()["pos"]

    def on_imu(now, e, est):
        gyro, acc = e.get_imu()
        chk.imu(now, *sampler.sample(gyro, acc))

    def on_measure(now, e, est):
        chk.measure(now, e.get_state()["pos"])

    def before(tick, now, e, fol, est):
        cfg = seen["cfg"]
        s = chk.state()["est"]
        assert gc.same_bits(est.state()["est"], s), tick
        plans = fol.get_plans()
        seen["est"], seen["plans"] = s, plans
        inp = fol.planner_inputs()
        want = fc.planner_inputs(s[0:3], s[3:6], s[6:10], seen["prev_thrust"], seen["goal"], cfg["mount"])
        for k in ("vel0", "acc0", "grav", "cost_vec"):
            assert fc.same_bits(inp[k], want[k]), (tick, k)
        adopted_now = plans["planned"].astype(bool) & (plans["t_plan_us"] == now)
        if adopted_now.any():
            assert fc.same_bits(plans["traj_att"][:, adopted_now], want["cam"][:, adopted_now]), tick
            assert fc.same_bits(plans["offset"][:, adopted_now], s[0:3][:, adopted_now]), tick
            assert fc.same_bits(plans["grav"][:, adopted_now], want["grav"][:, adopted_now]), tick
            seen["adopted"] += int(adopted_now.sum())

    def after(tick, now, e, fol, est):
        cfg, s, plans = seen["cfg"], seen["est"], dict(seen["plans"])
        plans["hold"] = seen["hold"]
        ref14 = fc.reference(s[6:10], plans, cfg, now, fm)
        thrust, w = fc.run_tracking(s[0:3], s[3:6], s[6:10], ref14, cfg, fm)
        with np.errstate(all="ignore"):
            computed = np.concatenate([thrust[None], w]).astype(np.float32)
        got_c, got_s = fol.get_command()
        assert fc.same_bits(fol.get_reference(), ref14), tick
        assert fc.same_bits(got_c, computed), tick
        assert fc.same_bits(got_s, fc.radio_quantise(computed, 35)), tick
        seen["prev_thrust"] = thrust
        seen["ticks"] += 1

    log = fly_gps(afa, n=n, ticks=100, seed=0, on_create=on_create, on_imu=on_imu, on_measure=on_measure,
                  before_tick=before, after_tick=after)
    assert seen["ticks"] == 100 and seen["adopted"] > 0 and log["found"].size > 0
    assert log["estimator_info"] == {"n_vehicles": n, "n_imu": 500, "n_measures": 100, "last_tick": 500}
    _assert_states_equal(log["estimator"], chk.state(), "end of flight")
    err = np.sqrt(((log["estimator"]["est"][0:3] - log["pos"]) ** 2).sum(0))
    print("attached flight: worst |estimate - truth| at the end %.4f m, adopted %d, found %.0f %%" % (err.max(), seen["adopted"], 100 * log["found"].mean()))
    assert np.isfinite(log["pos"]).all() and np.isfinite(log["estimator"]["est"]).all()


# ---- the estimate against the truth ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,mode", [(afa.AFE_F64, afa.AFE_STEP_LAUNCH), (afa.AFE_F32, afa.AFE_STEP_LAUNCH), (afa.AFE_F32, afa.AFE_STEP_RESIDENT)],
                         ids=["f64-launches", "f32-launches", "f32-resident"])
def test_estimate_against_truth_within_twice_the_checkers_error(precision, mode):
    """tests/gps_truth_flight.py on the engine with the device estimator: the largest position, velocity and tilt error
    against the engine's own true state, behind every update from the first on, within twice what the checker shows against
    the CPU oracle's flight of the same scenario (tests/test_gps_estimator_cpu.py measures and records those:
    1.66 mm, 0.0645 m/s, 0.0115 rad).  The one check here that does not go through the restatement."""
    from tests import gps_truth_flight as tf
    from tests.test_gps_estimator_cpu import TRUTH_POSITION_M, TRUTH_TILT_RAD, TRUTH_VELOCITY_M_S
    r = tf.fly_engine(afa, precision, mode)
    print("device against the engine's truth: position %.5g m, velocity %.5g m/s, tilt %.6g rad; %d ticks, %d updates"
          % (r["worst"] + (r["n_ticks"], r["n_updates"])))
    assert (r["n_ticks"], r["n_updates"]) == (299, 59)
    assert 0 < r["worst"][0] <= 2 * TRUTH_POSITION_M
    assert 0 < r["worst"][1] <= 2 * TRUTH_VELOCITY_M_S
    assert 0 < r["worst"][2] <= 2 * TRUTH_TILT_RAD


# ---- stream ordering --------------------------------------------------------------------------------------------------------
from tests.test_gpu_caller_stream import _delay, _delays_as_they_ran, _streams, _timed      # noqa: E402,F401  (the autouse fixture judges the delays)


def _periods(e, est, periods, S=None):
    """-> (state, the longest time an imu + measure pair held the host [ms], the shortest delay queued ahead [ms])"""
    held, bound = 0.0, np.inf
    for _ in range(periods):
        for k in range(5):
            if S is not None and k == 4:
                _delay(S, 1.0, "gps estimator")
                bound = 20.0
            _step_to_tick(e)
            t0 = time.perf_counter()
            est.imu()
            if k == 4:
                est.measure()
            if S is not None and k == 4:
                held = max(held, (time.perf_counter() - t0) * 1e3)
    return est.state(), held, bound


def test_imu_and_measure_do_not_wait_and_are_ordered_on_a_callers_stream():
    """On a caller's stream a delay (tests/test_gpu_caller_stream.py's) is queued ahead of the last step of every period;
    imu and measure behind it return long before the delay ends (they download nothing), and what they computed -- behind
    the step they must see the sample of -- equals the run on the engine's own stream bit for bit.  (A call that ran ahead
    of the step would have consumed the previous tick's sample: with IMU noise every sample differs.)"""
    import torch
    e, _ = make_engine(N, afa.AFE_F32, afa.AFE_STEP_LAUNCH, noise=True)
    est = afa.GpsEstimator(e)
    own, _, _ = _periods(e, est, 4)
    est.close()
    e.close()
    for k, S in enumerate(_streams()):
        e, _ = make_engine(N, afa.AFE_F32, afa.AFE_STEP_LAUNCH, noise=True)
        e.set_stream(S.cuda_stream)
        est = afa.GpsEstimator(e)
        try:
            theirs, held, bound = _periods(e, est, 4, S)
            torch.cuda.synchronize()
        finally:
            est.close()
            e.set_stream(None)
            e.close()
        print("stream %d: imu + measure held the host %.2f ms behind a delay of at least %.0f ms" % (k, held, bound))
        assert held < 0.5 * bound
        _assert_states_equal(theirs, own, "caller's stream %d against the engine's own" % k)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    L = afa.library()
    cfg = afa.gps_estimator_default_config()
    h = C.c_void_p()
    e, _ = make_engine(N, afa.AFE_F32)
    short = afa.GpsEstimatorConfig.from_buffer_copy(bytes(cfg))
    short.struct_bytes = C.sizeof(afa.GpsEstimatorConfig) - 8
    assert L.afe_gps_estimator_create(e.handle, C.byref(short), C.byref(h)) == INVALID_ARG
    assert L.afe_gps_estimator_create(e.handle, None, C.byref(h)) == INVALID_ARG
    assert L.afe_gps_estimator_create(e.handle, C.byref(cfg), None) == INVALID_ARG
    assert L.afe_gps_estimator_create(None, C.byref(cfg), C.byref(h)) == INVALID_ARG
    bare = afa.Ensemble(N, precision=afa.AFE_F32)                 # no rates logic
    bare.set_type_table([afa.params_from_type(5)])
    assert L.afe_gps_estimator_create(bare.handle, C.byref(cfg), C.byref(h)) == NOT_CONFIGURED
    bare.close()
    est = afa.GpsEstimator(e)
    f = afa.Follower(e)
    other, _ = make_engine(N, afa.AFE_F32)
    gh = est._h
    d13, d81, d3 = np.zeros((13, N)), np.zeros((81, N)), np.zeros((3, N))
    try:
        # the tick rule: no tick yet; one tick; none since; two ticks since
        assert L.afe_gps_estimator_imu(gh) == NOT_CONFIGURED
        _step_to_tick(e)
        est.imu()
        before = est.state()
        assert L.afe_gps_estimator_imu(gh) == NOT_CONFIGURED
        _step_to_tick(e)
        _step_to_tick(e)
        assert L.afe_gps_estimator_imu(gh) == NOT_CONFIGURED
        after = est.state()
        for k in before:
            assert gc.same_bits(before[k], after[k]), k            # nothing changed
        assert est.info() == {"n_vehicles": N, "n_imu": 1, "n_measures": 0, "last_tick": 1}
        est.reset()
        # all arrays NULL; ranges: negative, beyond the end, and sums that wrap; empty requests
        assert L.afe_gps_estimator_get_state(gh, 0, N, None, None, None, None, None, None) == INVALID_ARG
        assert L.afe_gps_estimator_set_state(gh, 0, N, None, None, None) == INVALID_ARG
        big = 2 ** 63 - 1
        for first, count, want in ((-1, 1, INVALID_ARG), (0, -1, INVALID_ARG), (0, N + 1, OUT_OF_RANGE), (N + 1, 0, OUT_OF_RANGE),
                                   (N, 1, OUT_OF_RANGE), (big, big, OUT_OF_RANGE), (2, big, OUT_OF_RANGE), (N, 0, 0), (0, 0, 0)):
            assert L.afe_gps_estimator_get_state(gh, first, count, d13.ctypes.data, d81.ctypes.data, None, None, None, None) == want, (first, count)
            assert L.afe_gps_estimator_set_state(gh, first, count, d13.ctypes.data, None, d3.ctypes.data) == want, (first, count)
            assert L.afe_gps_estimator_reset(gh, first, count) == want, (first, count)
        for entry in (L.afe_gps_estimator_imu, L.afe_gps_estimator_destroy):
            assert entry(None) == INVALID_ARG
        assert L.afe_gps_estimator_measure(None, None) == INVALID_ARG
        assert L.afe_gps_estimator_selftest_math(-1, 3, 4, d3.ctypes.data, d3.ctypes.data) == INVALID_ARG
        # the link without a current imu
        f.attach_gps_estimator(est)
        assert L.afe_follower_tick(f._h, None) == NOT_CONFIGURED            # (the estimator is two ticks behind)
        assert L.afe_follower_planner_inputs(f._h, d3.ctypes.data, None, None, None) == NOT_CONFIGURED
        assert L.afe_follower_plan(f._h, C.byref(afa.planner_default_config(64, 48, 10.0 / 256.0, 32.0, 0.116, 0.174, 0.5)), 1,
                                   np.zeros(4).ctypes.data, 1, None, None, None, None) == NOT_CONFIGURED
        fresh = afa.GpsEstimator(e)                                         # (its first imu takes the latest tick)
        f.attach_gps_estimator(fresh)
        assert L.afe_follower_tick(f._h, None) == NOT_CONFIGURED            # no imu at all
        fresh.imu()
        f.tick()
        assert f.info()["n_ticks"] == 1
        _step_to_tick(e)
        assert L.afe_follower_tick(f._h, None) == NOT_CONFIGURED            # a stale one
        fresh.imu()
        f.tick()
        # the second kind of estimator while one is attached, either way round
        mocap = afa.Estimator(e)
        assert L.afe_follower_attach_estimator(f._h, mocap._h) == INVALID_ARG
        f.attach_gps_estimator(None)
        f.attach_estimator(mocap)
        assert L.afe_follower_attach_gps_estimator(f._h, fresh._h) == INVALID_ARG
        f.attach_estimator(None)
        mocap.close()
        # an estimator on another engine
        stranger = afa.GpsEstimator(other)
        assert L.afe_follower_attach_gps_estimator(f._h, stranger._h) == INVALID_ARG
        stranger.close()
        assert L.afe_follower_attach_gps_estimator(None, gh) == INVALID_ARG
        # a destroyed follower first: the estimators outlive it and go on
        f.close()
        _step_to_tick(e)
        fresh.imu()
        fresh.measure()
        assert fresh.info() == {"n_vehicles": N, "n_imu": 3, "n_measures": 1, "last_tick": e.logic_ticks}
        fresh.close()
    finally:
        f.close()
        est.close()
        other.close()
        e.close()


def test_a_gps_estimator_on_a_host_visible_engine_is_refused():
    e = afa.Ensemble(N, precision=afa.AFE_F32, host_visible=True)
    e.set_type_table([afa.params_from_type(5)])
    e.set_rates_logic([afa.rates_logic_params_from_type(5)])
    h = C.c_void_p()
    try:
        assert afa.library().afe_gps_estimator_create(e.handle, C.byref(afa.gps_estimator_default_config()), C.byref(h)) == INVALID_ARG
    finally:
        e.close()
