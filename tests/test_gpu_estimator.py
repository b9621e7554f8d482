"""The mocap state estimator on the device (include/agrifly_engine.h, "mocap state estimator") against its numpy
specification (tests/estimator_checker.py).  The judging rule is the follower's: all arithmetic outside sin, cos, asin, acos
and exp is IEEE and uncontracted on both sides, so with the device's own values of those five
(afe_estimator_selftest_math) the checker equals the device BIT FOR BIT in every field after every call; with glibc's values
the two may differ by what a last bit of those functions carries over the script, which is measured here, not assumed.
Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

from tests import estimator_checker as ec
from tests import follower_checker as fc
from tests.estimator_flight import fly_estimated
from tests import scenarios
from tests.scenarios import afa

pytestmark = pytest.mark.gpu

N = 130                      # two full waves and two lanes
FAR = (100, 30, 4000.0)      # on the fp32 engine this group flies 4 km out: the anchors matter
INVALID_ARG, HIP, OUT_OF_RANGE, NOT_CONFIGURED = 1, 3, 4, 5
# Two runs of the checker over the script, every transcendental result of one moved one ulp up, are 3.1e-14 apart at most
# in the estimate (tests/test_estimator_cpu.py prints it; the covariances never see a transcendental).  The device may be
# 8 x that from the glibc checker: one ulp per call is what the first test below shows, and the factor covers sign and
# accumulation over 40 calls.  The bound that is asserted is measured again on the very poses each run was fed.
ONE_ULP_DRIFT_ON_THE_SCRIPT = 3.1e-14
DRIFT_FACTOR = 8


def make_engine(n, precision, mode=None):
    params = afa.params_from_type(5)
    e = afa.Ensemble(n, precision=precision)
    e.set_type_table([params])
    e.set_rates_logic([afa.rates_logic_params_from_type(5)])
    if mode is not None:
        e.set_step_mode(mode)
    return e, afa.scenarios.hover_speed(params)


def script_cfg():
    c = afa.estimator_default_config()
    c.max_measure_gap_us = 1000 * max(ec.GAPS_MS)
    return c


@pytest.fixture(scope="module")
def dmath():
    return ec.device_math(afa)


RUNS = [pytest.param((afa.AFE_F32, afa.AFE_STEP_LAUNCH), id="f32-launches"), pytest.param((afa.AFE_F64, afa.AFE_STEP_LAUNCH), id="f64-launches"),
        pytest.param((afa.AFE_F32, afa.AFE_STEP_RESIDENT), id="f32-resident"), pytest.param((afa.AFE_F64, afa.AFE_STEP_RESIDENT), id="f64-resident")]


@pytest.fixture(scope="module", params=RUNS)
def flown(request, dmath):
    """The script on the device: the pose of every call is put into the engine, the estimator measures it, and everything
    is downloaded.  Under launches the pose goes in right before the measure call; under the resident grid one step earlier,
    so that it is the measure call that ends the grid (and the pose is the script's after one step of physics).  Beside
    it the checker, fed the poses the engine reported, with the device's functions, with glibc's, and with glibc's moved
    one ulp up."""
    precision, mode = request.param
    resident = mode == afa.AFE_STEP_RESIDENT
    script = ec.make_script(N, 7, FAR if precision == afa.AFE_F32 else None)
    e, w_hover = make_engine(N, precision, mode)
    est = afa.Estimator(e, cfg=script_cfg())
    got = dict(states={}, predictions={}, n_rejected={})
    truth, grid_was_running = {}, []
    zeros3, hover = np.zeros((3, N)), np.full((4, N), w_hover)
    try:
        assert est.info() == {"n_vehicles": N, "slots": 7, "n_measures": 0, "n_messages": 0, "error": 0}
        events = script["events"]
        for k, (kind, arg) in enumerate(events):
            if kind == "step":
                nxt = events[k + 1]
                if nxt[0] == "measure" and resident:
                    if arg > 1:
                        e.step(1000, arg - 1)
                    e.set_state(script["pos"][nxt[1] - 1], zeros3, script["att"][nxt[1] - 1], zeros3, hover)
                    e.step(1000, 1)
                else:
                    e.step(1000, arg)
                    if nxt[0] == "measure":
                        e.set_state(script["pos"][nxt[1] - 1], zeros3, script["att"][nxt[1] - 1], zeros3, hover)
            elif kind == "announce":
                est.announce(script["ang_vel"][arg], script["acc"][arg])
            elif kind == "measure":
                grid_was_running.append(e.persistent_running)
                got["n_rejected"][arg] = est.measure(count_rejected=True)
                assert not e.persistent_running
                st = e.get_state()
                truth[arg] = (st["pos"], st["att"])
                got["states"][arg] = est.state()
            else:
                est.predict(0.03)
                got["predictions"][arg] = est.prediction()
        info = est.info()
        # behind the script: a follower is attached and ticks once on the last prediction, on plans that reach its branches
        f = afa.Follower(e)
        try:
            f.attach_estimator(est)
            now = e.time_us
            plans = fc.make_plans(got["predictions"][ec.N_CALLS][0:3], 5, now)
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
    cfg = ec.config_from(script_cfg())
    runs = {}
    for name, math in (("device", dmath), ("glibc", ec.glibc_math), ("glibc_up", ec.nudged(ec.glibc_math))):
        checker = ec.Estimator(N, cfg, math, ec.Ring(ec.ring_slots(cfg)))
        runs[name] = ec.run_script(script, checker, truth)
        if name == "device":
            counts = checker.count
    return dict(precision=precision, resident=resident, got=got, runs=runs, counts=counts, info=info, truth=truth,
                grid_was_running=grid_was_running, tick=tick)


def test_device_functions_are_the_library_functions_to_an_ulp_or_two(dmath):
    """not the judging rule, its premise: the device's five double functions are ordinary implementations of them"""
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, 4096)
    for op, scale in ((0, 3.2), (1, 3.2), (2, 1.0), (3, 1.0), (4, 3.0)):
        xs = x * scale
        d, g = dmath(op, xs), ec.glibc_math(op, xs)
        assert d.dtype == np.float64 and (np.abs(d - g) <= 2 * np.spacing(np.abs(g))).all(), op
    assert ec.same_bits(dmath(3, x), dmath(3, x.copy()))
    with np.errstate(all="ignore"):
        above = np.array([float(np.nextafter(np.float32(1), np.float32(2))) ** 2, 1.0, 0.0])
    assert np.isnan(dmath(3, above)[0]) and dmath(3, above)[1] == 0.0 and dmath(2, above)[2] == 0.0     # acos above 1 is NaN on the device too


def _assert_states_equal(got, want, call):
    for k in ("est", "cov", "valid_at_us", "started", "rejected_in_a_row", "rejected"):
        a, b = got[k], want[k]
        if not ec.same_bits(a, b):
            bad = np.argwhere(np.atleast_2d(a).view(np.uint64 if a.dtype.itemsize == 8 else a.dtype) !=
                              np.atleast_2d(b).view(np.uint64 if b.dtype.itemsize == 8 else b.dtype))
            raise AssertionError("call %d, %s: %d values differ, first at %r: device %r, checker %r"
                                 % (call, k, len(bad), bad[:4].tolist(), np.atleast_2d(a)[tuple(bad[0])], np.atleast_2d(b)[tuple(bad[0])]))


def test_every_call_is_bit_identical_with_the_devices_functions(flown):
    want = flown["runs"]["device"]
    assert sorted(flown["got"]["states"]) == list(range(1, ec.N_CALLS + 1))
    for c in sorted(flown["got"]["states"]):
        _assert_states_equal(flown["got"]["states"][c], want["states"][c], c)
    assert sorted(flown["got"]["predictions"]) == [10, 20, 30, 40]
    for c, pred in flown["got"]["predictions"].items():
        bad = np.argwhere(pred.view(np.uint64) != want["predictions"][c].view(np.uint64))
        assert bad.size == 0, (c, bad[:4].tolist(), pred[tuple(bad[0])], want["predictions"][c][tuple(bad[0])])
    assert flown["got"]["n_rejected"] == want["n_rejected"]
    assert flown["info"] == {"n_vehicles": N, "slots": 7, "n_measures": ec.N_CALLS, "n_messages": 7, "error": 0}


def test_the_script_reaches_the_branches_on_the_engine(flown):
    counts = flown["counts"]
    print(counts)
    quirk = ("nan_gate",) if flown["resident"] else ()           # (one step of physics normalises the attitude above 1 away)
    for k in ec.BRANCHES:
        if k not in quirk or counts[k]:
            assert counts[k] > 0, "no vehicle takes the branch %r: %r" % (k, counts)
    assert counts["reject"] == 80 and counts["forced_reset"] == 8 and counts["init"] == N + 8
    assert sum(flown["got"]["n_rejected"].values()) == 80
    if flown["precision"] == afa.AFE_F32:
        first, count, metres = FAR
        assert (flown["truth"][1][0][0, first:first + count] > metres - 10).all()
    if flown["resident"]:
        assert all(flown["grid_was_running"]), "the measure calls did not find the resident grid running"
    else:
        assert not any(flown["grid_was_running"])
        q0 = flown["truth"][3][1][0, ec.Q0_ABOVE_1]
        assert q0 > 1.0 and np.isnan(flown["truth"][ec.NAN_CALL][0][:, ec.NAN_POS]).all()


def test_against_glibc_within_eight_times_what_one_ulp_carries(flown):
    runs = flown["runs"]
    one_ulp = ec.drift(runs["glibc"], runs["glibc_up"])
    device = ec.drift(flown["got"], runs["glibc"])
    name = "%s-%s" % ("f32" if flown["precision"] == afa.AFE_F32 else "f64", "resident" if flown["resident"] else "launches")
    print("%s: one ulp of glibc's functions carries %r over the script; the device is %r from the glibc checker" % (name, one_ulp, device))
    scenarios.MEASUREMENTS["estimator_device_vs_glibc[%s]" % name] = {"one_ulp": one_ulp, "device": device}
    assert 0 < one_ulp["est"] < 100 * ONE_ULP_DRIFT_ON_THE_SCRIPT and one_ulp["cov"] == 0.0
    assert device["est"] <= DRIFT_FACTOR * one_ulp["est"]
    assert device["cov"] == 0.0


def test_sent_codes_against_glibc_at_most_one_code_in_at_most_one_percent(flown, dmath):
    """the follower's cap for the whole chain: the tick an attached follower makes behind the script, on the device, against
    glibc's estimator (the checker's last prediction) under glibc's follower.  With the device's functions in both the tick
    is bit-identical (the NaN vehicle left out: which NaN a float operation hands on is the hardware's business)."""
    t = flown["tick"]
    ok = np.delete(np.arange(N), ec.NAN_POS)
    pd = flown["runs"]["device"]["predictions"][ec.N_CALLS]
    same = fc.tick(pd[0:3], pd[3:6], pd[6:10], t["plans"], t["cfg"], t["now"], fc.device_math(afa))
    assert fc.same_bits(t["computed"][:, ok], same["computed"][:, ok]) and fc.same_bits(t["sent"][:, ok], same["sent"][:, ok])
    assert fc.same_bits(t["ref14"][:, ok], same["ref14"][:, ok])
    pg = flown["runs"]["glibc"]["predictions"][ec.N_CALLS]
    want = fc.tick(pg[0:3], pg[3:6], pg[6:10], t["plans"], t["cfg"], t["now"], fc.glibc_math)
    dist = fc.code_distance(t["sent"], want["sent"])
    print("device against glibc throughout: %d of %d sent codes differ, largest distance %d" % (np.count_nonzero(dist), dist.size, dist.max()))
    assert dist.size == 4 * N and dist.max() <= 1
    assert np.count_nonzero(dist) <= 0.01 * dist.size


# ---- announce: from host arrays and from an attached tick --------------------------------------------------------------------
def _stand(e, w_hover, seed):
    pos, vel, att = fc.make_state(e.n, seed)
    att = afa.scenarios.random_attitudes(np.random.default_rng(seed), e.n, max_tilt_deg=10.0)
    e.set_state(pos, vel * 0.2, att, np.zeros((3, e.n)), np.full((4, e.n), w_hover))


def test_host_announce_and_tick_announce_leave_the_same_ring_and_detaching_restores_the_truth():
    """Three estimators on one engine measure the same poses.  A is attached to a follower, whose tick announces; B is
    announced the same command from host arrays -- (cmdAngVel, att e3 cmdThrust - g) of the checker's tick on A's
    prediction, the doubles before any narrowing; C is announced zeros.  The ring has no read-back: what it holds shows
    50 ms later, when the message is the active one -- A and B are then the same bits in every field and C is not.
    Then the follower is detached, and its next tick is the unattached follower's, bit for bit."""
    e, w_hover = make_engine(N, afa.AFE_F32)
    _stand(e, w_hover, 3)
    f = afa.Follower(e)
    hold = e.get_state()["pos"]                                  # nobody gets a plan here: the hold points rule, the true places at creation
    ests = [afa.Estimator(e) for _ in range(3)]
    a, b, c = ests
    cfg = fc.config_from(f.cfg)
    fm = fc.device_math(afa)                                     # (the follower's functions: float, and acos)
    try:
        f.attach_estimator(a)
        for _ in range(2):
            e.step(1000, 5)
            for x in ests:
                x.measure()
        for x in ests:
            x.predict(0.03)
        pred = a.prediction()
        assert ec.same_bits(pred, b.prediction())
        plans = f.get_plans()
        plans["hold"] = hold
        f.tick()
        ref14 = f.get_reference()
        want = fc.reference(pred[6:10], plans, cfg, e.time_us, fm)
        assert fc.same_bits(ref14, want)
        thrust, w = fc.run_tracking(pred[0:3], pred[3:6], pred[6:10], want, cfg, fm)
        assert fc.same_bits(f.get_command()[0], np.concatenate([thrust[None], w]).astype(np.float32))
        ang_vel, acc = ec.announced(pred[6:10], thrust, w)
        b.announce(ang_vel, acc)
        c.announce(np.zeros((3, N)), np.zeros((3, N)))
        assert [x.info()["n_messages"] for x in ests] == [1, 1, 1]
        for _ in range(10):                                      # 50 ms: the message is active from 30 ms on
            e.step(1000, 5)
            for x in ests:
                x.measure()
        for x in ests:
            x.predict(0.03)
        sa, sb, sc = a.state(), b.state(), c.state()
        for k in sa:
            assert ec.same_bits(sa[k], sb[k]), k
        assert ec.same_bits(a.prediction(), b.prediction())
        assert not ec.same_bits(sa["est"], sc["est"]) and ec.same_bits(sa["cov"], sc["cov"])
        # detached: the truth again
        f.attach_estimator(None)
        e.step(1000, 10)
        st = e.get_state()
        f.tick()
        assert a.info()["n_messages"] == 1                       # ... and nothing is announced any more
        want = fc.tick(st["pos"], st["vel"], st["att"], plans, cfg, e.time_us, fm)
        assert fc.same_bits(f.get_reference(), want["ref14"])
        computed, sent = f.get_command()
        assert fc.same_bits(computed, want["computed"]) and fc.same_bits(sent, want["sent"])
    finally:
        f.close()
        for x in ests:
            x.close()
        e.close()


# ---- the follower, attached, in flight ----------------------------------------------------------------------------------------
def test_attached_follower_flight_is_bit_identical():
    """1 s of the estimated loop in the 6 x 10 orchard, 48 vehicles, teacher-forced: the checker's estimator is fed the poses
    the engine reported at every measure call and is announced what the checker's own tick commands; at every one of the 100
    ticks the device's prediction, planner inputs, adopted trajAtt / trajOffset / gravity, reference and computed and sent
    command equal follower_checker run on the CHECKER'S prediction instead of the truth.
    A MEASUREMENT rides along, without an assertion: the same chain with glibc's functions throughout, fed the device's
    poses and announces.  In this flight every vehicle is nearly level, where the float controller's acosf of a cosine next
    to 1 turns one float ulp (which sinf / cosf of the two libraries differ by now and then) into several radio codes: 325
    of 19 200 sent codes differ, by up to 5 -- the estimates themselves agree to 1e-15.  That is the follower's float chain
    near level flight, with or without an estimator; the cap of one code in 1 % is asserted where the follower's own test
    asserts it, on attitudes all over the sphere (test_sent_codes_against_glibc_... above)."""
    n = 48
    dm, fm = ec.device_math(afa), fc.device_math(afa)
    cfg_e = ec.default_config()
    chk = ec.Estimator(n, cfg_e, dm, ec.Ring(ec.ring_slots(cfg_e)))
    chk_g = ec.Estimator(n, cfg_e, ec.glibc_math, ec.Ring(ec.ring_slots(cfg_e)))
    seen = {"ticks": 0, "adopted": 0, "hold": None, "codes": 0, "codes_off": 0, "codes_worst": 0}

    def on_create(e, fol, est, goal):
        seen["cfg"], seen["goal"] = fc.config_from(fol.cfg), goal
        seen["prev_thrust"] = np.full(n, seen["cfg"]["hover_thrust"])
        seen["hold"] = e.get_state()["pos"]                      # the hold points are the TRUE places at creation
        assert est.info()["slots"] == ec.ring_slots(cfg_e)

    def on_measure(now, e, est):
        st = e.get_state()
        chk.measure(now, st["pos"], st["att"])
        chk_g.measure(now, st["pos"], st["att"])

    def before(tick, now, e, fol, est):
        cfg = seen["cfg"]
        pred = chk.predict(now, 0.03)
        assert ec.same_bits(est.prediction(), pred), tick
        plans = fol.get_plans()
        seen["pred"], seen["plans"] = pred, plans
        inp = fol.planner_inputs()
        want = fc.planner_inputs(pred[0:3], pred[3:6], pred[6:10], seen["prev_thrust"], seen["goal"], cfg["mount"])
        for k in ("vel0", "acc0", "grav", "cost_vec"):
            assert fc.same_bits(inp[k], want[k]), (tick, k)
        adopted_now = plans["planned"].astype(bool) & (plans["t_plan_us"] == now)
        if adopted_now.any():                                    # main.cpp:520-523 on estState
            assert fc.same_bits(plans["traj_att"][:, adopted_now], want["cam"][:, adopted_now]), tick
            assert fc.same_bits(plans["offset"][:, adopted_now], pred[0:3][:, adopted_now]), tick
            assert fc.same_bits(plans["grav"][:, adopted_now], want["grav"][:, adopted_now]), tick
            seen["adopted"] += int(adopted_now.sum())

    def after(tick, now, e, fol, est):
        cfg, pred, plans = seen["cfg"], seen["pred"], dict(seen["plans"])
        plans["hold"] = seen["hold"]
        ref14 = fc.reference(pred[6:10], plans, cfg, now, fm)
        thrust, w = fc.run_tracking(pred[0:3], pred[3:6], pred[6:10], ref14, cfg, fm)
        with np.errstate(all="ignore"):
            computed = np.concatenate([thrust[None], w]).astype(np.float32)
        got_c, got_s = fol.get_command()
        assert fc.same_bits(fol.get_reference(), ref14), tick
        assert fc.same_bits(got_c, computed), tick
        assert fc.same_bits(got_s, fc.radio_quantise(computed, 35)), tick
        chk.announce(now, *ec.announced(pred[6:10], thrust, w))
        seen["prev_thrust"] = thrust
        seen["ticks"] += 1
        # glibc's functions all the way: its own estimate and its own command, on the device's poses and announces
        pg = chk_g.predict(now, 0.03)
        ref_g = fc.reference(pg[6:10], plans, cfg, now, fc.glibc_math)
        thrust_g, w_g = fc.run_tracking(pg[0:3], pg[3:6], pg[6:10], ref_g, cfg, fc.glibc_math)
        with np.errstate(all="ignore"):
            sent_g = fc.radio_quantise(np.concatenate([thrust_g[None], w_g]).astype(np.float32), 35)
        dist = fc.code_distance(got_s, sent_g)
        seen["codes"] += dist.size
        seen["codes_off"] += int(np.count_nonzero(dist))
        seen["codes_worst"] = max(seen["codes_worst"], int(dist.max()))
        chk_g.announce(now, *ec.announced(pred[6:10], thrust, w))

    log = fly_estimated(afa, n=n, seconds=1.0, seed=0, log_every=0, on_create=on_create, on_measure=on_measure, before_tick=before,
                        after_tick=after)
    assert seen["ticks"] == 100 and log["found"].mean() > 0.5 and seen["adopted"] > n // 2
    print("device against glibc throughout (same poses, same announces): %d of %d sent codes differ, largest distance %d" % (seen["codes_off"], seen["codes"], seen["codes_worst"]))
    scenarios.MEASUREMENTS["estimator_attached_device_vs_glibc_codes"] = {"differing": seen["codes_off"], "of": seen["codes"],
                                                                          "largest": seen["codes_worst"]}
    assert seen["codes"] == 100 * 4 * n
    assert log["estimator_info"]["n_measures"] == 200 and log["estimator_info"]["error"] == 0
    assert ec.same_bits(log["estimator"]["est"], chk.state()["est"]) and ec.same_bits(log["estimator"]["cov"], chk.state()["cov"])
    assert np.abs(seen["hold"] - log["pos0"]).max() < 1e-6


# ---- free flight --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def free_flight():
    return fly_estimated(afa, n=48, seconds=3.0, seed=0, log_every=1)


def test_free_flight_on_the_estimate(free_flight):
    log = free_flight
    est = log["estimator"]
    assert np.isfinite(est["est"]).all() and np.isfinite(est["cov"]).all() and np.isfinite(log["pred"]).all()
    assert est["started"].all() and not est["rejected"].any() and not est["rejected_in_a_row"].any()     # no rejection after the initialisation
    assert log["estimator_info"] == {"n_vehicles": 48, "slots": 8, "n_measures": 600, "n_messages": 8, "error": 0}
    assert log["planned"].all()                                  # every vehicle has adopted a plan
    assert np.isfinite(log["pos"]).all() and log["trunk"].min() > 0.0
    # the prediction made at a tick is for 30 ms later: three ticks on
    err = np.sqrt(((log["pred"][:-3, 0:3] - log["pos"][3:]) ** 2).sum(1))
    advance = log["pos"][-1, 0] - log["pos0"][0]
    print("\nestimated flight: 48 vehicles, 3 s; worst |prediction - truth 30 ms later| %.4f m (mean %.4f m); x advance %.2f..%.2f m, "
          "min trunk clearance %.3f m, plans found %.0f %%" % (err.max(), err.mean(), advance.min(), advance.max(), log["trunk"].min(),
                                                               100 * log["found"].mean()))
    scenarios.MEASUREMENTS["estimator_flight_prediction_error_m"] = {"worst": float(err.max()), "mean": float(err.mean())}


def test_free_flight_is_reproducible(free_flight):
    again = fly_estimated(afa, n=48, seconds=3.0, seed=0, log_every=1)
    np.testing.assert_array_equal(free_flight["pos"], again["pos"])
    assert ec.same_bits(free_flight["pred"], again["pred"])
    assert ec.same_bits(free_flight["last_sent"], again["last_sent"])
    for k, v in free_flight["estimator"].items():
        assert ec.same_bits(v, again["estimator"][k]), k


def test_a_callers_stream_gives_the_bits_of_the_engines_own():
    import torch
    own = fly_estimated(afa, n=16, seconds=0.6, seed=5, rows=4, cols=6, start_planning=0.3)
    S = torch.cuda.Stream()
    theirs = fly_estimated(afa, n=16, seconds=0.6, seed=5, rows=4, cols=6, start_planning=0.3, stream=S.cuda_stream)
    torch.cuda.synchronize()
    assert own["found"].size >= 3 and own["found"].max() > 0
    np.testing.assert_array_equal(own["pos"], theirs["pos"])
    assert ec.same_bits(own["pred"], theirs["pred"]) and ec.same_bits(own["last_sent"], theirs["last_sent"])
    for k, v in own["estimator"].items():
        assert ec.same_bits(v, theirs["estimator"][k]), k


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    L = afa.library()
    cfg = afa.estimator_default_config()
    h = C.c_void_p()
    e, w_hover = make_engine(N, afa.AFE_F32)
    _stand(e, w_hover, 8)
    short = afa.EstimatorConfig.from_buffer_copy(bytes(cfg))
    short.struct_bytes = C.sizeof(afa.EstimatorConfig) - 8
    assert L.afe_estimator_create(e.handle, C.byref(short), C.byref(h)) == INVALID_ARG
    assert L.afe_estimator_create(e.handle, None, C.byref(h)) == INVALID_ARG
    assert L.afe_estimator_create(e.handle, C.byref(cfg), None) == INVALID_ARG
    many = afa.estimator_default_config()                        # more than 16 slots
    many.max_measure_gap_us = 50000
    assert L.afe_estimator_create(e.handle, C.byref(many), C.byref(h)) == 0 and L.afe_estimator_destroy(h) == 0      # 16
    many.max_measure_gap_us = 55000
    assert L.afe_estimator_create(e.handle, C.byref(many), C.byref(h)) == OUT_OF_RANGE                               # 17
    many.max_measure_gap_us, many.offboard_period_us = 10000, 0
    assert L.afe_estimator_create(e.handle, C.byref(many), C.byref(h)) == OUT_OF_RANGE
    est = afa.Estimator(e)
    f = afa.Follower(e)
    other, _ = make_engine(N, afa.AFE_F32)
    eh = est._h
    d13, d6, d3 = np.zeros((13, N)), np.zeros((6, N)), np.zeros((3, N))
    try:
        # all arrays NULL
        assert L.afe_estimator_get_state(eh, 0, N, None, None, None, None, None, None) == INVALID_ARG
        assert L.afe_estimator_get_prediction(eh, 0, N, None) == INVALID_ARG
        assert L.afe_estimator_announce(eh, 0, N, None, d3.ctypes.data) == INVALID_ARG
        assert L.afe_estimator_announce(eh, 0, N, d3.ctypes.data, None) == INVALID_ARG
        assert L.afe_estimator_predict(eh, float("nan")) == INVALID_ARG
        # ranges: negative, beyond the end, and sums that wrap
        big = 2 ** 63 - 1
        for first, count, want in ((-1, 1, INVALID_ARG), (0, -1, INVALID_ARG), (0, N + 1, OUT_OF_RANGE), (N + 1, 0, OUT_OF_RANGE),
                                   (N, 1, OUT_OF_RANGE), (big, big, OUT_OF_RANGE), (2, big, OUT_OF_RANGE)):
            assert L.afe_estimator_get_state(eh, first, count, d13.ctypes.data, d6.ctypes.data, None, None, None, None) == want, (first, count)
            assert L.afe_estimator_get_prediction(eh, first, count, d13.ctypes.data) == want, (first, count)
            assert L.afe_estimator_announce(eh, first, count, d3.ctypes.data, d3.ctypes.data) == want, (first, count)
            assert L.afe_estimator_reset(eh, first, count) == want, (first, count)
        assert est.info()["n_messages"] == 0
        # no prediction yet
        assert L.afe_estimator_get_prediction(eh, 0, N, d13.ctypes.data) == NOT_CONFIGURED
        f.attach_estimator(est)
        assert L.afe_follower_tick(f._h, None) == NOT_CONFIGURED
        assert L.afe_follower_planner_inputs(f._h, d3.ctypes.data, None, None, None) == NOT_CONFIGURED
        # a stale prediction: stamped before the engine moved on
        e.step(1000, 5)
        est.measure()
        est.predict()
        f.tick()
        assert f.info()["n_ticks"] == 1 and est.info()["n_messages"] == 1
        e.step(1000, 10)
        assert L.afe_follower_tick(f._h, None) == NOT_CONFIGURED
        assert L.afe_follower_plan(f._h, C.byref(afa.planner_default_config(64, 48, 10.0 / 256.0, 32.0, 0.116, 0.174, 0.5)), 1,
                                   np.zeros(4).ctypes.data, 1, None, None, None, None) == NOT_CONFIGURED
        assert f.info()["n_ticks"] == 1 and est.info()["n_messages"] == 1
        est.predict()
        f.tick()
        # an activation time that does not increase: a second announce at the same afe_time_us, from the host and from a tick
        assert L.afe_estimator_announce(eh, 0, N, d3.ctypes.data, d3.ctypes.data) == OUT_OF_RANGE
        assert L.afe_follower_tick(f._h, None) == OUT_OF_RANGE
        assert f.info()["n_ticks"] == 2 and est.info()["n_messages"] == 2
        # an estimator of another engine
        stranger = afa.Estimator(other)
        assert L.afe_follower_attach_estimator(f._h, stranger._h) == INVALID_ARG
        stranger.close()
        assert L.afe_follower_attach_estimator(None, eh) == INVALID_ARG
        f.attach_estimator(None)
        # an overwrite of a slot that is still needed: announces 10 ms apart with no measure call in between
        slots = est.info()["slots"]
        for k in range(slots - 2):
            e.step(1000, 10)
            est.announce(d3, d3)
        assert est.info()["n_messages"] == slots
        e.step(1000, 10)
        assert L.afe_estimator_announce(eh, 0, N, d3.ctypes.data, d3.ctypes.data) == OUT_OF_RANGE
        est.measure()
        assert L.afe_estimator_announce(eh, 0, N, d3.ctypes.data, d3.ctypes.data) == OUT_OF_RANGE      # need is the call before the last
        est.measure()
        est.announce(d3, d3)
        assert est.info()["n_messages"] == slots and est.info()["error"] == 0
        assert np.isfinite(est.state()["est"]).all()
    finally:
        f.close()
        est.close()
        other.close()
        e.close()
    assert L.afe_estimator_destroy(None) == INVALID_ARG


def test_an_estimator_on_a_host_visible_engine_is_refused():
    e = afa.Ensemble(N, precision=afa.AFE_F32, host_visible=True)
    e.set_type_table([afa.params_from_type(5)])
    h = C.c_void_p()
    try:
        assert afa.library().afe_estimator_create(e.handle, C.byref(afa.estimator_default_config()), C.byref(h)) == INVALID_ARG
    finally:
        e.close()


def test_a_failed_engine_refuses_the_estimator():
    """as tests/test_gpu_follower.py's: an engine whose resident grid has reported a failure (forced in the -DAFE_DEV_HOOKS
    build) refuses every estimator call that would touch it, naming that failure; requests for nothing are still answered"""
    from tests.test_gpu_fault_paths import ROOT, _child
    code = r'''
import ctypes as C, importlib, sys, numpy as np
sys.path.insert(0, %r)
from tests.test_gpu_persistent import make
afa = importlib.import_module("agri-fly_amd")
b, d = make(20000, afa.AFE_F32, True, logic=True)
est = afa.Estimator(b)
b.step(1000, 5)
try:
    b.get_state()
    raise SystemExit("the park's timeout was not reported")
except afa.AfeError as ex:
    assert "still running" in str(ex), str(ex)
z3 = np.zeros((3, b.n))
calls = [("measure", est.measure), ("measure, counted", lambda: est.measure(True)), ("predict", est.predict), ("state", est.state),
         ("announce", lambda: est.announce(z3, z3)), ("reset", est.reset), ("create", lambda: afa.Estimator(b))]
for name, call in calls:
    try:
        call()
        raise SystemExit("a failed engine accepted " + name)
    except afa.AfeError as ex:
        assert ex.status == 3, (name, ex.status)
assert "still running" in afa.library().afe_last_error(b.handle).decode()
L = afa.library()
assert L.afe_estimator_reset(est._h, 0, 0) == 0
assert L.afe_estimator_get_state(est._h, b.n, 0, z3.ctypes.data, None, None, None, None, None) == 0
assert est.info()["n_measures"] == 0 and est.info()["n_messages"] == 0
est.close()
b.close()
print("ok")
''' % ROOT
    out, secs = _child(code, "park_timeout")
    assert out.returncode == 0 and "ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
