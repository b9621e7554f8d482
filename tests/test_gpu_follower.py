"""The trajectory follower on the device (include/agrifly_engine.h, "trajectory follower") against its numpy
specification (tests/follower_checker.py).  The judging rule: all arithmetic outside sinf, cosf, asinf, acosf and acos
is IEEE and uncontracted on both sides, so with the device's own values of those five (afe_follower_selftest_math) the
checker equals the device BIT FOR BIT in every field; with glibc's values only their last bits differ, and the sent
commands are then equal or one radio code (35 / 32768) apart, in at most 1 % of the values.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

from tests import follower_checker as fc
from tests.follower_flight import fly_follower
from tests import scenarios
from tests.scenarios import afa

pytestmark = pytest.mark.gpu

N = 130                      # two full waves and two lanes
FAR = (100, 30, 4000.0)      # on the fp32 engine this group stands 4 km out: the anchors matter
INVALID_ARG, HIP, OUT_OF_RANGE, NOT_CONFIGURED = 1, 3, 4, 5
PRECISIONS = [pytest.param(afa.AFE_F32, id="f32"), pytest.param(afa.AFE_F64, id="f64")]


def make_engine(n, precision, noise=False):
    params = afa.params_from_type(5)
    e = afa.Ensemble(n, precision=precision)
    e.set_type_table([params])
    if noise:
        e.set_imu_noise(True, 0.1, 0.2, afa.AFE_SEED_DECORRELATED)
    e.set_rates_logic([afa.rates_logic_params_from_type(5)])
    return e, afa.scenarios.hover_speed(params)


def stand(e, w_hover, seed, far=None):
    """make_state's vehicles into the engine; -> the state as the engine reports it"""
    pos, vel, att = fc.make_state(e.n, seed, far)
    e.set_state(pos, vel, att, np.zeros((3, e.n)), np.full((4, e.n), w_hover))
    return e.get_state()


def put_plans(f, plans):
    f.set_plans(**{k: plans[k] for k in ("planned", "coeffs", "tf", "t_plan_us", "traj_att", "offset", "grav")})
    f.set_hold(plans["hold"])
    f.set_goal(plans["goal"])


@pytest.fixture(scope="module")
def dmath():
    return fc.device_math(afa)


@pytest.fixture(scope="module", params=PRECISIONS)
def scene(request, dmath):
    """One tick on injected plans that cover the branch list, then the planner's inputs: everything downloaded once,
    the checker's answers with the device's and with glibc's functions beside it."""
    precision = request.param
    e, w_hover = make_engine(N, precision)
    stand(e, w_hover, 5)
    e.step(1000, 200)                                        # the plans need a past to have been planned in
    now = e.time_us
    st = stand(e, w_hover, 5, FAR if precision == afa.AFE_F32 else None)
    f = afa.Follower(e)
    cfg = fc.config_from(f.cfg)
    plans = fc.make_plans(st["pos"], 5, now)
    put_plans(f, plans)
    back = f.get_plans()
    inputs0 = f.planner_inputs()                             # previous_thrust still the hover thrust
    n_tracking = f.tick(count_tracking=True)
    got = dict(ref14=f.get_reference(), now=now, n_tracking=n_tracking, info=f.info(), inputs0=inputs0, inputs1=f.planner_inputs(),
               rates=e.get_rates_commands(), plans_back=back)
    got["computed"], got["sent"] = f.get_command()
    info = {}
    want = fc.tick(st["pos"], st["vel"], st["att"], plans, cfg, now, dmath, info)
    glibc = fc.tick(st["pos"], st["vel"], st["att"], plans, cfg, now, fc.glibc_math)
    f.close()
    e.close()
    return dict(precision=precision, st=st, plans=plans, cfg=cfg, got=got, want=want, glibc=glibc, info=info)


def test_device_functions_are_the_library_functions_to_an_ulp_or_two(dmath):
    """not the judging rule, its premise: the device's five functions are ordinary implementations of them"""
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, 4096).astype(np.float32)
    for op, scale in ((0, 3.2), (1, 3.2), (2, 1.0), (3, 1.0)):
        xs = (x * np.float32(scale)).astype(np.float32)
        d, g = dmath(op, xs), fc.glibc_math(op, xs)
        assert d.dtype == np.float32 and np.abs(d.astype(np.float64) - g).max() <= 4 * np.spacing(np.float32(3.2))
    xd = rng.uniform(-1, 1, 4096)
    assert np.abs(dmath(4, xd) - fc.glibc_math(4, xd)).max() <= 4 * np.spacing(np.pi)
    assert fc.same_bits(dmath(3, x), dmath(3, x.copy()))


def test_set_plans_reads_back(scene):
    for k, v in scene["got"]["plans_back"].items():
        assert fc.same_bits(v, scene["plans"][k]), k


def test_the_inputs_reach_every_branch_on_the_engine(scene):
    counts = {k: int(np.count_nonzero(scene["info"][k])) for k in fc.BRANCHES + ("theta_small",)}
    print(counts)
    for k, v in counts.items():
        assert v > 0, "no vehicle takes the branch %r: %r" % (k, counts)
    if scene["precision"] == afa.AFE_F32:
        first, count, metres = FAR
        assert (scene["st"]["pos"][0, first:first + count] > metres - 10).all()


def test_reference_is_bit_identical(scene):
    got, want = scene["got"]["ref14"], scene["want"]["ref14"]
    names = ["pos"] * 3 + ["vel"] * 3 + ["acc"] * 3 + ["thrust"] + ["rates"] * 3 + ["running"]
    for k in range(14):
        bad = np.flatnonzero(got[k].view(np.uint64) != want[k].view(np.uint64))
        assert bad.size == 0, (names[k], k, bad[:8], got[k][bad[:8]], want[k][bad[:8]])
    assert scene["got"]["n_tracking"] == int(want[13].sum())
    assert scene["got"]["info"] == {"n_vehicles": N, "slots": 5, "n_ticks": 1, "in_flight": 1}


def test_command_is_bit_identical(scene):
    got, want = scene["got"]["computed"], scene["want"]["computed"]
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (bad[:8], [(got[tuple(b)], want[tuple(b)]) for b in bad[:8]])
    assert fc.same_bits(scene["got"]["sent"], scene["want"]["sent"])
    # nothing has been delivered yet: 30 ms of delay, one tick
    thrust, w, have = scene["got"]["rates"]
    assert not have.any() and not thrust.any() and not w.any()


def test_sent_is_the_host_codec_of_computed(scene):
    computed, sent = scene["got"]["computed"], scene["got"]["sent"]
    assert (computed >= 35).any() and (computed <= -35).any()
    for i in range(N):
        m = afa.radio_decode(afa.radio_create_rates_command(0, computed[0, i], computed[1:4, i]))
        host = np.array([m.floats[k] for k in range(4)], np.float32)
        assert fc.same_bits(host, sent[:, i]), (i, host, sent[:, i])


def test_against_glibc_at_most_one_code_in_at_most_one_percent(scene):
    dist = fc.code_distance(scene["got"]["sent"], scene["glibc"]["sent"])
    print("device against glibc: %d of %d codes differ, largest distance %d; computed differs by up to %.3g"
          % (np.count_nonzero(dist), dist.size, dist.max(),
             np.nanmax(np.abs(scene["got"]["computed"].astype(np.float64) - scene["glibc"]["computed"]))))
    scenarios.MEASUREMENTS["follower_device_vs_glibc_codes[%s]" % ("f32" if scene["precision"] == afa.AFE_F32 else "f64")] = {
        "differing": int(np.count_nonzero(dist)), "of": int(dist.size), "largest": int(dist.max())}
    assert dist.max() <= 1
    assert np.count_nonzero(dist) <= 0.01 * dist.size


def test_planner_inputs_are_bit_identical(scene):
    st, plans, cfg = scene["st"], scene["plans"], scene["cfg"]
    hover = np.full(N, cfg["hover_thrust"])
    for which, thrust in (("inputs0", hover), ("inputs1", scene["want"]["cmd_thrust"])):     # before and after the tick changed it
        want = fc.planner_inputs(st["pos"], st["vel"], st["att"], thrust, plans["goal"], cfg["mount"])
        for k in ("vel0", "acc0", "grav", "cost_vec"):
            assert fc.same_bits(scene["got"][which][k], want[k]), (which, k)
    assert not fc.same_bits(scene["got"]["inputs0"]["acc0"], scene["got"]["inputs1"]["acc0"])


# ---- plan adoption ---------------------------------------------------------------------------------------------------------
W, H, M = 64, 48, 32


def _images(kind, n, rng):
    clear, wall = np.full((H, W), 255, np.uint16), np.full((H, W), 25, np.uint16)      # 10 m / 256 per count: 25 counts = 1 m
    if kind == "clear":
        return np.tile(clear, (n, 1, 1))
    if kind == "wall":
        return np.tile(wall, (n, 1, 1))
    imgs = np.empty((n, H, W), np.uint16)
    for i in range(n):
        if i % 3 == 0:
            imgs[i] = clear
        elif i % 3 == 1:
            imgs[i] = wall
        else:                                                # a wall with a window somewhere
            imgs[i] = wall
            x0, y0 = rng.integers(0, W - 24), rng.integers(0, H - 20)
            imgs[i, y0:y0 + 20, x0:x0 + 24] = 255
    return imgs


@pytest.mark.parametrize("precision", PRECISIONS)
def test_plan_adopts_what_the_planner_returns(precision):
    rng = np.random.default_rng(3)
    e, w_hover = make_engine(N, precision)
    e.step(1000, 30)
    far = FAR if precision == afa.AFE_F32 else None
    pos, vel, att = fc.make_state(N, 9, far)
    att = afa.scenarios.random_attitudes(rng, N, max_tilt_deg=15.0)
    e.set_state(pos, vel * 0.3, att, np.zeros((3, N)), np.full((4, N), w_hover))
    st = e.get_state()
    f = afa.Follower(e)
    goal = st["pos"] + np.stack([np.full(N, 20.0), rng.uniform(-3, 3, N), np.zeros(N)])
    f.set_goal(goal)
    cfgf = fc.config_from(f.cfg)
    cam = afa.camera_default(W, H)
    cfg = afa.planner_default_config(W, H, cam.depth_scale, cam.focal_length, 0.116, 0.174, 0.5)
    cfg.cost_type = 1
    samples = afa.planner_samples(0, W, H, M)
    buf = afa.DeviceBuffer(N * H * W * 2)
    fields = ("planned", "coeffs", "tf", "t_plan_us", "traj_att", "offset", "grav")
    try:
        stored = f.get_plans()
        assert not stored["planned"].any()
        total_found = 0
        for step, kind in enumerate(("wall", "mixture", "clear", "wall", "wall")):
            e.step(1000, 10)
            now = e.time_us
            st = e.get_state()
            buf.upload(_images(kind, N, rng))
            inp = f.planner_inputs()
            want_in = fc.planner_inputs(st["pos"], st["vel"], st["att"], np.full(N, cfgf["hover_thrust"]), goal, cfgf["mount"])
            for k in ("vel0", "acc0", "grav", "cost_vec"):
                assert fc.same_bits(inp[k], want_in[k]), (kind, k)
            ref_out, ref_flags, _ = afa.rappids_plan(cfg, buf, inp["vel0"], inp["acc0"], inp["grav"], samples, cost_vec=inp["cost_vec"],
                                                     want_flags=True)
            want = afa.plans_as_array(ref_out)
            n_found, out, flags, _ = f.plan(cfg, buf, samples, want_out=True, want_flags=True)
            got = afa.plans_as_array(out)
            for name in want.dtype.names:                                       # what afe_rappids_plan_device returns, to the bit
                assert fc.same_bits(got[name], want[name]), (kind, name)
            assert np.array_equal(flags, ref_flags)
            found = want["found"].astype(bool)
            assert n_found == int(found.sum())
            n_quiet, _, _, _ = f.plan(cfg, buf, samples)                        # nothing downloaded but the count: the same plans again
            assert n_quiet == n_found
            after = f.get_plans()
            print("%s: %d of %d found" % (kind, n_found, N))
            if kind == "mixture":
                assert 0 < n_found < N
            expect = {k: stored[k].copy() for k in fields}
            expect["planned"][found] = 1
            expect["coeffs"][:, found] = want["coeffs"][found].reshape(-1, 18).T
            expect["tf"][found] = want["tf"][found]
            expect["t_plan_us"][found] = now
            expect["traj_att"][:, found] = want_in["cam"][:, found]
            expect["offset"][:, found] = st["pos"][:, found]
            expect["grav"][:, found] = want_in["grav"][:, found]
            for k in fields:
                assert fc.same_bits(after[k], expect[k]), (kind, step, k)       # the others keep what they had
            stored = after
            total_found += n_found
        assert stored["planned"].any() and total_found > 0
    finally:
        buf.close()
        f.close()
        e.close()


# ---- delay line -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delay_us", [0, 25000, 30000])
def test_delay_line_delivers_what_the_checkers_queue_delivers(delay_us, dmath):
    e, w_hover = make_engine(N, afa.AFE_F32, noise=True)
    st = stand(e, w_hover, 21)
    e.set_state(att=afa.scenarios.random_attitudes(np.random.default_rng(1), N, max_tilt_deg=10.0), vel=st["vel"] * 0.2)
    cfg_c = afa.follower_default_config(5)
    cfg_c.delay_us = delay_us
    f = afa.Follower(e, cfg=cfg_c)
    cfg = fc.config_from(cfg_c)
    hold = e.get_state()["pos"]
    plans = None
    line = fc.DelayLine(delay_us)
    held = (np.zeros(N, np.float32), np.zeros((3, N), np.float32), np.zeros(N, np.uint8))
    try:
        assert f.info()["slots"] == fc.ring_slots(10000, delay_us)
        for tick in range(1, 9):
            e.step(1000, 10)
            now = e.time_us
            st = e.get_state()
            if tick in (1, 4, 6):                            # a changing plan
                plans = fc.make_plans(st["pos"], 30 + tick, max(now, 100000))
                plans["t_plan_us"] = np.minimum(plans["t_plan_us"], np.uint64(now))
                plans["hold"] = hold
                put_plans(f, plans)
            f.tick()
            want = fc.tick(st["pos"], st["vel"], st["att"], plans, cfg, now, dmath)
            msg = line.tick(now, want["sent"])
            if msg is not None:
                held = (msg[0], msg[1:4], np.ones(N, np.uint8))
            thrust, w, have = e.get_rates_commands()
            assert fc.same_bits(thrust, held[0]) and fc.same_bits(w, held[1]) and np.array_equal(have, held[2]), (delay_us, tick)
            assert fc.same_bits(f.get_command()[1], want["sent"]), (delay_us, tick)
            assert f.info()["in_flight"] == len(line.queue) and f.info()["n_ticks"] == tick
        assert held[2].all()
    finally:
        f.close()
        e.close()


def test_a_delay_that_needs_more_than_sixteen_slots_is_refused_at_create():
    e, _ = make_engine(N, afa.AFE_F32)
    cfg = afa.follower_default_config(5)
    h = C.c_void_p()
    L = afa.library()
    try:
        cfg.delay_us = 149999
        assert L.afe_follower_create(e.handle, C.byref(cfg), C.byref(h)) == 0
        assert L.afe_follower_destroy(h) == 0
        cfg.delay_us = 150000
        assert L.afe_follower_create(e.handle, C.byref(cfg), C.byref(h)) == OUT_OF_RANGE
        cfg.delay_us, cfg.period_us = 30000, 0
        assert L.afe_follower_create(e.handle, C.byref(cfg), C.byref(h)) == OUT_OF_RANGE
    finally:
        e.close()


def test_ticks_closer_together_than_the_period_fill_the_ring():
    e, w_hover = make_engine(N, afa.AFE_F32)
    stand(e, w_hover, 2)
    f = afa.Follower(e)
    try:
        for _ in range(5):                                   # no step in between: five messages due at the same time
            f.tick()
        with pytest.raises(afa.AfeError) as ei:
            f.tick()
        assert ei.value.status == OUT_OF_RANGE
        assert f.info()["in_flight"] == 5 and f.info()["n_ticks"] == 5
        e.step(1000, 30)
        f.tick()                                             # all five delivered, one sent
        assert f.info()["in_flight"] == 1
    finally:
        f.close()
        e.close()


# ---- delivery is afe_set_rates_commands -------------------------------------------------------------------------------------
def _everything(e):
    return dict(e.get_state(), rng=e.get_rng_state(), cmds=e.get_motor_cmds(), **dict(zip(("gyro", "acc"), e.get_imu())))


@pytest.mark.parametrize("mode", [pytest.param(afa.AFE_STEP_LAUNCH, id="launches"), pytest.param(afa.AFE_STEP_RESIDENT, id="resident")])
def test_delivery_is_set_rates_commands(mode):
    """Engine A flies with the follower (10 ms of delay: five deliveries in 60 steps); engine B is handed A's sent commands
    through afe_set_rates_commands at the same ticks.  After 60 steps the two hold the same bits."""
    engines = []
    for _ in range(2):
        e, w_hover = make_engine(N, afa.AFE_F32, noise=True)
        e.set_step_mode(mode)
        pos, vel, _ = fc.make_state(N, 17)
        att = afa.scenarios.random_attitudes(np.random.default_rng(4), N, max_tilt_deg=10.0)
        e.set_state(pos, vel * 0.2, att, np.zeros((3, N)), np.full((4, N), w_hover))
        e.set_rates_commands(np.full(N, 9.81, np.float32), np.zeros((3, N), np.float32))
        engines.append(e)
    a, b = engines
    cfg = afa.follower_default_config(5)
    cfg.delay_us = 10000
    f = afa.Follower(a, cfg=cfg)
    line = fc.DelayLine(cfg.delay_us)
    try:
        delivered = 0
        for tick in range(1, 7):
            a.step(1000, 10)
            b.step(1000, 10)
            f.tick()
            msg = line.tick(a.time_us, f.get_command()[1])
            if msg is not None:
                b.set_rates_commands(msg[0], msg[1:4])
                delivered += 1
        assert delivered == 5 and a.time_us == b.time_us == 60000
        ea, eb = _everything(a), _everything(b)
        for k in ea:
            assert fc.same_bits(ea[k], eb[k]), k
        ra, rb = a.get_rates_commands(), b.get_rates_commands()
        assert all(fc.same_bits(x, y) for x, y in zip(ra, rb))
        assert np.abs(ea["ang_vel"]).max() > 0.01            # they did something
    finally:
        f.close()
        a.close()
        b.close()


# ---- flights ---------------------------------------------------------------------------------------------------------------
def test_teacher_forced_flight_is_bit_identical(dmath):
    """1 s of the follower loop in the 6 x 10 orchard, 48 vehicles: at every tick the downloaded state and the follower's
    stored plans go through the checker with the device's functions -- the computed command equals it, all ticks, all
    vehicles."""
    seen = {"ticks": 0, "planned": 0, "hold": None, "cfg": None}

    def before(tick, now, e, fol):
        if seen["hold"] is None:
            seen["cfg"] = fc.config_from(fol.cfg)
        seen["st"], seen["plans"] = e.get_state(), fol.get_plans()

    def after(tick, now, e, fol):
        st, plans = seen["st"], dict(seen["plans"])
        if seen["hold"] is None:
            seen["hold"] = fol.get_reference()[0:3].copy()           # nobody has a plan at the first tick: the hold points
            assert not plans["planned"].any()
        plans["hold"] = seen["hold"]
        want = fc.tick(st["pos"], st["vel"], st["att"], plans, seen["cfg"], now, dmath)
        computed, sent = fol.get_command()
        assert fc.same_bits(computed, want["computed"]), tick
        assert fc.same_bits(sent, want["sent"]), tick
        assert fc.same_bits(fol.get_reference(), want["ref14"]), tick
        seen["ticks"] += 1
        seen["planned"] = int(plans["planned"].sum())

    log = fly_follower(afa, n=48, seconds=1.0, seed=0, before_tick=before, after_tick=after, log_every=0)
    assert seen["ticks"] == 100 and seen["planned"] > 24 and log["found"].mean() > 0.5
    # the hold points are where the vehicles stood when the follower was made
    assert np.abs(seen["hold"] - log["pos0"]).max() < 1e-6


def test_follower_flight_is_reproducible():
    a = fly_follower(afa, n=16, seconds=2.5, seed=3, rows=4, cols=6)
    b = fly_follower(afa, n=16, seconds=2.5, seed=3, rows=4, cols=6)
    np.testing.assert_array_equal(a["pos"], b["pos"])
    np.testing.assert_array_equal(a["found"], b["found"])
    assert fc.same_bits(a["last_sent"], b["last_sent"])


def test_follower_flies_through_the_orchard_without_touching_a_tree():
    """tests/test_gpu_orchard_flight.py's flight and its assertions, as they stand there, for the follower loop"""
    log = fly_follower(afa, n=48, seconds=8.0, seed=0)
    pos = log["pos"]
    assert np.isfinite(pos).all() and np.isfinite(log["vel"]).all()
    advance = pos[-1, 0] - log["pos0"][0]
    six = np.searchsorted(log["t"], 6.0)
    print("\nfollower flight: %d vehicles, x advance %.1f..%.1f m in 8 s (%.1f m at least after 6 s), min trunk clearance %.3f m, "
          "min canopy level %.2f, plans found %.0f %%, planner %.1f ms / render %.2f ms per frame"
          % (pos.shape[2], advance.min(), advance.max(), (pos[six, 0] - log["pos0"][0]).min(), log["trunk"].min(), log["canopy"].min(),
             100 * log["found"].mean(), log["plan_ms"].mean(), log["render_ms"].mean()))
    assert advance.min() > 10.0                       # every vehicle made its way east
    assert pos[:, 2].min() > 0.1                      # nobody on the ground
    assert log["trunk"].min() > 0.116                 # physicalVehicleRadius = 2 * armLength (main.cpp:167)
    assert log["canopy"].min() > 1.0                  # outside every canopy ellipsoid
    assert log["found"].mean() > 0.9 and log["planned"].all()
    assert np.sqrt((log["vel"] ** 2).sum(1)).max() < 5.0   # DepthImagePlanner's velocity limit (DIP.cpp:48)


def test_a_callers_stream_gives_the_bits_of_the_engines_own():
    """plans and ticks on a non-blocking stream set with afe_set_stream: the planner launches on the null stream, which
    such a stream does not wait for, so the follower has to order the two itself"""
    import torch
    own = fly_follower(afa, n=16, seconds=0.6, seed=5, rows=4, cols=6, start_planning=0.3)
    S = torch.cuda.Stream()
    theirs = fly_follower(afa, n=16, seconds=0.6, seed=5, rows=4, cols=6, start_planning=0.3, stream=S.cuda_stream)
    torch.cuda.synchronize()
    assert own["found"].size >= 3 and own["found"].max() > 0
    np.testing.assert_array_equal(own["pos"], theirs["pos"])
    np.testing.assert_array_equal(own["found"], theirs["found"])
    assert fc.same_bits(own["last_sent"], theirs["last_sent"])


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals():
    L = afa.library()
    cfg = afa.follower_default_config(5)
    h = C.c_void_p()
    bare = afa.Ensemble(N, precision=afa.AFE_F32)            # no rates logic
    bare.set_type_table([afa.params_from_type(5)])
    try:
        assert L.afe_follower_create(bare.handle, C.byref(cfg), C.byref(h)) == NOT_CONFIGURED
        assert L.afe_get_rates_commands(bare.handle, 0, 1, np.zeros(1, np.float32).ctypes.data, None, None) == NOT_CONFIGURED
    finally:
        bare.close()
    e, w_hover = make_engine(N, afa.AFE_F32)
    stand(e, w_hover, 8)
    short = afa.FollowerConfig.from_buffer_copy(bytes(cfg))
    short.struct_bytes = C.sizeof(afa.FollowerConfig) - 8
    assert L.afe_follower_create(e.handle, C.byref(short), C.byref(h)) == INVALID_ARG
    assert L.afe_follower_create(e.handle, None, C.byref(h)) == INVALID_ARG
    assert L.afe_follower_create(e.handle, C.byref(cfg), None) == INVALID_ARG
    f = afa.Follower(e)
    fh = f._h
    d3, d14, f4 = np.zeros((3, N)), np.zeros((14, N)), np.zeros((4, N), np.float32)
    try:
        # NULL arrays
        assert L.afe_follower_set_hold(fh, 0, N, None) == INVALID_ARG
        assert L.afe_follower_set_goal(fh, 0, N, None) == INVALID_ARG
        assert L.afe_follower_set_plans(fh, 0, N, None, None, None, None, None, None, None) == INVALID_ARG
        assert L.afe_follower_get_plans(fh, 0, N, None, None, None, None, None, None, None) == INVALID_ARG
        assert L.afe_follower_get_reference(fh, 0, N, None) == INVALID_ARG
        assert L.afe_follower_get_command(fh, 0, N, None, None) == INVALID_ARG
        assert L.afe_follower_planner_inputs(fh, None, None, None, None) == INVALID_ARG
        assert L.afe_follower_plan(fh, None, None, None, 0, None, None, None, None) == INVALID_ARG
        assert L.afe_get_rates_commands(e.handle, 0, N, None, None, None) == INVALID_ARG
        # ranges: negative, beyond the end, and sums that wrap
        big = 2 ** 63 - 1
        for first, count, want in ((-1, 1, INVALID_ARG), (0, -1, INVALID_ARG), (0, N + 1, OUT_OF_RANGE), (N + 1, 0, OUT_OF_RANGE),
                                   (N, 1, OUT_OF_RANGE), (big, big, OUT_OF_RANGE), (2, big, OUT_OF_RANGE)):
            assert L.afe_follower_set_hold(fh, first, count, d3.ctypes.data) == want, (first, count)
            assert L.afe_follower_get_reference(fh, first, count, d14.ctypes.data) == want, (first, count)
            assert L.afe_follower_get_command(fh, first, count, f4.ctypes.data, None) == want, (first, count)
            assert L.afe_follower_set_plans(fh, first, count, None, None, d3.ctypes.data, None, None, None, None) == want, (first, count)
        for first, count in ((-1, 1), (0, N + 1), (big, big)):
            assert L.afe_get_rates_commands(e.handle, first, count, f4.ctypes.data, None, None) == OUT_OF_RANGE
        # an empty range is answered before the engine is touched: a resident grid stays where it is
        e.set_step_mode(afa.AFE_STEP_RESIDENT)
        e.step(1000, 5)
        running = C.c_int(0)
        assert L.afe_persistent_running(e.handle, C.byref(running)) == 0
        was_running = running.value
        for first in (0, N):
            assert L.afe_follower_set_hold(fh, first, 0, d3.ctypes.data) == 0
            assert L.afe_follower_get_reference(fh, first, 0, d14.ctypes.data) == 0
            assert L.afe_follower_get_command(fh, first, 0, f4.ctypes.data, None) == 0
            assert L.afe_follower_get_plans(fh, first, 0, None, None, d3.ctypes.data, None, None, None, None) == 0
        assert L.afe_persistent_running(e.handle, C.byref(running)) == 0 and running.value == was_running
        print("resident grid running across the empty requests:", was_running)
        f.tick()                                             # ... and a tick goes through the engine's gate
        # the rates logic switched off under a live follower
        e.set_rates_logic(None)
        assert L.afe_follower_tick(fh, None) == NOT_CONFIGURED
    finally:
        f.close()
        e.close()
    assert L.afe_follower_destroy(None) == INVALID_ARG


def test_a_follower_on_a_host_visible_engine_is_refused():
    e = afa.Ensemble(N, precision=afa.AFE_F32, host_visible=True)
    e.set_type_table([afa.params_from_type(5)])
    e.set_rates_logic([afa.rates_logic_params_from_type(5)])
    h = C.c_void_p()
    try:
        assert afa.library().afe_follower_create(e.handle, C.byref(afa.follower_default_config(5)), C.byref(h)) == INVALID_ARG
    finally:
        e.close()


def test_a_failed_engine_refuses_the_follower():
    """An engine whose resident grid has reported a failure (forced in the -DAFE_DEV_HOOKS build, as
    tests/test_gpu_fault_paths.py does) refuses every follower call that would touch it, naming that failure; requests
    for nothing are still answered."""
    from tests.test_gpu_fault_paths import ROOT, _child
    code = r'''
import ctypes as C, importlib, sys, numpy as np
sys.path.insert(0, %r)
from tests.test_gpu_persistent import make
afa = importlib.import_module("agri-fly_amd")
b, d = make(20000, afa.AFE_F32, True, logic=True)
f = afa.Follower(b)
b.step(1000, 5)
try:
    b.get_state()
    raise SystemExit("the park's timeout was not reported")
except afa.AfeError as ex:
    assert "still running" in str(ex), str(ex)
z3 = np.zeros((3, b.n))
calls = [("tick", f.tick), ("tick, counted", lambda: f.tick(True)), ("get_reference", f.get_reference), ("get_command", f.get_command),
         ("get_plans", f.get_plans), ("set_hold", lambda: f.set_hold(z3)), ("set_goal", lambda: f.set_goal(z3)),
         ("set_plans", lambda: f.set_plans(tf=np.zeros(b.n))), ("planner_inputs", f.planner_inputs), ("create", lambda: afa.Follower(b)),
         ("get_rates_commands", b.get_rates_commands)]
for name, call in calls:
    try:
        call()
        raise SystemExit("a failed engine accepted " + name)
    except afa.AfeError as ex:
        assert ex.status == 3, (name, ex.status)
assert "still running" in afa.library().afe_last_error(b.handle).decode()
L = afa.library()
assert L.afe_follower_set_hold(f._h, 0, 0, z3.ctypes.data) == 0
assert L.afe_follower_get_reference(f._h, b.n, 0, z3.ctypes.data) == 0
assert f.info()["n_ticks"] == 0
f.close()
b.close()
print("ok")
''' % ROOT
    out, secs = _child(code, "park_timeout")
    assert out.returncode == 0 and "ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
