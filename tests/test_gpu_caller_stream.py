"""Caller-owned streams (afe_set_stream): what the header promises a host that makes the engine's work part of its own
stream -- the same bits as on the engine's stream, the host's work and the engine's ordered on the stream with no
synchronisation in between, the library's consumers of the engine's state behind the same stream, switching and destroying
with work still queued, and the refusal of the default stream's reserved handles.  torch provides streams, events and buffers.

How an ordering test is made sharp.  A call that went to another stream than the caller's starts at once; it must then
read something else than the ordered call.  So the caller's stream first gets a DELAY (_delay: a chain of torch matmuls,
calibrated on the device to at least max(20 ms, 10 x the duration of the engine calls under test)), behind it whatever
produces the input, then the consumer -- and the buffers hold a valid STALE input meanwhile, which the test shows (on the
CPU, with the checkers) to give another answer than the fresh one.  Each case runs on four streams (_streams says why).
Held this way, a copy of the library broken on purpose -- afe_pack_positions or afe_stats_update launched on the NULL
stream, the automatic split let loose on a caller's stream -- fails these tests by wrong answers.  A mis-ordered library
gives a wrong answer, never a fault: every buffer holds finite data at all times, every stream and tensor outlives the
work queued on it.  The delays, the step blocks and the stale / fresh differences go to the ledger
(tests.scenarios.MEASUREMENTS: caller_stream_delay_ms, caller_stream_step_block_ms, caller_stream_stale_vs_fresh).
Needs an MI355X."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

from tests import clearance_checker as cck
from tests import stats_checker as sck
from tests.scenarios import FLOORS, MEASUREMENTS, afa, random_ensemble, record_parity

pytestmark = pytest.mark.gpu

scen = afa.scenarios
AFE_F32, AFE_F64 = afa.AFE_F32, afa.AFE_F64
F32_TOL, F64_TOL = 1e-5, 1e-11       # the rollout tolerances of tests/test_gpu_parity.py


# ---- the two helpers -------------------------------------------------------------------------------------------------
_CAL = {}      # the matmul operands, the calibration stream and the measured duration of a chain per repeat count


def _chain(stream, repeats):
    import torch
    if "mats" not in _CAL:
        g = torch.Generator().manual_seed(5)
        a = (torch.rand((2048, 2048), generator=g) - 0.5).cuda()
        b = (torch.rand((2048, 2048), generator=g) - 0.5).cuda()
        c = torch.zeros((2048, 2048), device="cuda")
        torch.mm(a, b, out=c)                       # (the first product loads the BLAS library: not part of any measurement)
        torch.cuda.synchronize()
        _CAL["mats"] = (a, b, c)
    a, b, c = _CAL["mats"]
    with torch.cuda.stream(stream):
        for _ in range(repeats):
            torch.mm(a, b, out=c)


def _chain_ms(repeats):
    """duration of the chain on an idle device, measured once per repeat count with torch events: the shorter of two runs
    (what is wanted is a lower bound of the delay), behind an untimed product that takes the stream's first-use costs"""
    import torch
    key = ("ms", repeats)
    if key not in _CAL:
        if "stream" not in _CAL:
            _CAL["stream"] = torch.cuda.Stream()
            _chain(_CAL["stream"], 1)
        s = _CAL["stream"]
        ms = []
        for _ in range(2):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            _chain(s, repeats)
            e1.record(s)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        _CAL[key] = min(ms)
    return _CAL[key]


_QUEUED = []       # delays queued in the running test: (ledger entry, bound, events round the chain)


def _delay(stream, t_call_ms, what=None):
    """Queues on `stream` a chain of 2048 x 2048 fp32 matmuls that takes at least max(20 ms, 10 x t_call_ms) -- ten times,
    so that a mis-ordered call, which starts at once, has long finished reading when the chain ends.  The repeat count is
    found by doubling on the device (nothing is hard-coded); out of reach within 4096 repeats: the test fails."""
    import torch
    bound = max(20.0, 10.0 * t_call_ms)
    repeats = 1
    while _chain_ms(repeats) < bound:
        repeats *= 2
        if repeats > 4096:
            pytest.fail("no delay of %.1f ms within 4096 matmuls (%.2f ms at 4096)" % (bound, _chain_ms(4096)))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    _chain(stream, repeats)
    e1.record(stream)
    entry = {"delay_ms": _chain_ms(repeats), "repeats": repeats, "t_call_ms": t_call_ms, "bound_ms": bound}
    if what is not None:
        MEASUREMENTS.setdefault("caller_stream_delay_ms", {})[what] = entry
    _QUEUED.append((entry, bound, e0, e1))


@pytest.fixture(autouse=True)
def _delays_as_they_ran():
    """After the test: what each delay took where it ran, into the ledger beside the calibrated figure.  A calibration gone
    wrong (a chain timed with some one-off cost in it) would leave every ordering test here passing and blunt: a delay
    that ran in less than half its bound fails the test."""
    del _QUEUED[:]
    yield
    short = []
    for entry, bound, e0, e1 in _QUEUED:
        e1.synchronize()
        entry["delay_ms_in_the_test"] = e0.elapsed_time(e1)
        if entry["delay_ms_in_the_test"] < 0.5 * bound:
            short.append(entry)
    del _QUEUED[:]
    assert not short, "delays shorter than calibrated: %r" % short


def _timed(stream, fn):
    """duration of fn()'s work on the idle `stream` (torch events round it), and fn's result"""
    import torch
    stream.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    out = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), out


def _differ(what, n_differing):
    """stale and fresh inputs give different answers: shown on the CPU, and ledgered"""
    MEASUREMENTS.setdefault("caller_stream_stale_vs_fresh", {})[what] = int(n_differing)
    assert n_differing > 0, "%s: the stale input gives the fresh input's answer -- the test could not tell" % what


class _Slab:
    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(ptr, False), version=2, strides=None)


def _everything(e):
    st = e.get_state()
    gyro, acc = e.get_imu()
    return dict(st, gyro=gyro, acc=acc, rng=e.get_rng_state(), logic_ticks=e.logic_ticks, time_us=e.time_us)


def _same_bits(got, want, what):
    for k in want:
        assert_array_equal(got[k], want[k], err_msg="%s: %s" % (what, k))


# ---- 1. bits do not depend on the stream -----------------------------------------------------------------------------
BLOCKS = (7, 1, 32)       # 40 steps of 1000 us


def _fly(ens, precision, before=None, after=None):
    """the tick path (logic period 1/500 s, IMU noise of the reference's seed policy), external force on"""
    with ens.to_engine(precision) as e:
        e.set_logic_period(1.0 / 500.0)
        e.set_imu_noise(True, seed_policy=afa.AFE_SEED_REFERENCE)
        for k, steps in enumerate(BLOCKS):
            if before:
                before(e, k)
            e.step(1000, steps)
            if after:
                after(e, k)
        return _everything(e), e.step_kernel_info()[0]      # (the getters wait for the stream the engine is on)


@pytest.mark.parametrize("layout", ["one record", "four types shuffled"])
@pytest.mark.parametrize("precision,tol", [(AFE_F32, F32_TOL), (AFE_F64, F64_TOL)])
def test_bits_do_not_depend_on_the_stream(precision, tol, layout):
    """(a) the engine's stream, one launch per call; (b) a caller's stream; (c) a caller's stream, two parts; (d) a caller's
    stream with the resident grid asked for (it must not start); (e) the resident grid on the engine's stream, then a
    caller's stream under it, then the engine's again.  (b) to (e) equal (a) bit for bit, and (b) is judged by the CPU
    oracle at the tolerances of tests/test_gpu_parity.py."""
    import torch
    uniform = layout == "one record"
    ens = random_ensemble(3000, seed=61, ground_fraction=0.0, **(dict(type_ids=(5,)) if uniform else {}))
    ens.data.pos[2] += 20.0               # (away from the ground: a contact time one ulp apart cannot flip the clamp against the oracle)
    ens.data.ext_torque = None            # the resident grid of (d) and (e) serves ensembles without an external torque
    S = torch.cuda.Stream()
    on_s = S.cuda_stream

    def launch(e, k):
        if k == 0:
            e.set_step_mode(afa.AFE_STEP_LAUNCH)

    def b_before(e, k):
        if k == 0:
            e.set_step_mode(afa.AFE_STEP_LAUNCH)
            e.set_split_stepping(0)
            e.set_stream(on_s)

    def c_before(e, k):
        if k == 0:
            e.set_step_mode(afa.AFE_STEP_LAUNCH)
            e.set_stream(on_s)
            e.set_split_stepping(2)

    def d_before(e, k):
        if k == 0:
            e.set_split_stepping(0)
            e.set_stream(on_s)
            e.set_step_mode(afa.AFE_STEP_PERSISTENT)

    def d_after(e, k):
        assert not e.persistent_running, "a resident grid on a caller's stream (block %d)" % k

    def e_before(e, k):
        if k == 0:
            e.set_split_stepping(0)
            e.set_step_mode(afa.AFE_STEP_PERSISTENT)
        elif k == 1:
            e.set_stream(on_s)
            assert not e.persistent_running, "the grid outlived the engine's stream"
        else:
            e.set_stream(None)

    def e_after(e, k):
        assert e.persistent_running == (uniform and k != 1), "block %d" % k

    a, path = _fly(ens, precision, launch)
    assert path == ("kernel arguments" if uniform else "LDS table")
    assert a["time_us"] == 40000 and a["logic_ticks"] == int(afa.plan_ticks(1.0 / 500.0, 0, 1000, 40)[0].sum())
    b, _ = _fly(ens, precision, b_before)
    _same_bits(b, a, "(b) caller's stream")
    _same_bits(_fly(ens, precision, c_before)[0], a, "(c) caller's stream, two parts")
    _same_bits(_fly(ens, precision, d_before, d_after)[0], a, "(d) caller's stream, resident grid asked for")
    _same_bits(_fly(ens, precision, e_before, e_after)[0], a, "(e) streams switched under the resident grid")
    S.synchronize()
    # the caller's stream against the reference, not against the engine
    ob = ens.to_oracle_batch()
    ob.step(1000 * 1e-6, 40, ticks=afa.plan_ticks(1.0 / 500.0, 0, 1000, 40)[0])
    what = "caller's stream, 40 steps, %s" % layout
    for k, ref in dict(pos=ob.pos, vel=ob.vel, att=ob.att, ang_vel=ob.ang_vel, motor_speed=ob.motor_speed, gyro=ob.gyro,
                       acc=ob.acc).items():
        err = record_parity(what, precision, k, b[k], ref)
        t = max(tol, 1e-6) if k in ("gyro", "acc") else tol      # (the IMU sample is float arithmetic in every build: test_gpu_parity._cmp_state)
        assert err <= t, "%s %s: rel err %.3g > %.1g (floor %g)" % (what, k, err, t, FLOORS[k])
    assert_array_equal(b["rng"], ob.rng)


@pytest.mark.parametrize("n", [1024, 1023])
def test_split_edges_on_a_callers_stream(n):
    """two parts on a caller's stream at the smallest ensemble that splits (1 024: at 512) and the largest that does not"""
    import torch
    ens = random_ensemble(n, seed=62)
    S = torch.cuda.Stream()

    def split(e, k):
        if k == 0:
            e.set_step_mode(afa.AFE_STEP_LAUNCH)
            e.set_stream(S.cuda_stream)
            e.set_split_stepping(2)

    def launch(e, k):
        if k == 0:
            e.set_step_mode(afa.AFE_STEP_LAUNCH)
            e.set_split_stepping(1)

    _same_bits(_fly(ens, AFE_F32, split)[0], _fly(ens, AFE_F32, launch)[0], "n = %d" % n)
    S.synchronize()


# ---- 2. torch produces, the engine consumes, no sync in between ------------------------------------------------------
N_STREAMS = 4


def _streams():
    """HIP carries a process's streams on a handful of hardware queues (four unless the host asks for more), and two streams
    that share a queue are serialised by it: a launch that left the caller's stream for one that happens to share its
    queue would be ordered by luck.  Every ordering case therefore runs on four streams made one after the other."""
    import torch
    return [torch.cuda.Stream() for _ in range(N_STREAMS)]


def test_torch_produces_and_the_engine_queries_at_once(ora):
    """xyz holds world A; on the caller's stream: the delay, xyz <- world B, the engine's query -- which must answer for B.
    The plain query and the one on the engine's query stream, which is ordered behind the caller's stream at the call."""
    import torch
    what = "torch produces, the engine queries"
    n = 3000
    A = random_ensemble(n, seed=21).data.pos.astype(np.float32)
    B = random_ensemble(n, seed=22).data.pos.astype(np.float32)
    ref_a, ref_b = ora.nearest_neighbour(A), ora.nearest_neighbour(B)
    _differ(what, (ref_a[1] != ref_b[1]).sum())
    t_a, t_b = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    xyz = t_a.clone()
    d2 = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
    idx = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    streams = _streams()
    with random_ensemble(n, seed=21).to_engine(AFE_F32) as e:

        def grid():
            e.nearest_neighbour(xyz.data_ptr(), n, d2.data_ptr(), idx.data_ptr())

        def on_its_own_stream():       # ordered behind the caller's stream at the call
            e.nearest_neighbour_async(xyz.data_ptr(), n, d2.data_ptr(), idx.data_ptr())
            e.query_sync()

        for k, stream in enumerate(streams):
            e.set_stream(stream.cuda_stream)
            for query in (grid, on_its_own_stream):
                with torch.cuda.stream(stream):
                    xyz.copy_(t_a)
                t_call, _ = _timed(stream, query)                     # with nothing ahead of it: world A's answer
                assert_array_equal(idx.cpu().numpy(), ref_a[1])
                assert_array_equal(d2.cpu().numpy(), ref_a[0])
                _delay(stream, t_call, "%s, %s, stream %d" % (what, query.__name__, k))
                with torch.cuda.stream(stream):
                    xyz.copy_(t_b, non_blocking=True)
                query()                                               # queued by the host at once
                stream.synchronize()
                assert_array_equal(idx.cpu().numpy(), ref_b[1], err_msg="%s, stream %d" % (query.__name__, k))
                assert_array_equal(d2.cpu().numpy(), ref_b[0], err_msg="%s, stream %d" % (query.__name__, k))
        e.set_stream(None)
    torch.cuda.synchronize()           # (the buffers go only now)


def test_two_engines_on_one_callers_stream(ora):
    """Two engines are shards of one world (first_global_index 0 and 1500) on the SAME caller's stream: both step, A packs
    its half, B packs its half, torch puts the halves into the world buffer (afe_pack_positions writes a contiguous
    [3][n]: the column blocks of the world are torch's copies, on the same stream), A and B query -- no sync before the
    last one.  Whoever left the stream would read the world of before the steps."""
    import torch
    n, h, steps = 3000, 1500, 100
    ens = random_ensemble(n, seed=31, type_ids=(5,))
    streams = _streams()
    start = ens.data.pos.astype(np.float32)
    xyz = torch.from_numpy(start).cuda()
    halves = [xyz[:, :h].contiguous(), xyz[:, h:].contiguous()]
    d2 = [torch.full((h,), -1.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    idx = [torch.full((h,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    shards = []
    for k in range(2):
        d = ens.data.slice(k * h, h)
        e = afa.Ensemble(h, first_global_index=k * h)
        e.set_type_table([afa.params_from_type(5)])
        e.set_state(d.pos, d.vel, d.att, d.ang_vel, d.motor_speed)
        e.set_motor_cmds(d.motor_cmd)
        e.set_step_mode(afa.AFE_STEP_LAUNCH)
        e.set_split_stepping(0)
        e.set_stream(streams[0].cuda_stream)
        shards.append(e)

    def cycle(S):
        for e in shards:
            e.step(1000, steps)
        for k, e in enumerate(shards):
            e.pack_positions(halves[k].data_ptr())
            with torch.cuda.stream(S):
                xyz[:, k * h:(k + 1) * h].copy_(halves[k], non_blocking=True)
        for k, e in enumerate(shards):
            e.nearest_neighbour(xyz.data_ptr(), n, d2[k].data_ptr(), idx[k].data_ptr())

    def judge(what):
        world = np.concatenate([e.get_state(dtype=np.float32)["pos"] for e in shards], axis=1)
        assert_array_equal(xyz.cpu().numpy(), world, err_msg=what)
        for k in range(2):
            ref_d, ref_i = ora.nearest_neighbour(world, k * h, h)
            assert_array_equal(idx[k].cpu().numpy(), ref_i, err_msg=what)
            assert_array_equal(d2[k].cpu().numpy(), ref_d, err_msg=what)
        return world

    try:
        t_call, _ = _timed(streams[0], lambda: cycle(streams[0]))    # with nothing ahead of it; the buffers then hold a valid world, stale for the next cycle
        stale = judge("rehearsal")
        for k, S in enumerate(streams):
            for e in shards:
                e.set_stream(S.cuda_stream)
            _delay(S, t_call, "two engines on one stream, stream %d" % k)
            cycle(S)
            S.synchronize()
            fresh = judge("behind the delay, stream %d" % k)
            _differ("two engines on one stream, stream %d" % k, (ora.nearest_neighbour(stale)[0] != ora.nearest_neighbour(fresh)[0]).sum())
            stale = fresh
    finally:
        for e in shards:
            e.close()
    torch.cuda.synchronize()


# ---- 3. torch and the engine take turns on the state, no engine call in between ---------------------------------------
DT3 = 200        # us: the kernels of a 1000 us step; the blocks below stay within a second of flight


def _step_block(e, calls):
    for _ in range(calls):
        e.step(DT3, 1)


def _calibrate_block(e, S):
    """Doubles the number of afe_step calls until the block takes at least 2 ms ON THE DEVICE -- timed with torch events
    behind a delay, so that the host's launch rate is not in the figure: that much work is still queued when torch's clone
    is launched right behind the block.  -> (calls, ms on the idle stream, ms behind a delay, steps spent)"""
    import torch
    calls, spent = 32, 0
    while True:
        t_idle, _ = _timed(S, lambda: _step_block(e, calls))
        _delay(S, t_idle)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(S)
        _step_block(e, calls)
        e1.record(S)
        e1.synchronize()
        spent += 2 * calls
        if e0.elapsed_time(e1) >= 2.0:
            return calls, t_idle, e0.elapsed_time(e1), spent
        calls *= 2
        if calls > 1 << 14:
            pytest.fail("no step block of 2 ms within 16 384 afe_step calls")


@pytest.mark.parametrize("n,parts", [(131072, 0), (1 << 19, 0), (131072, 2)])
def test_the_engine_produces_and_torch_reads_at_once(n, parts):
    """The engine has stepped on the caller's stream.  Then, on that stream: the delay, torch writes new velocities into
    the slab (the device view), a block of steps, and IMMEDIATELY behind it torch's clone of the position slab and a pack
    into a torch tensor, cloned.  The steps must have started from torch's velocities, and both clones hold the state
    after the block -- order at the return of afe_step; everything equals a twin on its own stream that was given the
    same velocities by the host.  At 2^19 vehicles the automatic split must not engage on a caller's stream: its second
    half would step beside the stream, from the velocities of before.  With two parts asked for, the documented
    obligation (afe_event_record) goes between afe_step and torch's work."""
    import torch
    ens = random_ensemble(n, seed=41, type_ids=(5,))
    streams = _streams()
    rng = np.random.default_rng(42)
    what = "n = %d, parts = %d" % (n, parts)
    with ens.to_engine(AFE_F32) as e, ens.to_engine(AFE_F32) as twin:
        e.set_split_stepping(parts)       # stated: with the suite's forced split every engine starts with two parts
        e.set_stream(streams[0].cuda_stream)
        v = e.device_view()
        assert v.state_elem_size == 4
        pos = torch.as_tensor(_Slab(v.pos, (3, v.stride), "<f4"), device="cuda")[:, :n]
        vel = torch.as_tensor(_Slab(v.vel, (3, v.stride), "<f4"), device="cuda")[:, :n]
        anchor = torch.as_tensor(_Slab(v.pos_anchor_xy, (2, v.stride), "<f8"), device="cuda")[:, :n]
        packed = torch.from_numpy(ens.data.pos.astype(np.float32)).cuda()      # valid and stale
        ev = e.event()
        torch.cuda.synchronize()
        calls, t_idle, t_device, spent = _calibrate_block(e, streams[0])
        assert t_device >= 2.0
        twin.step(DT3, spent)
        blocks = MEASUREMENTS.setdefault("caller_stream_step_block_ms", {})
        for k, S in enumerate(streams):
            fresh = rng.normal(0.0, 2.0, (3, n)).astype(np.float32)
            fresh_t = torch.from_numpy(fresh).cuda()
            torch.cuda.synchronize()
            e.set_stream(S.cuda_stream)
            _step_block(e, 1)             # the engine is at work on this stream before the host's writer arrives
            if parts == 2:
                e.record(ev)              # joins the second stream into the caller's, on the device
            _delay(S, t_idle, "the engine produces, %s, stream %d" % (what, k))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(S):
                vel.copy_(fresh_t, non_blocking=True)
            e0.record(S)
            _step_block(e, calls)
            e1.record(S)
            if parts == 2:
                e.record(ev)
            with torch.cuda.stream(S):
                seen = pos.clone()
            e.pack_positions(packed.data_ptr())
            with torch.cuda.stream(S):
                seen_packed = packed.clone()
            S.synchronize()
            blocks["%s, stream %d" % (what, k)] = {"afe_step_calls": calls, "idle_stream_ms": t_idle, "device_ms_calibrated": t_device,
                                                   "device_ms_in_the_test": e0.elapsed_time(e1)}
            st = e.get_state()
            absolute = seen.cpu().numpy().astype(np.float64)
            absolute[:2] += anchor.cpu().numpy()          # x, y live in the slab relative to their anchors
            assert_array_equal(absolute, st["pos"], err_msg="the slab's clone, stream %d" % k)
            assert_array_equal(seen_packed.cpu().numpy(), e.get_state(dtype=np.float32)["pos"], err_msg="the packed clone, stream %d" % k)
            twin.step(DT3, 1)
            twin.set_state(vel=fresh.astype(np.float64))
            twin.step(DT3, calls)
            _same_bits(_everything(e), _everything(twin), "against a twin on its own stream, stream %d" % k)
        e.destroy_event(ev)
        e.set_stream(None)
    torch.cuda.synchronize()


# ---- 4. the library's consumers read the slabs behind the caller's stream --------------------------------------------
N4, FALL = 300, 200


@pytest.fixture(scope="module")
def orchard():
    tris = scen.orchard_mesh(rows=4, cols=4, seed=21)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    rng = np.random.default_rng(2)
    pos = np.stack([rng.uniform(lo[0] * 0.5, hi[0] * 0.8, N4), rng.uniform(lo[1] * 0.5, hi[1] * 0.8, N4), rng.uniform(0.4, 3.0, N4)])
    att = scen.random_attitudes(rng, N4, max_tilt_deg=25.0)
    return tris, pos, att


def _free_fall(precision, pos, att, consumer, what, judge):
    """On each of four caller's streams: the delay, 200 steps of free fall, the consumer -- no sync before it -- and then
    judge(state before the fall, state after, the consumer's answer, engine time, stream number).  `consumer(engine)`
    returns (the call, its cleanup)."""
    streams = _streams()

    def make(S):
        e = afa.Ensemble(N4, precision=precision)
        e.set_type_table([afa.params_from_type(5)])
        e.set_state(pos, np.zeros((3, N4)), att, np.zeros((3, N4)), np.zeros((4, N4)))
        e.set_motor_cmds(np.zeros((4, N4), np.float32))
        e.set_step_mode(afa.AFE_STEP_LAUNCH)
        e.set_split_stepping(0)
        e.set_stream(S.cuda_stream)
        return e

    e = make(streams[0])                    # a rehearsal times the calls with nothing ahead of them
    call, done = consumer(e)
    t_call, _ = _timed(streams[0], lambda: (e.step(1000, FALL), call()))
    done()
    e.close()
    for k, S in enumerate(streams):
        e = make(S)
        try:
            call, done = consumer(e)
            e.step(1000, 1)                 # (the first step of an engine uploads its table and waits for that: not behind the delay)
            before = e.get_state()
            _delay(S, t_call, "%s, stream %d" % (what, k))
            e.step(1000, FALL)
            got = call()
            S.synchronize()
            after, now = e.get_state(), e.time_us
            done()
        finally:
            e.close()
        assert np.all(after["pos"][2] < before["pos"][2])
        judge(before, after, got, now, k)


def _precision_name(precision):
    return "f32" if precision == AFE_F32 else "f64"


@pytest.mark.parametrize("precision", [AFE_F32, AFE_F64])
def test_depth_camera_behind_the_callers_stream(orchard, ora, precision):
    tris, pos, att = orchard
    scene = afa.Scene(tris)
    cam, mount = afa.camera_default(64, 48), afa.camera_default_mount()
    first, count = 17, 9
    oc = ora.render_camera(cam.width, cam.height, cam.focal_length, cam.depth_scale, cam.max_count)
    oc.cx, oc.cy = cam.cx, cam.cy
    what = "depth camera, " + _precision_name(precision)

    def views(st):
        return [ora.render_depth(oc, tris, st["pos"][:, first + i], st["att"][:, first + i], mount) for i in range(count)]

    def judge(before, after, got, now, k):
        want = views(after)
        _differ("%s, stream %d" % (what, k), sum(int((a != b).sum()) for a, b in zip(views(before), want)))
        for i in range(count):
            assert_array_equal(got[i], want[i], err_msg="view %d, stream %d" % (i, k))

    _free_fall(precision, pos, att, lambda e: (lambda: scene.render_engine(e, cam, mount, first=first, count=count)[0], lambda: None),
               what, judge)
    scene.close()


@pytest.mark.parametrize("precision", [AFE_F32, AFE_F64])
def test_clearance_query_behind_the_callers_stream(orchard, precision):
    tris, pos, att = orchard
    cmap = afa.ClearanceMap(tris)
    what = "clearance query, " + _precision_name(precision)

    def judge(before, after, got, now, k):
        want = cck.query(tris, after["pos"], 2.0)
        _differ("%s, stream %d" % (what, k), (cck.query(tris, before["pos"], 2.0)[0] != want[0]).sum())
        for j in range(3):
            assert_array_equal(got[j], want[j], err_msg="stream %d" % k)

    _free_fall(precision, pos, att, lambda e: (lambda: cmap.query_engine(e, 2.0), lambda: None), what, judge)
    cmap.close()


@pytest.mark.parametrize("precision", [AFE_F32, AFE_F64])
def test_contact_monitor_behind_the_callers_stream(orchard, precision):
    tris, pos, att = orchard
    cmap = afa.ClearanceMap(tris)
    what = "contact monitor, " + _precision_name(precision)

    def consumer(e):
        mon = afa.ContactMonitor(e, cmap, 0.116, 1.0)

        def call():
            counts = mon.update()
            return counts, mon.get()
        return call, mon.close

    def judge(before, after, got, now, k):
        counts, latches = got
        twin, stale = cck.MonitorTwin(tris, N4, 0.116, 1.0), cck.MonitorTwin(tris, N4, 0.116, 1.0)
        want = twin.update(after["pos"], now)
        stale.update(before["pos"], now)
        _differ("%s, stream %d" % (what, k), (stale.min_dist2 != twin.min_dist2).sum())
        assert counts == want, "stream %d" % k
        assert_array_equal(latches["min_dist2"], twin.min_dist2, err_msg="stream %d" % k)
        assert_array_equal(latches["first_contact_us"], twin.first_us, err_msg="stream %d" % k)
        assert_array_equal(latches["first_contact_tri"], twin.first_tri, err_msg="stream %d" % k)

    _free_fall(precision, pos, att, consumer, what, judge)
    cmap.close()


@pytest.mark.parametrize("precision", [AFE_F32, AFE_F64])
def test_statistics_behind_the_callers_stream(orchard, precision):
    tris, pos, att = orchard
    edges = np.array([3, 100, 100, 297])                # a group that starts off the slab's granule, an empty one, a ragged one
    ref = pos + np.random.default_rng(3).standard_normal((3, N4)) * 0.1
    what = "statistics, " + _precision_name(precision)

    def consumer(e):
        mon = afa.StatsMonitor(e, edges)
        mon.set_reference(ref)

        def call():
            rec, _ = mon.update()
            return rec, mon.latches()
        return call, mon.close

    def judge(before, after, got, now, k):
        rec, latches = got
        lat, stale_lat = sck.Latches(N4), sck.Latches(N4)
        want, _ = sck.update(after, ref, lat, edges, now)
        stale, _ = sck.update(before, ref, stale_lat, edges, now)
        _differ("%s, stream %d" % (what, k), sum(int((stale[f] != want[f]).sum()) for f in sck.FLOAT_FIELDS))
        for f in sck.DTYPE.names:
            assert_array_equal(rec[f], want[f], err_msg="%s, stream %d" % (f, k))
        for f, val in lat.as_dict().items():
            assert_array_equal(latches[f], val, err_msg="%s, stream %d" % (f, k))

    _free_fall(precision, pos, att, consumer, what, judge)


# ---- 5. switching streams --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pending", ["steps", "an async query", "half of a split step"])
def test_switching_streams_with_work_queued(pending, ora):
    """Steps are queued on S1 behind a delay, then afe_set_stream(S2): it returns only when S1's work is done (a torch event
    recorded on S1 behind the steps has happened), and the steps that follow on S2 continue the bits of an engine that
    never left its own stream.  Also with a neighbour query pending on the engine's query stream, and with the second
    half of a split step pending on the engine's second stream."""
    import torch
    n = 3000
    ens = random_ensemble(n, seed=51, type_ids=(5,))
    S1, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    query = pending == "an async query"
    xyz = torch.from_numpy(ens.data.pos.astype(np.float32)).cuda()
    d2 = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
    idx = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with ens.to_engine(AFE_F32) as e, ens.to_engine(AFE_F32) as plain:
        e.set_step_mode(afa.AFE_STEP_LAUNCH)
        e.set_split_stepping(2 if pending == "half of a split step" else 0)
        e.set_stream(S1.cuda_stream)
        if query:
            e.set_neighbour_grid_refresh(1000)       # after the first query none reads anything back: the second one stays queued

        def block():
            for _ in range(20):
                e.step(1000, 1)
            if query:
                e.pack_positions(xyz.data_ptr())
                e.nearest_neighbour_async(xyz.data_ptr(), n, d2.data_ptr(), idx.data_ptr())

        t_call, _ = _timed(S1, lambda: (block(), e.query_sync()))
        e.sync()                                     # (joined: the first split step behind the delay orders the second stream behind it too)
        _delay(S1, t_call, "switching streams, " + pending)
        block()
        behind = torch.cuda.Event()
        behind.record(S1)
        e.set_stream(S2.cuda_stream)
        assert behind.query(), "afe_set_stream returned with the old stream's work still queued"
        e.step(1000, 13)
        if query:
            e.query_sync()
            snap = xyz.cpu().numpy()
            ref_d, ref_i = ora.nearest_neighbour(snap)
            assert_array_equal(idx.cpu().numpy(), ref_i)
            assert_array_equal(d2.cpu().numpy(), ref_d)
        got = _everything(e)
        plain.step(1000, 20)
        plain.step(1000, 20)
        if query:
            assert_array_equal(snap, plain.get_state(dtype=np.float32)["pos"])     # the snapshot behind the 40 steps
        plain.step(1000, 13)
        _same_bits(got, _everything(plain), "after the switch")
        e.set_stream(None)
    S1.synchronize()
    S2.synchronize()
    torch.cuda.synchronize()


# ---- 6. destroy ------------------------------------------------------------------------------------------------------
def test_destroy_waits_for_the_callers_stream_and_leaves_it_alone():
    import torch
    n = 3000
    S = torch.cuda.Stream()
    e = random_ensemble(n, seed=71).to_engine(AFE_F32)
    e.set_step_mode(afa.AFE_STEP_LAUNCH)
    e.set_stream(S.cuda_stream)
    t_call, _ = _timed(S, lambda: e.step(1000, 50))
    _delay(S, t_call, "destroy")
    e.step(1000, 50)
    behind = torch.cuda.Event()
    behind.record(S)
    e.close()                               # the slabs are freed here: not under the steps
    assert behind.query(), "afe_destroy returned with the engine's steps still queued on the caller's stream"
    with torch.cuda.stream(S):              # the stream is the caller's: still there, still usable
        y = torch.arange(8, device="cuda") * 3
    S.synchronize()
    assert y.tolist() == [0, 3, 6, 9, 12, 15, 18, 21]


# ---- 7. handle 0 -----------------------------------------------------------------------------------------------------
def test_the_default_stream_is_refused_by_its_reserved_handles():
    """afe_set_stream(e, NULL) restores the engine's own stream, and torch's default stream has handle 0 -- so the default
    stream cannot be meant by its handle.  HIP's reserved handles for it (hipStreamLegacy 1, hipStreamPerThread 2) are not
    supported: refused with AFE_ERR_INVALID_ARG, and the engine stays on the stream it had."""
    import torch
    assert torch.cuda.default_stream().cuda_stream == 0
    S = torch.cuda.Stream()
    with random_ensemble(3000, seed=81, type_ids=(5,), with_wrench=False).to_engine(AFE_F32) as e:
        e.set_split_stepping(0)
        e.set_step_mode(afa.AFE_STEP_PERSISTENT)
        for stream_now in (None, S.cuda_stream):
            e.set_stream(stream_now)
            for handle in (1, 2):
                with pytest.raises(afa.AfeError) as ei:
                    e.set_stream(handle)
                assert ei.value.status == 1 and "default stream" in str(ei.value)
            e.step(1000, 3)
            assert e.persistent_running == (stream_now is None)     # the resident grid tells which stream the engine is on
        e.set_stream(0)                       # 0 is NULL: the engine's own stream, not torch's default stream
        e.step(1000, 3)
        assert e.persistent_running
    S.synchronize()
