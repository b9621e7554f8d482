"""The flight stage machine without a GPU: its host-only entry points, and the numpy specification
(tests/stages_checker.py) against the scalar, line by line restatement of the reference's classes
(tests/stage_machine_reference.py), against its own branch list, against the library's host codec and against the
judging rule's library condition (numpy's functions against glibc's: at most one radio code apart, in at most 1 % of
the values)."""
import ctypes as C

import numpy as np
import pytest

from tests import stage_machine_reference as ref
from tests import stages_checker as sc

INVALID_ARG, OUT_OF_RANGE = 1, 4
N = 130


def fly_script(traj_id, math, info=None, every_tick=None, n=N):
    """the scripted mission on the checker -> list of per-tick dicts (a copy of the state, the held command)"""
    cfg = sc.default_config(traj_id)
    st = sc.new_state(n, cfg)
    st["desired_pos"], st["desired_yaw"], st["centre"] = sc.desired_for(n)
    line = sc.DelayLine(cfg["delay_us"])
    held = (np.zeros((4, n), np.float32), np.zeros(n, np.uint8))
    now, out = 0, []
    for k, step in enumerate(sc.script(n)):
        now += step["dt_us"]
        sc.apply_step(st, step)
        pos, vel, att, since = sc.script_state(n, k)
        msg = sc.tick(st, cfg, now, pos, vel, att, since, step["start"], step["stop"], math, info)
        held = sc.deliver(held, line.tick(now, msg), info)
        out.append(dict(st={f: st[f].copy() for f in sc.GET_FIELDS}, held=held, counters=sc.counters(st), now=now))
        if every_tick is not None:
            every_tick(k, step, now, (pos, vel, att, since), out[-1])
    return out


@pytest.fixture(scope="module")
def flown():
    """all six trajectories with glibc's functions, the branch counts summed"""
    info = {}
    return {t: fly_script(t, sc.glibc_math, info) for t in range(6)}, info


def test_default_config_values_and_refusals(afa):
    c = afa.stages_default_config(5)
    assert c.struct_bytes == C.sizeof(afa.StagesConfig)
    got, want = sc.config_from(c), sc.default_config()
    assert (got["period_us"], got["delay_us"]) == (20000, 30000)
    assert list(c.min_corner) == [-100.0, -100.0, -2.0] and list(c.max_corner) == [100.0, 100.0, 20.0] and c.min_normal_height == 0.0
    assert (c.not_seen_timeout_s, c.spool_up_time_s, c.spool_up_thrust_by_weight, c.takeoff_time_s, c.get_into_action_time_s,
            c.landing_speed, c.traj_id) == (0.5, 0.5, 0.25, 2.0, 2.0, 0.5, 3)
    for k, v in want.items():
        assert np.array_equal(got[k], v), k
    f = afa.follower_default_config(5)                         # the controller's four, as the follower derives them
    for t in (1, 2, 4, 5):
        ct, ft = afa.stages_default_config(t), afa.follower_default_config(t)
        assert (ct.nat_freq, ct.damping, ct.att_time_const_xy, ct.att_time_const_z) == (ft.nat_freq, ft.damping, ft.att_time_const_xy,
                                                                                       ft.att_time_const_z)
    assert np.float32(c.att_time_const_z) == np.float32(f.att_time_const_z) != np.float32(0.4)
    L = afa.library()
    assert L.afe_stages_default_config(5, None) == INVALID_ARG
    for bad in (0, 3, 6, -1):
        assert L.afe_stages_default_config(bad, C.byref(afa.StagesConfig())) == INVALID_ARG


def test_the_stage_machine_refuses_null_handles_without_a_gpu(afa):
    L = afa.library()
    d = np.zeros(3)
    assert L.afe_stages_destroy(None) == INVALID_ARG
    assert L.afe_stages_info(None, None, None, None, None) == INVALID_ARG
    assert L.afe_stages_tick(None, 0, 0, None) == INVALID_ARG
    assert L.afe_stages_create(None, C.byref(afa.stages_default_config(5)), C.byref(C.c_void_p())) == INVALID_ARG
    assert L.afe_stages_set_desired_position(None, 0, 1, d.ctypes.data) == INVALID_ARG
    assert L.afe_stages_set_desired_yaw(None, 0, 1, d.ctypes.data) == INVALID_ARG
    assert L.afe_stages_set_centre(None, 0, 1, d.ctypes.data) == INVALID_ARG
    assert L.afe_stages_set_unsafe(None, 0, 1) == INVALID_ARG
    assert L.afe_stages_request(None, 0, 1, 1, 0) == INVALID_ARG
    assert L.afe_stages_set_warnings(None, 0, 1, d.ctypes.data) == INVALID_ARG
    assert L.afe_stages_get(None, 0, 1, None) == INVALID_ARG
    assert L.afe_stages_attach_gps_estimator(None, None) == INVALID_ARG
    x = np.zeros(4)
    assert L.afe_stages_selftest_math(-1, 6, 4, x.ctypes.data, x.ctypes.data) == INVALID_ARG
    assert L.afe_stages_selftest_math(-1, 0, -1, x.ctypes.data, x.ctypes.data) == INVALID_ARG
    assert L.afe_stages_selftest_math(-1, 0, 4, None, x.ctypes.data) == INVALID_ARG
    assert L.afe_stages_selftest_math(-1, 0, 0, x.ctypes.data, x.ctypes.data) == 0          # nothing to do
    # the constants the package and the header share
    assert (afa.AFE_STAGE_WAIT_FOR_START, afa.AFE_STAGE_EMERGENCY, afa.AFE_SAFETY_USER_UNSAFE, afa.AFE_WARN_LOW_BATT) == (0, 6, 8, 1)
    assert (sc.WAIT, sc.SPOOLUP, sc.TAKEOFF, sc.FLIGHT, sc.LANDING, sc.COMPLETE, sc.EMERGENCY) == tuple(range(7))


def test_the_script_reaches_every_live_branch(flown):
    _, info = flown
    counts = {k: info.get(k, 0) for k in sc.BRANCHES}
    print(counts)
    for k, live in sc.BRANCHES.items():
        if live:
            assert counts[k] > 0, "no vehicle of the script takes the branch %r: %r" % (k, counts)
        else:
            assert counts[k] == 0, "the branch %r is marked dead and was taken" % k
    assert set(info) == set(sc.BRANCHES)


def test_the_script_ends_a_mission(flown):
    last = flown[0][3][-1]
    c = last["counters"]
    assert c[sc.COMPLETE] + c[sc.EMERGENCY] == N and c[sc.EMERGENCY] > 0 and c[7] == c[sc.COMPLETE]
    # Emergency is never left, and the overrides are the reference's: vehicle 0 (unsafe when its spool-up time passed) took
    # off, vehicle 4 (unsafe at frac >= 1) flew, vehicle 2 (unsafe with a low battery) landed, vehicle 16 completed
    stages = np.stack([t["st"]["stage"] for t in flown[0][3]])
    for v in range(N):
        em = np.flatnonzero(stages[:, v] == sc.EMERGENCY)
        assert em.size == 0 or (stages[em[0]:, v] == sc.EMERGENCY).all(), v
    assert stages[3, 0] == sc.TAKEOFF and stages[8, 4] == sc.FLIGHT and stages[2, 2] == sc.LANDING and stages[24, 16] == sc.COMPLETE
    assert stages[2, 1] == sc.EMERGENCY and stages[5, 3] == sc.EMERGENCY and stages[10, 5] == sc.EMERGENCY and stages[10, 17] == sc.EMERGENCY


@pytest.mark.parametrize("traj_id", range(6))
def test_checker_equals_the_scalar_restatement(traj_id):
    """130 objects of the scalar class beside the numpy checker: every field after every tick, the held commands included"""
    cfg = sc.default_config(traj_id)
    des, yaw, centre = sc.desired_for(N)
    machines = [ref.ExampleVehicleStateMachine(cfg) for _ in range(N)]
    for v, m in enumerate(machines):
        m.desired_pos, m.desired_yaw, m.centre = tuple(des[:, v]), des.dtype.type(yaw[v]), tuple(centre[:, v])
    lines = [sc.DelayLine(cfg["delay_us"]) for _ in range(N)]
    held = [((np.float32(0),) * 4, 0) for _ in range(N)]
    vec = lambda name, v: np.array(getattr(machines[v], name))      # noqa: E731

    def every_tick(k, step, now, state, got):
        pos, vel, att, since = state
        if step["request"] is not None:
            idx, start, stop = step["request"]
            for v in idx:
                machines[v].request = start | (stop << 1)
        for v in ([] if step["warnings"] is None else step["warnings"]):
            machines[v].warnings = 1
        for v in ([] if step["unsafe"] is None else step["unsafe"]):
            machines[v].safety.set_unsafe()
        for v, m in enumerate(machines):
            msg = m.run(step["start"], step["stop"], now, pos[:, v], vel[:, v], att[:, v], since[v], sc.glibc_math)
            due = lines[v].tick(now, msg)
            if due is not None:
                held[v] = ref.deliver(held[v], due)
        st = got["st"]
        for v, m in enumerate(machines):
            where = (traj_id, k, v)
            assert (st["stage"][v], st["last_stage"][v], st["t0_us"][v], st["safety"][v], st["ready"][v], st["msg_type"][v]) == \
                (m.stage, m.last_stage, m.t0_us, m.safety.bits(), int(m.ready), m.msg_type), where
            for name in ("init_pos", "last_pos", "last_vel", "last_acc", "computed", "sent"):
                assert sc.same_bits(np.ascontiguousarray(st[name][:, v]), vec(name, v)), (where, name, st[name][:, v], vec(name, v))
            assert sc.same_bits(st["cmd_yaw"][v:v + 1], np.array([m.cmd_yaw])), where
            assert sc.same_bits(np.ascontiguousarray(got["held"][0][:, v]), np.array(held[v][0], np.float32)), where
            assert got["held"][1][v] == held[v][1], where

    fly_script(traj_id, sc.glibc_math, every_tick=every_tick)
    assert sum(m.stage == ref.COMPLETE for m in machines) > N // 2


def test_numpy_against_glibc_stays_inside_the_cap(flown):
    """The judging rule's condition: an ulp-level difference between two libraries' functions moves the sent commands by at
    most one radio code (35 / 32768), in at most 1 % of the values.  The stage of a vehicle never depends on them."""
    differing = total = 0
    for traj_id in range(6):
        other = fly_script(traj_id, sc.numpy_math)
        for a, b in zip(flown[0][traj_id], other):
            dist = sc.code_distance(a["st"]["sent"], b["st"]["sent"])
            assert dist.max() <= 1
            differing += np.count_nonzero(dist)
            total += dist.size
            for name in ("stage", "last_stage", "t0_us", "safety", "ready", "msg_type", "init_pos"):
                assert sc.same_bits(a["st"][name], b["st"][name]), name
    print("numpy against glibc: %d of %d codes differ" % (differing, total))
    assert differing <= 0.01 * total


def test_codec_and_delivery_are_the_librarys(afa, flown):
    """decode(create_rates_command(computed)) == sent bit for bit with the host codec; what a delivery leaves is what
    afe_set_commands_from_radio's rule leaves of a rates, an idle and a kill packet"""
    seen = set()
    for k in (0, 5, 12, 26, 40):
        st = flown[0][3][k]["st"]
        for v in range(N):
            t = int(st["msg_type"][v])
            seen.add(t)
            if t == sc.MSG_RATES:
                m = afa.radio_decode(afa.radio_create_rates_command(0, st["computed"][0, v], st["computed"][1:4, v]))
                assert m.type == 5
                assert sc.same_bits(np.array([m.floats[i] for i in range(4)], np.float32), np.ascontiguousarray(st["sent"][:, v])), (k, v)
            else:
                assert not st["computed"][:, v].any() and not st["sent"][:, v].any()
    assert seen == {sc.MSG_NONE, sc.MSG_RATES, sc.MSG_IDLE, sc.MSG_KILL}
    # idle and kill: type 6 / 2 leave zeros and have = 0, as afe_set_commands_from_radio does (afe_engine.cpp); type 0 leaves what was
    held = (np.full((4, 3), 7, np.float32), np.ones(3, np.uint8))
    rates, have = sc.deliver(held, (np.array([sc.MSG_IDLE, sc.MSG_KILL, sc.MSG_NONE], np.uint8), np.full((4, 3), 9, np.float32)))
    assert rates[:, 0].tolist() == [0] * 4 and rates[:, 1].tolist() == [0] * 4 and rates[:, 2].tolist() == [7] * 4
    assert have.tolist() == [0, 0, 1]
