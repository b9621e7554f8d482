"""The GPS + IMU state estimator on the device against the REFERENCE's recorded behaviour (tests/golden/gps_reference.npz,
recorded from the reference's own GPSIMUStateEstimator.cpp by tests/golden/make_gps_reference.py) where that behaviour is the
dense algebra's: the first measurement behind 0 to 5 ordinary Predicts, and covariances with one entry that is not finite.
The device is held to the numpy checker bit for bit with the device's own sin, cos and acosf (as in
tests/test_gpu_gps_estimator.py), and the branch of every call, the finite / non-finite masks and the number of restarts
to the fixture's FREE-RUNNING record of the same phase groups and the same covariances.  Neither the reference tree nor
oracle/_ref/gps_probe is needed.  Needs an MI355X."""
import os

import numpy as np
import pytest

from tests import gps_estimator_checker as gc
from tests.scenarios import afa
from tests.test_gpu_gps_estimator import RUNS, _assert_states_equal, _step_to_tick, make_engine

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gps_reference.npz")
SINGULAR = (gc.CALL_BRANCHES.index("singular_nonfinite"), gc.CALL_BRANCHES.index("singular_tiny"))
FIXTURE_N_MAIN = gc.SCRIPT_MIN_N               # the fixture's script m: vehicle g < 6 is phase group g


@pytest.fixture(scope="module")
def fx():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def dmath():
    return gc.device_math(afa)


def _mask(fx, name, events, n):
    return np.unpackbits(fx[name])[:events * 97 * n].reshape(events, 97, n).astype(bool)


def _fly(e, est, script, chk, sampler):
    """the script on the device and, event by event on what the engine reported, in the checker -> per event (device state,
    checker state, checker's branch per vehicle), and per measure (device's n_reinitialised, checker's)"""
    out, counts = [], []
    for ev in script:
        if ev[0] == "imu":
            _step_to_tick(e)
            est.imu()
            gyro, acc = e.get_imu()
            inp = (e.time_us, acc, gyro)
        elif ev[0] == "measure":
            got = est.measure(count_reinitialised=True)
            inp = (e.time_us, e.get_state()["pos"])
        elif ev[0] == "reset_ranges":
            for first, count in ev[1]:
                est.reset(first, count)
            inp = e.time_us
        else:
            raise AssertionError(ev)
        _, sing = gc.run_script([ev], chk, [inp], sampler)
        branch = chk.last_branch.copy()
        if ev[0] == "reset_ranges":
            branch[:] = gc.NO_CALL
            for first, count in ev[1]:
                branch[first:first + count] = gc.CALL_BRANCHES.index("reset")
        if ev[0] == "measure":
            counts.append((got, sing[0]))
        out.append((est.state(), chk.state(), branch))
    return out, counts


def _shifts(n):
    return range(gc.PHASE_GROUPS) if n == 1 else (0,)


@pytest.mark.parametrize("run", RUNS)
def test_phase_groups_device_equals_checker_and_the_references_branches_and_masks(run, fx, dmath):
    """0 to 5 ordinary Predicts between the alignment and the first measurement (gps_estimator_checker.make_phase_script: the
    groups interleaved, so each has vehicles in both waves and in the tail of 130; one vehicle flies the six phases one after
    the other).  After EVERY call the device equals the checker in every field; the checker's branch per vehicle, the
    finite mask of mean and covariance and n_reinitialised equal the reference's free-running record of the same group.
    (The vehicle with the NaN position is held to the checker alone: its branches are its own.)"""
    precision, mode, n = run
    events = len(gc.make_phase_script(FIXTURE_N_MAIN))
    ref_branch = fx["m_fr_branch"][:events]
    ref_mask = _mask(fx, "m_fr_mask", fx["m_fr_branch"].shape[0], FIXTURE_N_MAIN)[:events]
    for shift in _shifts(n):
        script = gc.make_phase_script(n, shift)
        group = gc.phase_group(n, shift)
        e, sampler = make_engine(n, precision, mode)
        est = afa.GpsEstimator(e)
        try:
            chk = gc.Estimator(n, gc.config_from(est.cfg), dmath)
            flown, counts = _fly(e, est, script, chk, sampler)
        finally:
            est.close()
            e.close()
        healthy = np.ones(n, bool)
        if n > 1:
            healthy[n - 1] = False                                   # the NaN position
        m = 0
        for k, (got, want, branch) in enumerate(flown):
            _assert_states_equal(got, want, "shift %d event %d %r" % (shift, k, script[k]))
            rb = ref_branch[k][group]
            assert np.array_equal(branch[healthy], rb[healthy]), (shift, k, script[k], branch.tolist(), rb.tolist())
            mine = np.concatenate([np.isfinite(got["est"]), np.isfinite(got["cov"])])
            theirs = np.concatenate([ref_mask[k][0:13], ref_mask[k][16:97]])[:, group]
            called = healthy & (rb != gc.NO_CALL)
            assert np.array_equal(mine[:, called], theirs[:, called]), (shift, k, script[k])
            if script[k][0] == "measure":
                device, checker = counts[m]
                m += 1
                sick = int(np.isin(branch[~healthy], SINGULAR).sum())
                assert device == checker == int(np.isin(rb[healthy], SINGULAR).sum()) + sick, (shift, k, device, checker)
        # what the issue is about, said once more in plain words: at the first measurement group 0 makes an ordinary update and
        # every other group restarts; nobody hands on a NaN
        first = flown[gc.PHASE_FIRST_MEASURE]
        assert np.array_equal(np.isin(first[2], SINGULAR)[healthy], (group != 0)[healthy])
        assert np.isfinite(first[0]["est"][:, healthy]).all() and np.isfinite(first[0]["cov"][:, healthy]).all()


@pytest.mark.parametrize("run", RUNS)
def test_one_entry_that_is_not_finite_poisons_all_81_and_the_update_restarts_clean(run, fx, dmath):
    """set_state with each of the fixture's covariances -- one NaN, +Inf or -Inf on a diagonal and an off-diagonal place of
    each block --, then imu, then measure.  After the imu all 81 entries are NaN; the measure restarts: the mean is the
    measurement at rest, the covariance ResetVariance's, the vehicle counted.  Device equals checker bit for bit, and branch
    and masks equal the reference's record (script p, its second and third event).  At 130 the 36 vehicles lie across the
    first wave's edge; one vehicle takes the 36 covariances one after the other."""
    precision, mode, n = run
    p = gc.N_POISON
    ref_branch = fx["p_fr_branch"]
    ref_mask = _mask(fx, "p_fr_mask", ref_branch.shape[0], p)
    assert (ref_branch[1] == gc.CALL_BRANCHES.index("predict")).all() and (ref_branch[2] == SINGULAR[0]).all()
    assert not ref_mask[1][16:97].any() and ref_mask[2][16:97].all() and ref_mask[2][0:13, :p - 1].all()      # (its last vehicle's position is NaN)
    first = 46 if n > 1 else 0
    e, sampler = make_engine(n, precision, mode)
    est = afa.GpsEstimator(e)
    try:
        chk = gc.Estimator(n, gc.config_from(est.cfg), dmath)

        def imu():
            _step_to_tick(e)
            est.imu()
            gyro, acc = e.get_imu()
            chk.imu(e.time_us, *sampler.sample(gyro, acc))

        imu()
        for case in (range(p) if n == 1 else [None]):
            near = e.get_state()["pos"][:, first:first + (1 if n == 1 else p)]
            e13, c81, k3 = gc.payload("poison", p, np.zeros((3, p)))
            cols = slice(case, case + 1) if n == 1 else slice(0, p)
            e13, c81, k3 = e13[:, cols].copy(), c81[:, cols], k3[:, cols]
            e13[0:3] = near
            est.set_state(e13, c81, k3, first=first)
            chk.set_state(e13, c81, k3, first=first)
            who = slice(first, first + e13.shape[1])
            imu()
            got = est.state()
            _assert_states_equal(got, chk.state(), "case %r, behind the imu" % case)
            assert np.isnan(got["cov"][:, who]).all()
            assert (chk.last_branch[who] == gc.CALL_BRANCHES.index("predict")).all()
            assert np.isfinite(got["est"][:, who]).all() == bool(ref_mask[1][0:13, :p - 1].all())
            before = chk.count["singular_nonfinite"]
            counted = est.measure(count_reinitialised=True)
            now, z = e.time_us, e.get_state()["pos"]
            assert counted == chk.measure(now, z)
            got = est.state()
            _assert_states_equal(got, chk.state(), "case %r, behind the measure" % case)
            assert (chk.last_branch[who] == SINGULAR[0]).all() and chk.count["singular_nonfinite"] - before >= e13.shape[1]
            fresh = gc.Estimator(e13.shape[1], chk.cfg).cov.reshape(81, -1)
            assert gc.same_bits(got["cov"][:, who], fresh) and gc.same_bits(got["est"][0:3, who], z[:, who])
            assert (got["est"][3:6, who] == 0).all() and (got["est"][10:13, who] == 0).all() and (got["est"][6, who] == 1).all()
            assert np.isfinite(got["cov"][:, who]).all() == bool(ref_mask[2][16:97].all())
    finally:
        est.close()
        e.close()


@pytest.mark.parametrize("run", RUNS[:4])
def test_attached_consumers_read_a_finite_estimate_behind_the_first_measurement(run, dmath):
    """A trajectory follower and a flight stage machine attached to the estimator while the phase groups meet their first
    measurement.  The stage machine is started three ticks ahead (spool-up time 0, so that it stands in take-off and runs the
    position controller on the estimate at its tick behind the measurement); the follower ticks there too.  What both
    compute from the estimate is finite for every vehicle but the one whose position is NaN -- in particular for the groups
    with one and two ordinary Predicts, whose velocity and attitude were NaN there before the definition took the dense
    algebra's non-finite behaviour."""
    precision, mode, n = run
    script = gc.make_phase_script(n)[:gc.PHASE_FIRST_MEASURE + 1]
    e, sampler = make_engine(n, precision, mode)
    est = afa.GpsEstimator(e)
    cfg = afa.stages_default_config(5)
    cfg.traj_id = 0
    cfg.spool_up_time_s = 0.0
    cfg.period_us, cfg.delay_us = 2000, 0            # it ticks with the IMU here: a message is delivered at once, the ring never fills
    for k in range(3):
        cfg.min_corner[k], cfg.max_corner[k] = -1e4, 1e4
    stages = afa.FlightStages(e, cfg=cfg)
    fol = afa.Follower(e)
    try:
        stages.attach_gps_estimator(est)
        stages.set_desired_position(np.tile(np.array([[300.0], [-200.0], [42.0]]), (1, n)))
        fol.attach_gps_estimator(est)
        imus = 0
        for ev in script:
            if ev[0] == "imu":
                _step_to_tick(e)
                est.imu()
                imus += 1
                if imus in (3, 4, 5):
                    stages.tick(True, False)
            elif ev[0] == "measure":
                est.measure()
            else:
                for first, count in ev[1]:
                    est.reset(first, count)
        ok = np.arange(n - 1)
        state = est.state()["est"]
        assert np.isfinite(state[:, ok]).all()
        stages.tick(True, False)
        got = stages.get(fields=["stage", "computed", "sent"])
        assert (got["stage"][ok] == 2).all(), np.unique(got["stage"])       # take-off: the position controller ran
        assert np.isfinite(got["computed"][:, ok]).all() and np.isfinite(got["sent"][:, ok]).all()
        inp = fol.planner_inputs()                                    # (nobody has a plan: every vehicle holds its place)
        for k in ("vel0", "acc0", "grav"):
            assert np.isfinite(inp[k][:, ok]).all(), k
        fol.tick()
        computed, sent = fol.get_command()
        assert np.isfinite(computed[:, ok]).all() and np.isfinite(sent[:, ok]).all()
    finally:
        fol.close()
        stages.close()
        est.close()
        e.close()
