"""The planner's four per-candidate tests, exercised and independently judged (tests/plan_checker.py).  CPU only.

Every other planner test draws tame states (|v0| <~ 4 m/s, acc0 sigma <= 1.5 m/s^2, gravity exactly +y) and samples of
2-3 s: under those no candidate is ever rejected for thrust, body rate or speed, so half of RapidTrajectoryGenerator's
feasibility code runs without consequence.  Here the aggressive distribution of plan_checker makes each of the flag
values 1 / 3 / 7 / 15 at least 5 % of the candidates, every candidate is planned alone (no cost pruning: all four tests
run) and each flag is held against conditions a correct planner must satisfy whatever its implementation.

First the judge itself against planted cases with known answers, then the oracle under it."""
import numpy as np
import pytest

from tests import plan_checker as pc

W, H, FOCAL, SCALE = 320, 240, 160.0, 10.0 / 256.0
RADIUS, PLANNING_RADIUS, MIN_DIST = 0.116, 0.174, 0.5
SECTION_TIMES = (0.5, 0.02, 1e-3, 1e-6)
TIGHT_LIMITS = dict(min_thrust=8.0, max_thrust=20.0, max_ang_vel=5.0, max_velocity=3.0)


class Cfg:
    """what the judge reads of a planner configuration"""

    def __init__(self, **kw):
        self.width, self.height, self.depth_scale, self.focal_length = W, H, 0.04, FOCAL
        self.cx, self.cy = W / 2.0, H / 2.0
        self.true_vehicle_radius, self.planning_vehicle_radius, self.min_checking_dist = RADIUS, PLANNING_RADIUS, MIN_DIST
        self.min_thrust, self.max_thrust, self.max_ang_vel, self.max_velocity = 5.0, 30.0, 20.0, 5.0
        self.cost_type, self.cost_vec = 0, [0.0, 0.0, 1.0]
        self.__dict__.update(kw)


# ---- the judge against planted cases -----------------------------------------------------------------------------
def _straight_ahead(depth, T):
    cfg = Cfg()
    j = pc.Judged(cfg, [[0, 0, 0]], [[0, 0, 0]], [[0, 9.81, 0]], [[cfg.cx, cfg.cy, depth, T]])
    return cfg, j


def test_closed_form_meets_its_boundary_conditions():
    rng = np.random.default_rng(1)
    n = 64
    v0, a0, pf, T = rng.normal(0, 2, (n, 3)), rng.normal(0, 3, (n, 3)), rng.normal(0, 3, (n, 3)), rng.uniform(0.25, 3.0, n)
    c = pc.min_jerk(v0, a0, pf, T)
    t = np.stack([np.zeros(n), T], axis=1)
    for order, start, end in ((0, np.zeros((n, 3)), pf), (1, v0, np.zeros((n, 3))), (2, a0, np.zeros((n, 3)))):
        got = pc._evaluate(pc._derivative(c, order), t)
        np.testing.assert_allclose(got[:, 0], start, rtol=0, atol=1e-15)
        np.testing.assert_allclose(got[:, 1], end, rtol=0, atol=2e-11)       # (sums of terms up to 1e4 that cancel)


def test_hover_to_hover_has_closed_form_thrust_and_body_rate():
    """from rest to rest L ahead in T: a_z(t) = L / T^2 (60 s - 180 s^2 + 120 s^3), s = t / T, largest 10 / sqrt(3) L / T^2;
    the thrust is that against gravity at right angles, and at t = 0 the body turns at jerk / g = 60 L / T^3 / 9.81"""
    L, T = 3.0, 1.5
    cfg, j = _straight_ahead(L, T)
    peak = 10.0 / np.sqrt(3.0) * L / T ** 2
    assert j.thrust_min[0] == pytest.approx(9.81, rel=1e-14)
    assert j.thrust_max[0] == pytest.approx(np.hypot(9.81, peak), rel=1e-5)    # (the grid misses the peak by T / 1600 at most)
    assert j.thrust_max[0] <= np.hypot(9.81, peak) * (1 + 1e-14)
    assert j.rate_max[0] >= 60.0 * L / T ** 3 / 9.81 * (1 - 1e-14)
    lo, hi, rate = pc.dynamics(j.coeffs, [[0, 9.81, 0]], [T], points=2)       # (t = 0 and T alone)
    assert rate[0] == pytest.approx(60.0 * L / T ** 3 / 9.81, rel=1e-13) and lo[0] == pytest.approx(9.81, rel=1e-14)


def test_six_metres_per_second_on_one_axis_fails_the_velocity_rule():
    """rest to rest: v_z(t) = L / T 30 s^2 (1 - s)^2, largest 1.875 L / T at half time -- 6 m/s for 6.4 m in 2 s"""
    cfg, j = _straight_ahead(6.4, 2.0)
    assert j.speed[0, 2] == pytest.approx(6.0, rel=1e-13) and j.speed[0, 0] == 0 and j.speed[0, 1] == 0
    bad, _ = pc.violations(cfg, j, [7])
    assert len(bad) == 1 and "admissible" in bad[0]
    assert pc.violations(cfg, j, [3])[0] == []
    cfg.max_velocity = 6.5
    assert pc.violations(cfg, j, [7])[0] == []
    assert pc.violations(cfg, j, [3])[0] == []                # x and y do not move: the reference's early return on |alpha| / 6 <= 1e-6
    j = pc.Judged(cfg, [[0, 0, 0]], [[0, 0, 0]], [[0, 9.81, 0]], [[cfg.cx + 40, cfg.cy + 20, 6.4, 2.0]])
    np.testing.assert_allclose(j.speed[0], [1.5, 0.75, 6.0], rtol=1e-13)
    assert len(pc.violations(cfg, j, [3])[0]) == 1            # rejected for speed although no axis reaches the limit


def test_dynamics_rule_catches_an_accepted_candidate_beyond_a_limit():
    cfg, j = _straight_ahead(3.0, 0.6)                         # peak thrust ~ 49 m/s^2
    assert j.thrust_max[0] > 30
    assert len(pc.violations(cfg, j, [3])[0]) == 1 and pc.violations(cfg, j, [1])[0] == []
    assert pc.violations(cfg, j, [5])[0] != []                 # flags that do not nest


def _wall_image(first_column, counts):
    img = np.full((H, W), 250, np.uint16)                      # 10 m: out of reach
    img[:, first_column:] = counts
    return img


def test_clearance_through_a_trunk_and_beside_a_wall():
    cfg, j = _straight_ahead(4.0, 2.0)
    trunk = np.full((H, W), 250, np.uint16)
    trunk[:, 150:171] = 50                                     # 2 m ahead, 0.26 m wide, dead ahead
    assert pc.clearance(cfg, trunk, j.coeffs[0], 2.0) < 0.0    # inside a pixel's footprint
    # a wall 2 m ahead that starts 12 columns right of centre: its nearest ray starts at x = 2 * 12.5 / 160, z = 2 and
    # leads away from the path; the pixel's footprint takes half a diagonal, 2 * sqrt(0.5) / 160, off that
    offset = 2.0 * 12.5 / FOCAL
    got = pc.clearance(cfg, _wall_image(172, 50), j.coeffs[0], 2.0)
    assert got == pytest.approx(offset - 2.0 * np.sqrt(0.5) / FOCAL, abs=2e-3)
    assert pc.clearance(cfg, _wall_image(172, 50), j.coeffs[0], 2.0) > RADIUS > pc.clearance(cfg, _wall_image(166, 50), j.coeffs[0], 2.0)
    # out of reach, nearer than the vehicle's own radius, behind the end point's reach, and before min_checking_dist: not judged
    assert pc.clearance(cfg, _wall_image(260, 50), j.coeffs[0], 2.0) == pc.CLEARANCE_CAP
    assert pc.clearance(cfg, _wall_image(0, 2), j.coeffs[0], 2.0) == pc.CLEARANCE_CAP
    assert pc.clearance(cfg, _wall_image(0, 120), j.coeffs[0], 2.0) == pc.CLEARANCE_CAP
    short = pc.Judged(cfg, [[0, 0, 0]], [[0, 0, 0]], [[0, 9.81, 0]], [[cfg.cx, cfg.cy, 0.45, 1.0]])
    assert pc.clearance(cfg, _wall_image(0, 5), short.coeffs[0], 1.0) == pc.CLEARANCE_CAP


def test_replay_of_a_hand_made_search():
    #        0    1    2    3    4    5    6    7
    cost = [-1., -2., -1.5, -3., -2.5, -4., -3.5, -9.]
    flag = [15,   7,   0,    15,  0,    3,   0,    1]
    low, best, n = pc.replay(cost, flag)
    assert list(low) == [True, True, True, True, False, True, True, True] and best == 3 and n == 7
    # candidate 2 was examined (its cost beats candidate 0's, candidate 1 did not move the best) and 6 too
    low, best, n = pc.replay(cost, [15, 7, 1, 15, 0, 3, 1, 1])
    assert np.array_equal(low, np.array([15, 7, 1, 15, 0, 3, 1, 1]) != 0)
    low, best, n = pc.replay([1.0, 1.0], [15, 0])                                                # a tie is not lower
    assert list(low) == [True, False] and best == 0 and n == 1
    assert pc.replay([], [])[1:] == (-1, 0)


# ---- the oracle under the judge ----------------------------------------------------------------------------------
N_IMAGES, STATES_PER_IMAGE, N_CAND = 6, 6, 200


def _ocfg(ora, **kw):
    c = ora.planner_config(W, H, SCALE, FOCAL, RADIUS, PLANNING_RADIUS, MIN_DIST)
    c.max_pyramids = 64
    for key, value in kw.items():
        setattr(c, key, value)
    return c


@pytest.fixture(scope="module")
def singles(ora, afa):
    """6 synthetic images x 6 states x 200 candidates, each planned alone by the oracle at the reference's limits, and the
    judge's view of the same 7 200 trajectories (which does not depend on the limits)"""
    images = np.stack([afa.scenarios.synthetic_depth_image(seed=200 + k, n_trunks=4 + k) for k in range(N_IMAGES)])
    n = N_IMAGES * STATES_PER_IMAGE
    vel0, acc0, grav = pc.aggressive_states(45, n, upright_every=2)
    samples = pc.aggressive_samples(ora.planner_samples(0, W, H, N_CAND), 0)
    image_of = np.repeat(np.arange(N_IMAGES), STATES_PER_IMAGE)
    state_of = np.repeat(np.arange(n), N_CAND)
    judged = pc.Judged(_ocfg(ora), vel0[:, state_of].T, acc0[:, state_of].T, grav[:, state_of].T, np.tile(samples, (n, 1)))

    def run(cfg):
        flags = np.empty((n, N_CAND), np.uint8)
        results = {}
        for i in range(n):
            for k in range(N_CAND):
                res, f = ora.planner_run(cfg, images[image_of[i]], vel0[:, i], acc0[:, i], grav[:, i], samples[k:k + 1])
                flags[i, k] = f[0]
                if f[0] == 15:
                    results[(i, k)] = res
        return flags, results
    default_flags, default_results = run(_ocfg(ora))
    return dict(images=images, vel0=vel0, acc0=acc0, grav=grav, samples=samples, image_of=image_of, judged=judged, run=run,
                default_flags=default_flags, default_results=default_results)


def _assert_shares(flags, what):
    shares = pc.flag_shares(flags)
    print("%s: oracle's shares of flags 1 / 3 / 7 / 15: %s" % (what, " / ".join("%.1f %%" % (100 * shares[v]) for v in (1, 3, 7, 15))))
    assert min(shares.values()) >= 0.05, (what, shares)
    return shares


def test_oracle_single_candidates_satisfy_every_condition(ora, singles):
    cfg = _ocfg(ora)
    flags, results = singles["default_flags"], singles["default_results"]
    assert np.all(np.isin(flags, (1, 3, 7, 15)))              # alone, a candidate always has the lowest cost so far
    _assert_shares(flags, "single candidates")
    up = np.arange(len(flags)) % 2 == 0
    _assert_shares(flags[up], "upright gravity")
    _assert_shares(flags[~up], "tilted gravity")
    bad, seen = pc.violations(cfg, singles["judged"], flags)
    print(seen)
    assert bad == []
    # winners, at most 300 of them by a fixed stride: polynomial, cost, clearance
    winners = sorted(results)
    picked = winners[::max(1, -(-len(winners) // 300))]
    assert len(picked) >= 200
    worst = pc.CLEARANCE_CAP
    for i, k in picked:
        res, at = results[(i, k)], i * N_CAND + k
        cost = pc.costs(cfg, singles["judged"].pf[at], singles["judged"].T[at])[0]
        b, clear = pc.winner_violations(cfg, singles["images"][singles["image_of"][i]], singles["judged"], at,
                                        [[res.coeffs[q][a] for a in range(3)] for q in range(6)], res.best_cost, cost)
        bad += b
        worst = min(worst, clear)
    print("smallest clearance of %d winners: %.4f m (vehicle radius %.3f)" % (len(picked), worst, RADIUS))
    assert bad == []


@pytest.mark.parametrize("section_time", [s for s in SECTION_TIMES if s != 0.02])
def test_oracle_under_other_section_times(ora, singles, section_time):
    """a coarser bisection leaves more candidates undecided (rejected), a finer one fewer; every answer stays inside the
    judge's conditions"""
    cfg = _ocfg(ora, min_section_time=section_time)
    flags, _ = singles["run"](cfg)
    _assert_shares(flags, "min_section_time %g" % section_time)
    bad, seen = pc.violations(cfg, singles["judged"], flags)
    print(seen)
    assert bad == []
    ref = singles["default_flags"]
    fewer = ((flags & 2) != 0) & ((ref & 2) == 0)
    more = ((flags & 2) == 0) & ((ref & 2) != 0)
    print("min_section_time %g: %d rejected for dynamics (0.02: %d)" % (section_time, (flags == 1).sum(), (ref == 1).sum()))
    if section_time > 0.02:
        assert more.sum() > 0 and fewer.sum() == 0
    else:
        assert more.sum() == 0 and (fewer.sum() > 0 or section_time < 1e-3)


def test_oracle_under_tight_limits(ora, singles):
    cfg = _ocfg(ora, **TIGHT_LIMITS)
    flags, _ = singles["run"](cfg)
    _assert_shares(flags, "limits %s" % (TIGHT_LIMITS,))
    bad, seen = pc.violations(cfg, singles["judged"], flags)
    print(seen)
    assert bad == []


def test_oracle_whole_plans_replay(ora, afa):
    """12 whole 200-candidate searches (both cost types, tilted gravity): the LowCost bits, the winner and the counter
    follow from the judge's costs and the other flags; the winner is the closed form and stays clear"""
    images = np.stack([afa.scenarios.synthetic_depth_image(seed=200 + k, n_trunks=4 + k) for k in range(N_IMAGES)])
    vel0, acc0, grav = pc.aggressive_states(43, 12)
    bad, found = [], 0
    for i in range(12):
        cfg = _ocfg(ora, cost_type=i % 2)
        cfg.cost_vec[0], cfg.cost_vec[1], cfg.cost_vec[2] = (0.3, -0.2, 1.0) if i % 2 == 0 else (0.0, 0.0, 60.0)
        samples = pc.aggressive_samples(ora.planner_samples(i, W, H, N_CAND), i)
        res, flags = ora.planner_run(cfg, images[i % N_IMAGES], vel0[:, i], acc0[:, i], grav[:, i], samples)
        judged = pc.Judged(cfg, np.tile(vel0[:, i], (N_CAND, 1)), np.tile(acc0[:, i], (N_CAND, 1)), np.tile(grav[:, i], (N_CAND, 1)), samples)
        cost = pc.costs(cfg, judged.pf, judged.T)
        low, best, n_checks = pc.replay(cost, flags)
        assert np.array_equal(low, (flags & 1) != 0) and best == res.best_index and n_checks == res.n_cost_checks, i
        bad += pc.violations(cfg, judged, flags)[0]
        if res.found:
            found += 1
            bad += pc.winner_violations(cfg, images[i % N_IMAGES], judged, best, [[res.coeffs[q][a] for a in range(3)] for q in range(6)],
                                        res.best_cost, cost[best])[0]
    assert bad == [] and found >= 6
