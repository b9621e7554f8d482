"""Image ground truth (DepthImagePlanner.cpp:1031-1098), the parts that need no GPU: the library's host-only sample times,
the numpy checker (tests/truth_checker.py) on hand cases against a scalar restatement written pixel by pixel, and the
checker on a campaign of oracle-planned candidates (the reference's MeasureConservativeness idea: what the pyramid test
calls free must be free)."""
import math

import numpy as np
import pytest

from tests import truth_checker as tc


# ---- sample times -------------------------------------------------------------------------------------------------------
def _running_sum(tb, te, dt):
    out, t = [], tb
    while t < te:
        out.append(t)
        t = t + dt
    return out


def test_sample_times_are_the_running_sum(afa):
    """fails without the feature: the entry point does not exist"""
    n_product_differs = 0
    for tb, te, dt in [(0.0, 3.0, 0.1), (0.0, 2.0, 0.1), (0.3, 2.9, 0.1), (0.0, 0.7, 0.1), (-1.0, 1.1, 0.3), (0.0, 1.0, 0.25),
                       (0.0, 0.05, 0.1), (1e6, 1e6 + 1.0, 0.1), (0.0, 2.7, 0.1), (0.0, 4096.0, 1.0), (0.0, 0.8, 0.1), (0.0, 1.0, 0.1)]:
        want = _running_sum(tb, te, dt)
        got = afa.image_truth_sample_times(tb, te, dt)
        assert got.tobytes() == np.array(want).tobytes(), (tb, te, dt)
        assert tc.sample_times(tb, te, dt) == want
        k, by_product = 0, 0
        while tb + k * dt < te:
            by_product, k = by_product + 1, k + 1
        n_product_differs += by_product != len(want)
    assert n_product_differs >= 2                     # (0, 0.8, 0.1): 9 samples, k * 0.1 gives 8; (0, 1, 0.1): 11 and 10
    assert len(afa.image_truth_sample_times(0.0, 0.8, 0.1)) == 9 and len(afa.image_truth_sample_times(0.0, 1.0, 0.1)) == 11


def test_sample_times_empty_ranges_and_the_cap(afa):
    import ctypes as C
    for tb, te in [(1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.0, float("nan"))]:
        assert len(afa.image_truth_sample_times(tb, te, 0.1)) == 0
    assert len(afa.image_truth_sample_times(0.0, 4096.0, 1.0)) == 4096
    L = afa.library()
    k = C.c_int(-7)
    t = np.full(8, -1.0)
    assert L.afe_image_truth_sample_times(0.0, 4097.0, 1.0, C.byref(k), t.ctypes.data) == 4        # AFE_ERR_OUT_OF_RANGE
    assert L.afe_image_truth_sample_times(-np.inf, 0.0, 1.0, C.byref(k), t.ctypes.data) == 4
    for dt in (0.0, -0.1, float("nan"), float("inf")):
        assert L.afe_image_truth_sample_times(0.0, 1.0, dt, C.byref(k), t.ctypes.data) == 1         # AFE_ERR_INVALID_ARG
    assert L.afe_image_truth_sample_times(0.0, 1.0, 0.1, None, t.ctypes.data) == 1
    assert k.value == -7 and np.all(t == -1.0)         # refusals write nothing
    assert tc.sample_times(0.0, 4097.0, 1.0) is None


# ---- the checker on hand cases --------------------------------------------------------------------------------------------
W, H, F = 72, 40, 36.0


@pytest.fixture(scope="module")
def cfg(afa):
    # the reference vehicle: radii 0.116 / 0.174 m, 0.5 m; edge = int(36 * 0.116 / 0.5) = 8, ignore = int(0.116 * 25.6) = 2
    c = afa.planner_default_config(W, H, 10.0 / 256.0, F, 0.116, 0.174, 0.5)
    assert tc.scalars(c) == (2, 8)
    return c


def _line(p0, v):
    """p(t) = p0 + v t as coeffs [6][3]"""
    c = np.zeros((6, 3))
    c[4], c[5] = v, p0
    return c


def _scalar_judge(cfg, depth, coeffs, tb, te, dt):
    """the definition once more, pixel by pixel with the math module: (verdict, k_fov, k_hit, pixel_hit, n_samples, n_checked)"""
    ignore, edge = tc.scalars(cfg)
    f, cx, cy, r = cfg.focal_length, cfg.cx, cfg.cy, cfg.planning_vehicle_radius
    times = _running_sum(tb, te, dt)
    pts = []
    for t in times:
        pts.append([coeffs[0][a] * t * t * t * t * t + coeffs[1][a] * t * t * t * t + coeffs[2][a] * t * t * t + coeffs[3][a] * t * t +
                    coeffs[4][a] * t + coeffs[5][a] for a in range(3)])
    for k, p in enumerate(pts):
        if p[2] < cfg.min_checking_dist:
            continue
        if math.isnan(p[2]) or p[2] == 0.0:
            continue                      # (the hand cases project finite points only, except the all-NaN path: no violation)
        ix, iy = p[0] * f / p[2] + cx, p[1] * f / p[2] + cy
        if ix <= edge or ix > cfg.width - edge or iy <= edge or iy > cfg.height - edge:
            return 1, k, -1, -1, len(times), 0
    n_checked = 0
    for k, p in enumerate(pts):
        if p[2] < cfg.min_checking_dist:
            continue
        n_checked += 1
        if any(math.isnan(v) for v in p):
            continue                      # every s is a NaN: nothing occludes
        for y in range(cfg.height):
            for x in range(cfg.width):
                d16 = int(depth[y, x])
                if d16 <= ignore:
                    continue
                ex, ey = (x - cx) / f, (y - cy) / f
                n = float(np.float32(math.sqrt(ex * ex + ey * ey + 1.0 * 1.0)))
                ux, uy, uz = ex / n, ey / n, 1.0 / n
                d = p[0] * ux + p[1] * uy + p[2] * uz
                s = d * d - (p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) + r * r
                if s >= 0:
                    m = d16 * cfg.depth_scale
                    qx, qy, qz = m * ex, m * ey, m * 1.0
                    if math.sqrt(qx * qx + qy * qy + qz * qz) < d + math.sqrt(s):
                        return 2, -1, k, y * cfg.width + x, len(times), n_checked
    return 0, -1, -1, -1, len(times), n_checked


def _both(cfg, depth, coeffs, tb, te, dt=0.1):
    rec = tc.judge(tc.ImageRays(cfg, depth), coeffs, tb, te, dt)
    assert (rec["verdict"], rec["k_fov"], rec["k_hit"], rec["pixel_hit"], rec["n_samples"], rec["n_checked"]) == \
        _scalar_judge(cfg, depth, coeffs, tb, te, dt)
    times = _running_sum(tb, te, dt)
    for key, at in (("t_fov", rec["k_fov"]), ("t_hit", rec["k_hit"])):
        assert (math.isnan(rec[key]) and at < 0) or rec[key] == times[at]
    return rec


def test_checker_wall_is_reached_at_the_right_sample(cfg):
    """a wall of count 30 (1.17 m): the sphere (0.174 m) flying straight at it from 0.6 m at 0.5 m/s touches it when
    z + 0.174 > 1.17, i.e. z > 0.998: t > 0.796, the sample k = 8 (t = 0.1 summed eight times)"""
    wall = np.full((H, W), 30, np.uint16)
    rec = _both(cfg, wall, _line([0, 0, 0.6], [0, 0, 0.5]), 0.0, 2.0)
    assert rec["verdict"] == 2 and rec["k_hit"] == 8 and rec["n_samples"] == 20
    assert rec["n_checked"] == 9                                   # z >= 0.5 from the start: samples 0..8
    y, x = divmod(rec["pixel_hit"], W)
    assert abs(x - cfg.cx) <= 2 and abs(y - cfg.cy) <= 2           # the cap round the image centre
    # the same wall, flown past: starting behind it is occluded at once
    assert _both(cfg, wall, _line([0, 0, 1.5], [0, 0, 0.1]), 0.0, 1.0)["k_hit"] == 0


def test_checker_empty_sky_is_free(cfg):
    far = np.full((H, W), 255, np.uint16)
    rec = _both(cfg, far, _line([0, 0, 0.6], [0.1, -0.05, 0.5]), 0.0, 2.0)
    assert rec["verdict"] == 0 and rec["n_checked"] == 20 and rec["k_hit"] == -1 and rec["pixel_hit"] == -1


def test_checker_drift_to_the_border_is_out_of_view_at_the_right_sample(cfg):
    """p = (0.5 t, 0, 1): px = 18 t + 36 > 72 - 8 from t > 1.556 on: k = 16"""
    far = np.full((H, W), 255, np.uint16)
    rec = _both(cfg, far, _line([0, 0, 1.0], [0.5, 0, 0]), 0.0, 3.0)
    assert rec["verdict"] == 1 and rec["k_fov"] == 16 and rec["n_checked"] == 0 and rec["n_samples"] == 30
    # the view is tested for ALL samples first: a wall does not get to answer
    assert _both(cfg, np.full((H, W), 30, np.uint16), _line([0, 0, 1.5], [0.5, 0, 0]), 0.0, 3.0)["verdict"] == 1
    # px <= edge on the left, py on both sides
    assert _both(cfg, far, _line([0, 0, 1.0], [-0.5, 0, 0]), 0.0, 3.0)["k_fov"] == 16      # 36 - 18 t <= 8: t >= 1.556
    assert _both(cfg, far, _line([0, 0, 1.0], [0, 0.25, 0]), 0.0, 3.0)["verdict"] == 1
    assert _both(cfg, far, _line([0, 0, 1.0], [0, -0.25, 0]), 0.0, 3.0)["verdict"] == 1


def test_checker_ignore_boundary(cfg):
    """depth == ignore is the vehicle itself; ignore + 1 is an obstacle 0.117 m away"""
    ignore = tc.scalars(cfg)[0]
    path = _line([0, 0, 0.8], [0, 0, 0.2])
    own = _both(cfg, np.full((H, W), ignore, np.uint16), path, 0.0, 1.0)
    assert own["verdict"] == 0 and own["n_checked"] == 11            # (0.1 summed ten times is still below 1)
    near = _both(cfg, np.full((H, W), ignore + 1, np.uint16), path, 0.0, 1.0)
    assert near["verdict"] == 2 and near["k_hit"] == 0 and near["n_checked"] == 1
    one = np.full((H, W), ignore, np.uint16)
    one[21, 40] = ignore + 1
    assert _both(cfg, one, path, 0.0, 1.0)["pixel_hit"] == 21 * W + 40


def test_checker_all_samples_nearer_than_the_minimum(cfg):
    rec = _both(cfg, np.full((H, W), 3, np.uint16), _line([5.0, 5.0, 0.3], [0, 0, 0.05]), 0.0, 2.0)
    assert rec["verdict"] == 0 and rec["n_checked"] == 0 and rec["n_samples"] == 20


def test_checker_nan_coefficients_are_free_by_the_expressions(cfg):
    c = _line([0, 0, 1.0], [0, 0, 0.1])
    c[2, 1] = np.nan
    c[3, 2] = np.nan
    rec = _both(cfg, np.full((H, W), 3, np.uint16), c, 0.0, 1.0)
    assert rec["verdict"] == 0 and rec["n_checked"] == 11


def test_checker_tally():
    flags = np.array([15, 15, 15, 7, 7, 3, 1, 0], np.uint8)
    verdicts = np.array([0, 1, 2, 0, 2, 0, 0, 1], np.uint8)
    assert tc.tally(flags, verdicts) == dict(n_checked=5, n_planner_free=3, n_correct_in_collision=1, n_incorrect_in_collision=1,
                                             n_free_but_out_of_view=1, n_free_but_occluded=1)


# ---- the checker on a campaign of planned candidates ------------------------------------------------------------------------
def _candidate_coeffs(cfg, v0, a0, sample):
    """the candidate's quintic (RapidTrajectoryGenerator, goal at rest at the deprojected sample) in closed form"""
    px, py, depth, T = sample
    pf = [depth * ((px - cfg.cx) / cfg.focal_length), depth * ((py - cfg.cy) / cfg.focal_length), depth]
    c = np.zeros((6, 3))
    for a in range(3):
        da, dv, dp = -a0[a], -v0[a] - a0[a] * T, pf[a] - v0[a] * T - 0.5 * a0[a] * T * T
        al = (60 * T ** 2 * da - 360 * T * dv + 720 * dp) / T ** 5
        be = (-24 * T ** 3 * da + 168 * T ** 2 * dv - 360 * T * dp) / T ** 5
        ga = (3 * T ** 4 * da - 24 * T ** 3 * dv + 60 * T ** 2 * dp) / T ** 5
        c[:, a] = [al / 120, be / 24, ga / 6, a0[a] / 2, v0[a], 0.0]
    return c


def test_checker_on_planned_candidates(ora, afa):
    """4 synthetic images x 120 candidates, each planned alone by the oracle planner (no cost pruning): every verdict
    occurs in at least 5 % of the 480, and whatever the pyramid test calls collision-free (flags 15) is free."""
    v0, a0, grav = [0.2, -0.1, 0.8], [0.0, 0.0, 0.0], [0.0, 9.81, 0.0]
    verdicts, planner_free = [], []
    for s in range(4):
        img = afa.scenarios.synthetic_depth_image(seed=100 + s, n_trunks=8)
        ocfg = ora.planner_config(320, 240, 10.0 / 256.0, 160.0, 0.116, 0.174, 0.5)
        cfg = afa.planner_default_config(320, 240, 10.0 / 256.0, 160.0, 0.116, 0.174, 0.5)
        rays = tc.ImageRays(cfg, img)
        samples = ora.planner_samples(s, 320, 240, 240)
        for k in range(0, 240, 2):
            res, flags = ora.planner_run(ocfg, img, v0, a0, grav, samples[k:k + 1])
            free = flags[0] == 15
            co = np.array([[res.coeffs[q][a] for a in range(3)] for q in range(6)]) if free else _candidate_coeffs(cfg, v0, a0, samples[k])
            verdicts.append(tc.judge(rays, co, 0.0, samples[k][3], 0.1)["verdict"])
            planner_free.append(free)
    verdicts, planner_free = np.array(verdicts), np.array(planner_free)
    assert len(verdicts) == 480
    share = [np.mean(verdicts == v) for v in (0, 1, 2)]
    print("verdict shares free / out of view / occluded:", share, "planner-free:", int(planner_free.sum()),
          "rejected but free:", int((~planner_free & (verdicts == 0)).sum()))
    assert min(share) >= 0.05, share
    assert planner_free.sum() >= 100
    assert np.all(verdicts[planner_free] == 0), np.flatnonzero(planner_free & (verdicts != 0))
