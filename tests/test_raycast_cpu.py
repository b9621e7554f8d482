"""The ray query's numpy checker (tests/raycast_checker.py) is the depth camera's rule: bit for bit the existing oracle on
the camera's own rays, inside the exact-geometry judge's bounds, and right on the cases one can work out by hand."""
from fractions import Fraction

import numpy as np
import pytest

from tests import raycast_checker as rc
from tests import raycast_scenes as scenes
from tests import render_judge as rj
from tests import render_scenes as rs

INF = np.inf


def _views():
    # focal 12 at 3 m from a 1/4 m lattice: EVERY pixel's ray runs through a lattice vertex or along a lattice line
    tilt = rs.quat_mul(rs.yaw(20), rs.pitch(-8))
    return [rs.View("rays: lattice, axis-aligned", rs.Cam(32, 24, focal=12.0, depth_scale=2.0 ** -20, max_count=1 << 30), scenes.scene("lattice"),
                    (0.0, 0.0, 1.0), rs.IDENT, rs.MOUNT, all_hit=True),
            rs.View("rays: hanging rectangles", rs.Cam(32, 24, focal=14.0, depth_scale=2.0 ** -20, max_count=1 << 30), scenes.scene("hanging"),
                    (0.1, 0.2, 1.4), tilt, rs.MOUNT),
            rs.View("rays: orchard 2x2", rs.Cam(32, 24, focal=11.0, cx=15.3, cy=12.7, depth_scale=2.0 ** -20, max_count=1 << 30), scenes.scene("orchard"),
                    (-1.0, 0.5, 1.3), rs.quat_mul(rs.yaw(-35), rs.roll(12)), rs.MOUNT),
            rs.View("rays: 300 coincident", rs.Cam(32, 24, focal=16.0, depth_scale=2.0 ** -20, max_count=1 << 30), scenes.scene("coincident"),
                    (0.0, 0.0, 1.0), rs.IDENT, rs.MOUNT)]


VIEWS = _views()
_ANSWERS = {}


def answers(view):
    """the checker on the view's pixel rays, once: origin, dir, t, tri"""
    if view.name not in _ANSWERS:
        o, d = rc.pixel_rays(view.cam, view.pos, view.att, view.mount)
        _ANSWERS[view.name] = (o, d) + rc.raycast(view.tris, o, d)
    return _ANSWERS[view.name]


@pytest.mark.parametrize("view", VIEWS, ids=repr)
def test_checker_is_the_cameras_oracle_on_pixel_rays(ora, view):
    o, d, t, tri = answers(view)
    cam = view.cam.ora(ora)
    want = np.array([ora.render_pixel_depth(cam, view.tris, view.pos, view.att, view.mount, px, py)
                     for py in range(cam.height) for px in range(cam.width)])
    assert np.array_equal(t.view(np.uint64), want.view(np.uint64)), "%d of %d pixels differ" % ((t != want).sum(), t.size)
    assert np.isfinite(t).any()
    if view.all_hit:
        assert np.isfinite(t).all()
    else:
        assert np.isinf(t).any()
    assert ((tri >= 0) == np.isfinite(t)).all()


def _F(x):
    return Fraction(*float(x).as_integer_ratio())


def _exact_pair(tri9, o, d):
    """u, v, w, t of the ray (o, d: the doubles themselves) against the triangle, in Fractions; None: det == 0"""
    v0 = [_F(x) for x in tri9[0:3]]
    e1 = [_F(tri9[3 + k]) - v0[k] for k in range(3)]
    e2 = [_F(tri9[6 + k]) - v0[k] for k in range(3)]
    dd, tv = [_F(x) for x in d], [_F(o[k]) - v0[k] for k in range(3)]
    p = rj._cross(dd, e2)
    det = rj._dot(e1, p)
    if det == 0:
        return None
    q = rj._cross(tv, e1)
    u, v, t = rj._dot(tv, p) / det, rj._dot(dd, q) / det, rj._dot(e2, q) / det
    E = max(sum(abs(x) for x in e1), sum(abs(x) for x in e2))
    T, D = sum(abs(x) for x in tv), sum(abs(x) for x in dd)
    K, K_t = D * E * (T + E), T * E * E
    delta = Fraction(rj.C_TOL) * K / abs(det)
    n_t = abs(rj._dot(e2, q))
    tau = (Fraction(rj.C_TOL) * (K_t / n_t + K / abs(det)) + Fraction(rj.TAU_FLOOR)) if n_t else None
    return u, v, 1 - u - v, t, delta, tau


@pytest.mark.parametrize("view", VIEWS, ids=repr)
def test_checker_against_exact_geometry(view):
    """The judge knows only the geometry.  t lies between its dilated and its exact depth (each with the judge's tau): no
    leak through a shared edge or a vertex, nothing seen nearer than a delta-grown silhouette.  And the triangle reported is
    one of the delta-grown set at that depth: judged here, pair by pair, in exact arithmetic on the ray's own doubles."""
    o, d, t, tri = answers(view)
    j = rs.judged(view)
    z_lo, z_hi = j.z_lo.reshape(-1), j.z_hi.reshape(-1)
    bad = ~((t >= z_lo) & (t <= z_hi))
    assert not bad.any(), "%d rays outside the judge's bounds, first %d: t %r not in [%r, %r]" % (
        bad.sum(), np.flatnonzero(bad)[0], t[bad][0], z_lo[bad][0], z_hi[bad][0])
    if view.all_hit:
        assert np.isfinite(z_hi).all()              # the judge demands a hit everywhere: a leak would have failed above
    for i in np.flatnonzero(tri >= 0):
        res = _exact_pair(view.tris[tri[i]].astype(np.float64), o[:, i], d[:, i])
        assert res is not None, i
        u, v, w, t_exact, delta, tau = res
        assert u >= -delta and v >= -delta and w >= -delta, (i, float(u), float(v), float(w), float(delta))
        assert tau is not None and abs(_F(t[i]) - t_exact) <= tau * abs(t_exact), (i, t[i], float(t_exact), float(tau))


def test_hand_cases():
    tri = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], np.float32)                    # in the plane z = 0
    col = lambda *p: np.array(p, np.float64).reshape(3, 1)
    # straight down onto it from 2 m: t = 2 exactly (every operand is a small integer)
    t, k = rc.raycast(tri, col(0.25, 0.25, 2), col(0, 0, -1))
    assert t[0] == 2.0 and k[0] == 0
    # t is the ray PARAMETER: a direction four times as long gives a quarter of it
    assert rc.raycast(tri, col(0.25, 0.25, 2), col(0, 0, -4))[0][0] == 0.5
    # origin ON the triangle: no hit (t > 0 is required), whichever way the ray goes
    for d in ((0, 0, -1), (0, 0, 1), (1, 0, 0)):
        t, k = rc.raycast(tri, col(0.25, 0.25, 0), col(*d))
        assert t[0] == INF and k[0] == -1
    # pointing away
    assert rc.raycast(tri, col(0.25, 0.25, 2), col(0, 0, 1))[1][0] == -1
    # zero direction (+0 and -0)
    for z in (0.0, -0.0):
        t, k = rc.raycast(tri, col(0.25, 0.25, 2), col(z, z, z))
        assert t[0] == INF and k[0] == -1
    # non-finite inputs: the same answer
    for bad in (np.nan, np.inf, -np.inf):
        for which in range(6):
            o, d = col(0.25, 0.25, 2), col(0, 0, -1)
            (o if which < 3 else d)[which % 3, 0] = bad
            t, k = rc.raycast(tri, o, d)
            assert t[0] == INF and k[0] == -1
    # t_max: exactly the hit's t is a hit, the next double below is not; 0 and +inf
    assert rc.raycast(tri, col(0.25, 0.25, 2), col(0, 0, -1), 2.0)[1][0] == 0
    assert rc.raycast(tri, col(0.25, 0.25, 2), col(0, 0, -1), np.nextafter(2.0, 0.0))[1][0] == -1
    assert rc.raycast(tri, col(0.25, 0.25, 2), col(0, 0, -1), 0.0)[1][0] == -1
    assert rc.raycast(tri, col(0.25, 0.25, 2), col(0, 0, -1), INF)[0][0] == 2.0
    # the closed triangle: through a vertex and along... an edge's point, from above
    for p in ((0, 0), (1, 0), (0, 1), (0.5, 0.5), (0.5, 0), (0, 0.5)):
        assert rc.raycast(tri, col(p[0], p[1], 1), col(0, 0, -1))[0][0] == 1.0
    assert rc.raycast(tri, col(0.75, 0.75, 1), col(0, 0, -1))[1][0] == -1
    # a tie: two triangles in the same plane sharing the edge the ray meets, and two coincident ones: the lower index wins
    pair = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0], [1, 0, 0, 1, 1, 0, 0, 1, 0]], np.float32)
    for order in ((0, 1), (1, 0)):
        t, k = rc.raycast(pair[list(order)], col(0.5, 0.5, 3), col(0, 0, -1))
        assert t[0] == 3.0 and k[0] == 0
    t, k = rc.raycast(np.repeat(tri, 5, 0), col(0.25, 0.25, 2), col(0, 0, -1))
    assert t[0] == 2.0 and k[0] == 0
    # ... and the nearer one wins whatever its index
    stack = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1, 1, 0, 1, 0, 1, 1]], np.float32)
    t, k = rc.raycast(stack, col(0.25, 0.25, 2), col(0, 0, -1))
    assert t[0] == 1.0 and k[0] == 1
    # degenerate triangles hit nothing: a point, two coincident vertices, collinear -- aimed straight at them
    junk = scenes.degenerate_scene()[1::2][:4]
    for g in junk:
        v = g.reshape(3, 3).astype(np.float64)
        for target in (v[0], v[2], (v[0] + v[1] + v[2]) / 3.0):
            for eye in ((5.0, 4.0, 3.0), (-3.0, 0.5, 0.25)):
                t, k = rc.raycast(g[None], col(*eye), (target - np.array(eye)).reshape(3, 1))
                assert t[0] == INF and k[0] == -1


def test_line_of_sight_by_hand():
    tri = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], np.float32)
    col = lambda *p: np.array(p, np.float64).reshape(3, 1)
    assert rc.line_of_sight(tri, col(0.25, 0.25, 1), col(0.25, 0.25, -1))[0] == 1       # through it
    assert rc.line_of_sight(tri, col(0.25, 0.25, 1), col(0.25, 0.25, 0))[0] == 1        # touching it at t = 1 exactly
    assert rc.line_of_sight(tri, col(0.25, 0.25, 1), col(0.25, 0.25, 0.5))[0] == 0      # stopping short
    assert rc.line_of_sight(tri, col(0.25, 0.25, 0), col(0.25, 0.25, 1))[0] == 0        # starting on it
    assert rc.line_of_sight(tri, col(0.25, 0.25, 1), col(0.25, 0.25, 1))[0] == 0        # p0 == p1
    assert rc.line_of_sight(tri, col(0.25, 0.25, np.nan), col(0.25, 0.25, -1))[0] == 0
    assert rc.line_of_sight(tri, col(0.25, 0.25, 1), col(0.25, np.inf, -1))[0] == 0


def test_sensor_rays_by_hand():
    """identity attitude and mount: the sensor frame is the world frame; a quarter turn about z carries +x to +y"""
    beams = np.zeros(2, rc.BEAM_DTYPE)
    beams["off"] = [(0.5, 0.0, 0.0), (0.5, 0.0, 0.0)]
    beams["dir"] = [(1.0, 0.0, 0.0), (1.0, 0.0, 0.0)]
    beams["frame"] = [0, 1]
    pos = np.array([[1.0, 1.0], [2.0, 2.0], [3.0, 3.0]])
    h = np.sqrt(0.5)
    att = np.array([[1.0, h], [0.0, 0.0], [0.0, 0.0], [0.0, h]])
    o, d = rc.sensor_rays(pos, att, beams)
    np.testing.assert_allclose(o[0, :, 0], [1.5, 2, 3], atol=1e-15)
    np.testing.assert_allclose(d[0, :, 0], [1, 0, 0], atol=1e-15)
    np.testing.assert_allclose(o[0, :, 1], [1, 2.5, 3], atol=1e-15)                      # turned with the body
    np.testing.assert_allclose(d[0, :, 1], [0, 1, 0], atol=1e-15)
    np.testing.assert_array_equal(o[1, :, 1], [1.5, 2, 3])                               # levelled: the world's axes
    np.testing.assert_array_equal(d[1, :, 1], [1, 0, 0])


def test_python_surface_without_a_gpu(afa):
    beams = afa.crazyflie_range_beams()
    assert beams.dtype == afa.RANGE_BEAM_DTYPE and beams.dtype.itemsize == 64 and beams.shape == (6,)
    assert beams.dtype == rc.BEAM_DTYPE
    assert (beams["t_max"] == 4.0).all() and (beams["frame"] == afa.RANGE_FRAME_SENSOR).all() and (beams["off"] == 0).all()
    assert sorted(map(tuple, beams["dir"])) == sorted([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)])
    assert tuple(beams["dir"][5]) == (0, 0, -1)                                          # the z-ranger looks down, last
    L = afa.library()
    for name in ("afe_raycast", "afe_raycast_stats", "afe_line_of_sight", "afe_range_sensor_create", "afe_range_sensor_update",
                 "afe_range_sensor_info", "afe_range_sensor_destroy"):
        assert name in afa.ABI_FUNCTIONS and getattr(L, name).argtypes is not None
    # all-NULL / all-zero arguments are refused without a device
    assert L.afe_raycast(None, 0, None, None, None, None, None, None) == 1
    assert L.afe_raycast_stats(None, 0, None, None, None, None, None, None, None) == 1
    assert L.afe_line_of_sight(None, 0, None, None, None, None) == 1
    assert L.afe_range_sensor_create(None, None, None, None, 0, None) == 1
    assert L.afe_range_sensor_update(None, 0, 0, None, None, 0, None) == 1
    assert L.afe_range_sensor_info(None, None, None) == 1
    assert L.afe_range_sensor_destroy(None) == 1
