"""First-hit ray queries on the device (afe_raycast, afe_raycast_stats, afe_line_of_sight) against the numpy statement of
the definition (tests/raycast_checker.py): t as its 64 bits, and the triangle.  The checker tests every ray against every
triangle, so any bit the kernel's boxes changed shows here."""
import ctypes as C
import importlib

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from tests import raycast_checker as rc
from tests import raycast_scenes as scenes
from tests import render_scenes as rs

afa = importlib.import_module("agri-fly_amd")
pytestmark = pytest.mark.gpu
INF = np.inf
SCENE_NAMES = sorted(scenes.SCENES)

_MAPS, _RAYS = {}, {}


@pytest.fixture(scope="module")
def maps():
    def get(name):
        if name not in _MAPS:
            _MAPS[name] = afa.ClearanceMap(scenes.scene(name))
        return _MAPS[name]
    yield get
    for m in _MAPS.values():
        m.close()
    _MAPS.clear()


def rays(name, kind):
    """the rays of a scene and the checker's answers to them, computed once: origin, dir, t, tri"""
    if (name, kind) not in _RAYS:
        tris = scenes.scene(name)
        o, d = scenes.random_rays(tris) if kind == "random" else scenes.structured_rays(tris)
        _RAYS[(name, kind)] = (o, d) + rc.raycast(tris, o, d)
    return _RAYS[(name, kind)]


@pytest.mark.parametrize("kind", ["random", "structured"])
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_bit_parity(maps, name, kind):
    o, d, want_t, want_tri = rays(name, kind)
    t, tri, ms = maps(name).raycast(o, d, want_ms=True)
    hits = int((want_tri >= 0).sum())
    print("%s %s: %d rays x %d triangles, %d hits, kernel %.3f ms" % (name, kind, o.shape[1], len(scenes.scene(name)), hits, ms))
    assert 0 < hits < o.shape[1]                       # both answers are asked for
    rc.assert_same_bits(t, tri, want_t, want_tri, "%s %s" % (name, kind))
    # +inf for every ray is NULL
    t2, tri2 = maps(name).raycast(o, d, INF)
    rc.assert_same_bits(t2, tri2, want_t, want_tri, "%s %s t_max = +inf" % (name, kind))


def test_coincident_copies_report_the_first(maps):
    o, d, want_t, want_tri = rays("coincident", "random")
    assert (want_tri[want_tri >= 0] < 300).any() and not ((want_tri > 0) & (want_tri < 300)).any()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_ray_counts(maps, n):
    o, d, want_t, want_tri = rays("orchard", "random")
    t, tri = maps("orchard").raycast(o[:, 5:5 + n], d[:, 5:5 + n])
    rc.assert_same_bits(t, tri, want_t[5:5 + n], want_tri[5:5 + n], "n = %d" % n)


@pytest.mark.parametrize("name", ["orchard", "lattice"])
def test_t_max_per_ray(maps, name):
    """a third of the rays limited to exactly their true t (still a hit), a third to the double below it (the next triangle
    behind it does not count either: the limit is on t, not on the winner), the rest to 0.5, 0 and +inf"""
    tris = scenes.scene(name)
    o, d, t_true, _ = rays(name, "random")
    n = o.shape[1]
    k = np.arange(n)
    tm = np.where(k % 3 == 0, t_true, np.where(k % 3 == 1, np.nextafter(t_true, 0.0), np.choose(k % 9 // 3, [0.5, 0.0, INF])))
    tm = np.where(np.isfinite(tm) | (k % 3 == 2), tm, 7.0)
    want_t, want_tri = rc.raycast(tris, o, d, tm)
    at = (k % 3 == 0) & np.isfinite(t_true)
    assert at.sum() > 100 and (want_t[at] == t_true[at]).all()
    below = (k % 3 == 1) & np.isfinite(t_true)
    assert (want_tri[below] == -1).all()
    t, tri = maps(name).raycast(o, d, tm)
    rc.assert_same_bits(t, tri, want_t, want_tri, name)


@pytest.mark.parametrize("name", ["orchard", "hanging", "lattice"])
def test_counting_build(maps, name):
    o, d, want_t, want_tri = rays(name, "random")
    st, ms = maps(name).raycast_stats(o, d)
    n, T = o.shape[1], len(scenes.scene(name))
    print("%s: per ray %.1f nodes, %.1f box tests, %.2f fp64 tests (brute force: %d)" % (
        name, st["nodes"] / n, st["tri_box_tests"] / n, st["tri_fp64_tests"] / n, T))
    assert st["rays"] == n
    assert st["tri_fp64_tests"] <= st["tri_box_tests"] < n * T
    assert st["tri_fp64_tests"] >= int((want_tri >= 0).sum())          # every hit was at least tested
    if T > 100:
        assert st["tri_box_tests"] < n * T // 4 and st["nodes"] > 0


def test_counting_build_gives_the_same_answers(maps):
    """the counting instantiation is a second compilation of the walk: the same bits, with and without a limit"""
    for name in ("orchard", "coincident"):
        o, d, want_t, want_tri = rays(name, "structured")
        st, _, t, tri = maps(name).raycast_stats(o, d, want_answers=True)
        rc.assert_same_bits(t, tri, want_t, want_tri, name + " counting build")
        assert st["rays"] == o.shape[1]
        tm = np.where(np.isfinite(want_t), want_t, 1.0)
        _, _, t2, tri2 = maps(name).raycast_stats(o, d, tm, want_answers=True)
        rc.assert_same_bits(t2, tri2, *rc.raycast(scenes.scene(name), o, d, tm), what=name + " counting build, t_max")
    # without outputs (NULL): the counts alone, the same
    L = afa.library()
    o, d, _, _ = rays("orchard", "structured")
    st1, _ = maps("orchard").raycast_stats(o, d)
    raw = np.zeros(4, np.uint64)
    assert L.afe_raycast_stats(maps("orchard").handle, o.shape[1], o.ctypes.data, d.ctypes.data, None, None, None, raw.ctypes.data, None) == 0
    assert [int(x) for x in raw] == [st1[k] for k in ("nodes", "tri_box_tests", "tri_fp64_tests", "rays")]


def _views():
    tilt = rs.quat_mul(rs.yaw(20), rs.pitch(-8))
    return [("lattice", rs.Cam(64, 48, focal=24.0), (0.0, 0.0, 1.0), rs.IDENT),          # every ray on a lattice line or vertex
            ("hanging", rs.Cam(64, 48, focal=28.0), (0.1, 0.2, 1.4), tilt),
            ("orchard", rs.Cam(64, 48, focal=22.0, cx=30.3, cy=25.7, depth_scale=0.05, max_count=1000), (-1.0, 0.5, 1.3),
             rs.quat_mul(rs.yaw(-35), rs.roll(12)))]


@pytest.mark.parametrize("name,cam,pos,att", _views(), ids=[v[0] for v in _views()])
def test_the_camera_agrees(maps, name, cam, pos, att):
    """afe_render_depth walks its own tree (pair nodes, inflated boxes, 64 coherent rays) with the same ray/triangle rule:
    its counts are the quantised t of afe_raycast on the pixel rays"""
    tris = scenes.scene(name)
    scene = afa.Scene(tris)
    img, _ = scene.render(cam.afa(afa), np.array(pos, float).reshape(3, 1), np.array(att, float).reshape(4, 1), rs.MOUNT)
    scene.close()
    o, d = rc.pixel_rays(cam, pos, att, rs.MOUNT)
    t, tri = maps(name).raycast(o, d)
    with np.errstate(invalid="ignore"):
        want = np.where(np.isfinite(t), np.minimum(np.floor(np.where(np.isfinite(t), t, 0.0) / cam.depth_scale), cam.max_count), cam.max_count)
    assert (want < cam.max_count).sum() > 500
    assert_array_equal(np.asarray(img[0]).reshape(-1).astype(np.int64), want.astype(np.int64))


def _los_pairs():
    tris = scenes.scene("orchard")
    rng = np.random.default_rng(7)
    v = tris.reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    n = 4096
    p0 = rng.uniform(lo - [1, 1, 0], hi + [1, 1, 1], (n, 3)).T
    p0[2] = np.abs(p0[2]) + 0.05
    p1 = rng.uniform(lo - [1, 1, 0], hi + [1, 1, 1], (n, 3)).T
    p1[2] = np.abs(p1[2]) + 0.05
    near = np.arange(n) % 4 == 1                      # short hops, mostly clear
    p1[:, near] = p0[:, near] + rng.normal(0, 0.3, (3, int(near.sum())))
    p1[:, 0:8] = p0[:, 0:8]                            # p0 == p1
    # ending exactly on the ground (z = 0, the two big triangles kept out of the tree), straight down from 2 m at a dyadic
    # place with nothing in between: every product is exact, t = 1 exactly
    cand = np.round(rng.uniform(lo + 0.5, hi - 0.5, (400, 3)).T * 8) / 8
    cand[2] = 2.0
    t_c = rc.pair_t(tris, cand, np.array([[0.0], [0.0], [-2.0]]) * np.ones((1, 400))).min(1)
    cand = cand[:, t_c == 1.0][:, :16]
    assert cand.shape[1] == 16
    p0[:, 8:24] = cand
    p1[:, 8:24] = cand
    p1[2, 8:24] = 0.0
    # ending exactly where a first-hit ray lands (t = 1 up to the roundings of p0 + d t: either answer, but the same)
    o, d, t_true, _ = rc_rays_from(p0[:, 24:280], rng)
    p1[:, 24:280] = np.where(np.isfinite(t_true), o + d * np.where(np.isfinite(t_true), t_true, 0.0), p1[:, 24:280])
    for k, bad in enumerate((np.nan, np.inf, -np.inf)):
        p0[k, 300 + k] = bad
        p1[(k + 1) % 3, 310 + k] = bad
    return np.ascontiguousarray(p0), np.ascontiguousarray(p1)


def rc_rays_from(p0, rng):
    d = rng.normal(size=p0.shape)
    t, tri = rc.raycast(scenes.scene("orchard"), p0, d)
    return p0, d, t, tri


def test_line_of_sight(maps):
    tris = scenes.scene("orchard")
    p0, p1 = _los_pairs()
    want = rc.line_of_sight(tris, p0, p1)
    got, ms = maps("orchard").line_of_sight(p0, p1, want_ms=True)
    print("line of sight: %d pairs, %d blocked, kernel %.3f ms" % (want.size, int(want.sum()), ms))
    assert 400 < want.sum() < want.size - 400
    assert_array_equal(got, want)
    assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 1}
    # the any-hit kernel answers what the first-hit kernel answers
    with np.errstate(invalid="ignore"):
        t, tri = maps("orchard").raycast(p0, p1 - p0, 1.0)
    assert_array_equal(got, (t <= 1.0).astype(np.uint8))
    assert_array_equal(got, (tri >= 0).astype(np.uint8))
    assert (got[0:8] == 0).all()                        # p0 == p1
    t1 = rc.pair_t(tris, p0[:, 8:24], (p1 - p0)[:, 8:24]).min(1)
    assert (t1 == 1.0).all() and (got[8:24] == 1).all()    # touching the ground at t = 1 exactly: blocked
    assert (got[300:303] == 0).all() and (got[310:313] == 0).all()   # a non-finite end
    for n in (1, 65, 257):
        assert_array_equal(maps("orchard").line_of_sight(p0[:, :n], p1[:, :n]), want[:n])


def test_non_finite_and_zero_rays(maps):
    o, d, _, _ = rays("orchard", "random")
    o, d = o[:, :700].copy(), d[:, :700].copy()
    bad = {3: (0, np.nan), 64: (1, np.inf), 65: (2, -np.inf), 255: (3, -np.inf), 256: (5, np.nan), 699: (4, np.inf)}
    for k, (c, val) in bad.items():
        (o if c < 3 else d)[c % 3, k] = val
    d[:, 100] = 0.0
    d[:, 101] = -0.0
    want_t, want_tri = rc.raycast(scenes.scene("orchard"), o, d)
    t, tri = maps("orchard").raycast(o, d)
    rc.assert_same_bits(t, tri, want_t, want_tri, "non-finite")
    for k in list(bad) + [100, 101]:
        assert t[k] == INF and tri[k] == -1


def test_boundary(maps):
    L = afa.library()
    m = maps("orchard")
    o, d, want_t, want_tri = rays("orchard", "random")
    n = 300
    o, d = np.ascontiguousarray(o[:, :n]), np.ascontiguousarray(d[:, :n])
    t, tri = np.full(n, -7.0), np.full(n, -7, np.int32)
    blocked = np.full(n, 9, np.uint8)
    st = np.zeros(4, np.uint64)
    tm = np.full(n, 3.0)

    def cast(**kw):
        a = dict(m=m.handle, n=n, o=o.ctypes.data, d=d.ctypes.data, tm=None, t=t.ctypes.data, tri=tri.ctypes.data)
        a.update(kw)
        return L.afe_raycast(a["m"], a["n"], a["o"], a["d"], a["tm"], a["t"], a["tri"], None)

    def stats(**kw):
        a = dict(m=m.handle, n=n, o=o.ctypes.data, d=d.ctypes.data, tm=None, st=st.ctypes.data)
        a.update(kw)
        return L.afe_raycast_stats(a["m"], a["n"], a["o"], a["d"], a["tm"], None, None, a["st"], None)

    def los(**kw):
        a = dict(m=m.handle, n=n, o=o.ctypes.data, d=d.ctypes.data, out=blocked.ctypes.data)
        a.update(kw)
        return L.afe_line_of_sight(a["m"], a["n"], a["o"], a["d"], a["out"], None)

    for call in (cast, stats, los):
        assert call(m=None) == 1 and call(o=None) == 1 and call(d=None) == 1
        assert call(n=-1) == 1 and call(n=-2 ** 63) == 1 and call(n=2 ** 62) == 4
    assert cast(t=None) == 1 and cast(tri=None) == 1 and stats(st=None) == 1 and los(out=None) == 1
    assert cast(n=0) == 0 and los(n=0) == 0 and stats(n=0) == 1
    for bad in (np.nan, -1.0, -np.inf, -1e-300):
        tm[17] = bad
        assert cast(tm=tm.ctypes.data) == 4 and stats(tm=tm.ctypes.data) == 4
    assert (t == -7.0).all() and (tri == -7).all() and (blocked == 9).all()      # a refusal writes nothing
    tm[17] = 0.0                                                                  # 0 and -0 are valid limits: nothing is hit
    tm[18] = -0.0
    assert cast(tm=tm.ctypes.data) == 0
    want = rc.raycast(scenes.scene("orchard"), o, d, tm)
    rc.assert_same_bits(t, tri, want[0], want[1], "after the refusals")
    assert tri[17] == -1 and tri[18] == -1
