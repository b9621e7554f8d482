"""The depth camera's checker (oracle/agrifly_oracle_render.c) held to exact geometry (tests/render_judge.py).

First the judge itself against closed forms -- planes and the inside of a box -- which is what keeps the judge
honest; then every pixel of every scene of tests/render_scenes.py as the checker renders it.  The kernel is
required to equal the checker bit for bit (tests/test_gpu_render.py, tests/test_gpu_render_judged.py), so what
passes here is what the GPU computes.

With the two-sided open edge rule the checker had before (u < 0 || u > 1, v < 0 || u + v > 1 per triangle in
rounded fp64) these scenes failed: see test_lattice_walls for the counts."""
import numpy as np
import pytest

from tests import render_judge, render_scenes as rs


@pytest.fixture(scope="module")
def scen(afa):
    return afa.scenarios


def _rays(view):
    cam = view.cam
    R = rs.quat_matrix(rs.quat_mul(view.att, view.mount))
    px, py = np.meshgrid(np.arange(cam.width), np.arange(cam.height))
    cam_rays = np.stack([(px - cam.cx) / cam.focal_length, (py - cam.cy) / cam.focal_length, np.ones(px.shape)], -1)
    return cam_rays @ R.T


# ------------------------------------------------------------------------------------------------
# the judge against closed forms
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tilt_deg,az_deg,pos", [(0.0, 0.0, (0.0, 0.0, 0.0)), (35.0, 20.0, (0.3, -1.7, 0.9)),
                                                 (70.0, -115.0, (-2.0, 0.25, 4.0)), (55.0, 200.0, (1e-3, 5.0, -3.0))])
def test_judge_plane_closed_form(tilt_deg, az_deg, pos):
    """A plane filling the field of view: z = n . (P0 - o) / (n . d), with n and P0 of the float32 triangle hit."""
    t, a = np.deg2rad(tilt_deg), np.deg2rad(az_deg)
    n = np.array([-np.cos(t), np.sin(t) * np.cos(a), np.sin(t) * np.sin(a)])        # faces the camera that looks along +x
    p0 = np.asarray(pos) + [2.5, 0.0, 0.0]
    e_a = np.cross(n, [0.0, 0.3, 1.0]); e_a /= np.linalg.norm(e_a)
    e_b = np.cross(n, e_a)
    plane = rs.quad(p0 - 300.0 * e_a - 300.0 * e_b, 600.0 * e_a, 600.0 * e_b)
    view = rs.View("plane", rs.Cam(24, 18, focal=40.0, cx=11.3, cy=9.6), plane, pos, rs.IDENT, rs.MOUNT)
    j = render_judge.judge(view.cam, view.tris, view.pos, view.att, view.mount)
    d = _rays(view)
    assert (j.tri >= 0).all()
    T = view.tris.astype(np.float64)[j.tri]                                     # the triangle each pixel hit
    v0, nn = T[..., 0:3], np.cross(T[..., 3:6] - T[..., 0:3], T[..., 6:9] - T[..., 0:3])
    z = np.einsum("...k,...k", nn, v0 - view.pos) / np.einsum("...k,...k", nn, d)
    assert np.all(z > 0)
    np.testing.assert_allclose(j.z_exact, z, rtol=1e-12)
    np.testing.assert_allclose(j.z_dilated, z, rtol=1e-12)
    assert np.all(j.z_lo <= j.z_exact) and np.all(j.z_exact <= j.z_hi) and np.all(j.z_hi <= j.z_exact * (1 + 1e-9))
    assert np.all(j.z_lo >= j.z_exact * (1 - 1e-9))


@pytest.mark.parametrize("att", [rs.IDENT, rs.yaw(90), rs.pitch(90), np.array([0.8, 0.1, -0.5, 0.3])], ids=["ident", "yaw90", "down", "generic"])
@pytest.mark.parametrize("pos", [(0.0, 0.0, 1.25), (0.5, -1.25, 2.0)])
def test_judge_box_closed_form(att, pos):
    """From inside an axis-aligned box the depth of a ray is the nearest of the three faces ahead of it:
    z = min_k ((d_k > 0 ? hi_k : lo_k) - o_k) / d_k.  Rays into the corners and along the edges included."""
    lo, hi = np.array([-2, -2, 0.0]), np.array([2, 2, 2.5])
    view = rs.View("box", rs.Cam(33, 21, focal=8.0, cx=16.0, cy=10.0), rs.closed_box(lo, hi), pos, att, rs.MOUNT)
    j = render_judge.judge(view.cam, view.tris, view.pos, view.att, view.mount)
    d = _rays(view)
    with np.errstate(divide="ignore", invalid="ignore"):
        tk = np.where(d > 0, (hi - view.pos) / d, np.where(d < 0, (lo - view.pos) / d, np.inf))
    z = tk.min(-1)
    np.testing.assert_allclose(j.z_exact, z, rtol=1e-12)
    np.testing.assert_allclose(j.z_dilated, z, rtol=1e-12)
    assert (j.tri >= 0).all()
    u, v = j.bary[..., 0], j.bary[..., 1]
    assert np.all(u >= 0) and np.all(v >= 0) and np.all(u + v <= 1 + 1e-15)


def test_judge_refuses_leaks_and_lost_triangles_and_allows_ties():
    """What the pass rule means, on a wall 40 counts away in front of a wall at 90."""
    cam = rs.Cam(8, 6)
    x = np.float32(40 * rs.SCALE)
    tris = np.concatenate([rs.quad((x, -50.0, -50.0), (0, 100.0, 0), (0, 0, 100.0)), rs.quad((3.5, -50.0, -50.0), (0, 100.0, 0), (0, 0, 100.0))])
    j = render_judge.judge(cam, tris, (0, 0, 0), rs.IDENT, rs.MOUNT)
    good = np.full((6, 8), 40)
    assert j.passes(good).all() and j.passes(good - 1).all()            # the tie at an exact multiple may fall either way
    assert not j.passes(good - 2).any() and not j.passes(good + 1).any()
    leak = good.copy()
    leak[2, 3], leak[4, 4] = 89, 255                                    # the wall behind, or nothing: both seen through the first
    f = j.failures(leak)
    assert [(px, py, got) for px, py, got, *_ in f] == [(3, 2, 89), (4, 4, 255)]
    px, py, got, z_dil, z_ex, tri, (u, v) = f[0]
    assert z_dil <= z_ex and abs(z_ex - float(x)) < 1e-12 and tri in (0, 1) and 0 <= u <= 1 and 0 <= v <= 1
    with pytest.raises(AssertionError, match="2 of 48 pixels fail"):
        render_judge.assert_passes(j, leak)
    # a degenerate triangle and an exactly edge-on one hit nothing
    flat = np.array([[1, 0, 0, 1, 1, 1, 1, 2, 2], [1, 0, -5, 2, 0, 5, 3, 0, -5]], np.float32)
    j = render_judge.judge(cam, flat, (0, 0, 0), rs.IDENT, rs.IDENT)    # identity mount: exact axes, y = 0 is edge-on for row 3
    assert np.isinf(j.z_exact[3]).all() and np.isinf(j.z_dilated[3]).all() and (j.count_hi == 255).all()


# ------------------------------------------------------------------------------------------------
# the checker against the judge
# ------------------------------------------------------------------------------------------------
def _judge_checker(ora, views):
    failing = {}
    for v in views:
        img = rs.checker_image(ora, v)
        j = rs.judged(v)
        bad = int((~j.passes(img)).sum())
        if bad:
            failing[v.name] = (bad, j.explain(img, limit=3))
        if v.all_hit:
            assert (j.count_hi < v.cam.max_count).all(), v.name        # the judge agrees that nothing may be missed
    assert not failing, "%d scenes fail: " % len(failing) + "\n".join("%s: %s" % kv for kv in failing.items())


def test_lattice_walls(ora):
    """Walls on 1/16, 1/8 and 1/32 m lattices seen by axis-aligned cameras from whole-metre positions: every pixel ray
    runs along mesh edges and through vertices, and a second wall stands 2 m behind.  With the open edge rule 6 of these
    60 views failed, 158 pixels in all, every one reading the wall behind: the 1/16 m wall at 3 m from the origin through
    the default mount at yaw 90 / 180 / 270 deg (49, 57 and 49 of 1 728 pixels) and straight down (1), and the 1/8 m and
    1/32 m walls at yaw 180 deg (1 of 432 each).  A quarter-turn's cos 45 deg is not a double, so the rotation is a
    permutation only up to 1e-16 and the two triangles at an edge round apart."""
    _judge_checker(ora, rs.lattice_views())


def test_centred_box_and_icosphere(ora, scen):
    """From inside a closed convex mesh every pixel must hit: rays into the corners and along all twelve edges of the box
    (from its centre, and from the (0, 0, 1) of test_gpu_render.py::test_degenerate_meshes without that test's step aside:
    with the open edge rule pixel (0, 25) of that view looked out through a corner and read 255), through the vertices of
    an icosphere."""
    _judge_checker(ora, rs.box_views() + rs.icosphere_views(scen))


def test_degenerate_mesh_sliver_along_its_edge(ora):
    """The coincident / sliver / zero-area mesh of test_gpu_render.py::test_degenerate_meshes, where the engine is compared with
    the checker bit for bit.  Row 15 runs along the lower edge of the sliver at x = 2 m (51 counts).  Pixels 11 .. 29 hit it
    exactly and must read 51.  The rays of pixels (10, 15) and (30, 15) pass its end vertices 1e-16 m outside (the default
    mount is a permutation only up to 1e-16): the geometry says miss, the delta-grown sliver says hit, the judge takes either.
    The open edge rule read 255 there and the tolerant closed rule reads 51 -- the only two pixels of any image compared in
    that file that the closed rule changed."""
    view = rs.degenerate_view()
    j = rs.judged(view)
    assert (j.count_hi[15, 11:30] == 51).all() and (j.count_lo[15, 10:31] == 51).all()
    assert (j.count_hi[15, [10, 30]] == 255).all() and np.isinf(j.z_exact[15, [10, 30]]).all() and np.allclose(j.z_dilated[15, [10, 30]], 2.0, rtol=1e-12, atol=0)
    assert (j.count_lo[15, :10] == 255).all() and (j.count_lo[15, 31:] == 255).all()
    img = rs.checker_image(ora, view)
    assert (img[15, 10:31] == 51).all()
    _judge_checker(ora, [view])


def test_generic_views(ora, scen):
    """Nothing aligned with anything: random tilts up to 80 deg, off-centre principal point, odd sizes down to 1 x 1,
    a small orchard."""
    _judge_checker(ora, rs.generic_views(scen))


def test_quantisation(ora):
    _judge_checker(ora, rs.quantisation_views())


def test_grazing_incidence_and_scale(ora):
    """Centimetre triangles seen at a third of a degree, and the closed box at 2^-24 of its size: a determinant cutoff
    has to scale with the operands (the absolute 1e-12 the checker had lost all 693 pixels of the small box)."""
    _judge_checker(ora, rs.grazing_views())
