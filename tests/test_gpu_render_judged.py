"""The depth-camera kernel held to exact geometry: the scenes of tests/render_scenes.py -- walls on lattices whose edges and
vertices every pixel ray runs along, closed meshes seen from their centre, quantisation ties, grazing incidence -- rendered
by both walks, compared bit for bit with the CPU checker AND judged by tests/render_judge.py, which shares arithmetic with
neither.  tests/test_render_judge_cpu.py holds the checker to the same judge on a CPU.  Needs an MI355X."""
import numpy as np
import pytest

from tests import render_scenes as rs
from tests.render_judge import assert_passes
from tests.scenarios import afa

pytestmark = pytest.mark.gpu

scen = afa.scenarios


def _render_both_walks(ora, view):
    scene = afa.Scene(view.tris)
    cam = view.cam.afa(afa)
    want = rs.checker_image(ora, view)
    j = rs.judged(view)
    try:
        for plain in (False, True):
            scene.set_walk(plain)
            got, _ = scene.render(cam, view.pos.reshape(3, 1), view.att.reshape(4, 1), view.mount)
            np.testing.assert_array_equal(got[0], want, err_msg="%s, plain walk %s" % (view.name, plain))
            assert_passes(j, got[0], "%s, plain walk %s" % (view.name, plain))
            if view.all_hit:
                assert got[0].max() < view.cam.max_count, view.name
    finally:
        scene.close()


def test_lattice_walls(ora):
    """Every pixel ray along mesh edges and through vertices; the wall behind is two large triangles, kept out of the tree,
    so the corner-ray cull of the tile entry pass is exercised against the closed edge rule as well."""
    for view in rs.lattice_views():
        _render_both_walks(ora, view)


def test_centred_box_and_icosphere(ora):
    for view in rs.box_views() + rs.icosphere_views(scen):
        _render_both_walks(ora, view)


def test_quantisation(ora):
    for view in rs.quantisation_views():
        _render_both_walks(ora, view)


def test_grazing_incidence_and_scale(ora):
    for view in rs.grazing_views():
        _render_both_walks(ora, view)


def test_quarter_turns_from_fp32_engine_state_four_kilometres_out(ora):
    """render_engine from fp32 state 4 km out: x and y live in the slabs relative to their anchors and the pose kernel adds
    them in double.  Five vehicles on one whole-metre spot, the four quarter-turn yaws and straight down (as fp32 holds
    them: cos 45 deg is not a float), each facing a 1/8 m lattice wall 3 m away with a closed box behind it; judged from
    the pose get_state reports."""
    origin = np.array([4002.0, 3997.0, 1.0])
    atts = rs.AXIS_ATTITUDES[rs.MOUNT.tobytes()]
    cam_numbers = rs.Cam(24, 18, focal=48.0)
    walls = []
    for _, att in atts:
        ax = rs.camera_axes(att, rs.MOUNT)
        walls.append(rs.lattice_wall(origin, ax[:, 0], ax[:, 1], ax[:, 2], 3.0, 1.0 / 8, 1.0, 0.75))
    tris = np.concatenate(walls + [rs.closed_box(origin - 6.0, origin + 6.0)]).astype(np.float32)
    n = len(atts)
    e = afa.Ensemble(n, precision=afa.AFE_F32)
    e.set_type_table([afa.params_from_type(5)])
    e.set_state(np.tile(origin[:, None], (1, n)), np.zeros((3, n)), np.stack([a for _, a in atts], 1), np.zeros((3, n)), np.zeros((4, n)))
    scene = afa.Scene(tris)
    cam = cam_numbers.afa(afa)
    st = e.get_state()
    assert np.array_equal(st["pos"], np.tile(origin[:, None], (1, n)))
    try:
        for plain in (False, True):
            scene.set_walk(plain)
            imgs, _ = scene.render_engine(e, cam, rs.MOUNT)
            for i, (name, _) in enumerate(atts):
                view = rs.View("engine 4 km out %s" % name, cam_numbers, tris, st["pos"][:, i], st["att"][:, i], rs.MOUNT, all_hit=True)
                np.testing.assert_array_equal(imgs[i], rs.checker_image(ora, view), err_msg=view.name)
                assert_passes(rs.judged(view), imgs[i], view.name)
                assert imgs[i].max() < 255
    finally:
        scene.close()
        e.close()


def test_an_axis_aligned_orchard_view_is_held_to_geometry(ora):
    """tests/test_gpu_render.py::test_ordered_and_plain_walk_give_the_same_images_on_thousands_of_views compares its
    axis-aligned whole-metre views (0, 1, 6, 20, 21 of its sample) with the checker only; here view 1 of that very sample,
    through the default mount at a reduced camera size, is judged by geometry as well."""
    tris = scen.orchard_mesh(rows=16, cols=16, seed=11)
    rng = np.random.default_rng(21)                     # that test's own draw
    n = 4096
    pos = np.stack([rng.uniform(-10, 60, n), rng.uniform(-10, 60, n), rng.uniform(0.3, 9.0, n)])
    q = rng.normal(size=(4, n))
    q /= np.linalg.norm(q, axis=0)
    k = n // 8
    yaw = rng.integers(0, 4, k) * (np.pi / 2)
    q[:, :k] = np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)])
    pos[:, :k] = np.round(pos[:, :k])
    view = rs.View("orchard 16x16 sample view 1", rs.Cam(32, 24), tris, pos[:, 1], q[:, 1], afa.camera_default_mount())
    assert np.array_equal(np.abs(rs.camera_axes(view.att, view.mount)).sum(0), [1, 1, 1]) and np.array_equal(view.pos, np.round(view.pos))
    _render_both_walks(ora, view)
    img = rs.checker_image(ora, view)
    assert img.min() < 255
