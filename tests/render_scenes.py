"""Scenes for the exact-geometry judge of the depth camera (tests/render_judge.py), shared by the CPU tests
of the checker and the GPU tests of the kernel.  Every scene is small: tens of pixels square, at most a few
thousand triangles.  judged(scene) is computed once per session and shared."""
import numpy as np

from tests import render_judge

IDENT = np.array([1.0, 0.0, 0.0, 0.0])
SCALE = 10.0 / 256.0


def default_mount():
    # Rotationd::FromEulerYPR(-90 deg, 0, -90 deg): camera z = body x, camera x = body -y, camera y = body -z
    y, p, r = -np.pi / 2, 0.0, -np.pi / 2
    cy, sy, cp, sp, cr, sr = np.cos(y / 2), np.sin(y / 2), np.cos(p / 2), np.sin(p / 2), np.cos(r / 2), np.sin(r / 2)
    return np.array([cy * cp * cr + sy * sp * sr, cy * cp * sr - sy * sp * cr, cy * sp * cr + sy * cp * sr,
                     sy * cp * cr - cy * sp * sr])


MOUNT = default_mount()


class Cam:
    """The camera's numbers; .ora(ora) and .afa(afa) give the checker's and the engine's structures."""

    def __init__(self, width, height, focal=None, cx=None, cy=None, depth_scale=SCALE, max_count=255):
        self.width, self.height = width, height
        self.focal_length = width / 2.0 if focal is None else float(focal)
        self.cx = width / 2.0 if cx is None else float(cx)
        self.cy = height / 2.0 if cy is None else float(cy)
        self.depth_scale, self.max_count = float(depth_scale), int(max_count)

    def _fill(self, c):
        c.focal_length, c.cx, c.cy, c.depth_scale, c.max_count = self.focal_length, self.cx, self.cy, self.depth_scale, self.max_count
        return c

    def ora(self, ora):
        return self._fill(ora.render_camera(self.width, self.height))

    def afa(self, afa):
        return self._fill(afa.camera_default(self.width, self.height))


class View:
    def __init__(self, name, cam, tris, pos, att, mount, all_hit=False):
        self.name, self.cam = name, cam
        self.tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
        self.pos, self.att, self.mount = np.asarray(pos, float), np.asarray(att, float), np.asarray(mount, float)
        self.all_hit = all_hit        # a closed mesh seen from inside: every pixel below max_count

    def __repr__(self):
        return self.name


_JUDGED = {}


def judged(view):
    if view.name not in _JUDGED:
        _JUDGED[view.name] = render_judge.judge(view.cam, view.tris, view.pos, view.att, view.mount)
    return _JUDGED[view.name]


def checker_image(ora, view):
    return ora.render_depth(view.cam.ora(ora), view.tris, view.pos, view.att, view.mount)


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def quat_matrix(q):
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                     a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])


def camera_axes(att, mount):
    """columns: world directions of image right, image down and the optical axis, snapped to the nearest integers
    (for the axis-aligned attitudes the lattice scenes are built around)"""
    return np.rint(quat_matrix(quat_mul(att, mount))).astype(int)


def yaw(deg):
    a = np.deg2rad(deg) / 2
    return np.array([np.cos(a), 0.0, 0.0, np.sin(a)])


def pitch(deg):
    a = np.deg2rad(deg) / 2
    return np.array([np.cos(a), 0.0, np.sin(a), 0.0])


def roll(deg):
    a = np.deg2rad(deg) / 2
    return np.array([np.cos(a), np.sin(a), 0.0, 0.0])


def quad(p, a, b):
    """two triangles of the parallelogram p, p + a, p + a + b, p + b"""
    p, a, b = (np.asarray(x, float) for x in (p, a, b))
    return np.array([np.concatenate([p, p + a, p + a + b]), np.concatenate([p, p + a + b, p + b])])


def lattice_wall(origin, right, down, axis, dist, pitch_m, half_w, half_h, alternate=True):
    """A wall dist metres along `axis` from origin, tessellated on a pitch_m lattice of the plane's two
    coordinates (integer unit vectors right / down), cells split along alternating diagonals or all one way."""
    nx, ny = int(round(half_w / pitch_m)), int(round(half_h / pitch_m))
    tris = []
    c = np.asarray(origin, float) + dist * np.asarray(axis, float)
    r, d = np.asarray(right, float) * pitch_m, np.asarray(down, float) * pitch_m
    for i in range(-nx, nx):
        for j in range(-ny, ny):
            p00, p10, p11, p01 = c + i * r + j * d, c + (i + 1) * r + j * d, c + (i + 1) * r + (j + 1) * d, c + i * r + (j + 1) * d
            if (i + j) & 1 or not alternate:
                tris += [np.concatenate([p00, p10, p11]), np.concatenate([p00, p11, p01])]
            else:
                tris += [np.concatenate([p00, p10, p01]), np.concatenate([p10, p11, p01])]
    return np.array(tris)


def closed_box(lo, hi):
    """the box of test_gpu_render.py::test_degenerate_meshes"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    c = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], float)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return np.array([np.concatenate([c[a], c[b], c[d]]) for a, b, d, e in quads] +
                    [np.concatenate([c[a], c[d], c[e]]) for a, b, d, e in quads], np.float32)


# ------------------------------------------------------------------------------------------------
# lattice walls: every pixel ray runs along mesh edges and through vertices
# ------------------------------------------------------------------------------------------------
AXIS_ATTITUDES = {
    MOUNT.tobytes(): [("yaw0", IDENT), ("yaw90", yaw(90)), ("yaw180", yaw(180)), ("yaw270", yaw(270)), ("down", pitch(90))],
    IDENT.tobytes(): [("yaw0", IDENT), ("yaw90", yaw(90)), ("yaw180", yaw(180)), ("yaw270", yaw(270)), ("down", roll(180))],
}


def lattice_views():
    views = []
    for dist, pitch_m in ((3.0, 1.0 / 16), (3.0, 1.0 / 8), (1.5, 1.0 / 32)):
        for mname, mount in (("mount", MOUNT), ("nomount", IDENT)):
            for oname, origin in (("origin", (0.0, 0.0, 0.0)), ("metres", (2.0, -3.0, 1.0))):
                # the finest wall from the origin through the default mount on the larger camera, the rest on the smaller
                big = mname == "mount" and oname == "origin" and pitch_m == 1.0 / 16
                w, h = (48, 36) if big else (24, 18)
                # focal 48: the ray of pixel px meets the wall at 3 m (px - cx) / 16 m off the axis, at 1.5 m (px - cx) / 32 m: on a lattice line
                cam = Cam(w, h, focal=16.0 * 3.0)
                half_w, half_h = dist * (w / 2) / cam.focal_length, dist * (h / 2) / cam.focal_length
                for aname, att in AXIS_ATTITUDES[mount.tobytes()]:
                    ax = camera_axes(att, mount)
                    wall = lattice_wall(origin, ax[:, 0], ax[:, 1], ax[:, 2], dist, pitch_m, half_w + 2 * pitch_m, half_h + 2 * pitch_m,
                                        alternate=oname == "metres")
                    # a second wall behind the first: a leak shows a wrong depth, not only max_count
                    back = np.asarray(origin, float) + (dist + 2.0) * ax[:, 2]
                    behind = quad(back - 40.0 * ax[:, 0] - 40.0 * ax[:, 1], 80.0 * ax[:, 0], 80.0 * ax[:, 1])
                    views.append(View("lattice %gm/%g %s %s %s" % (dist, pitch_m, mname, oname, aname), cam,
                                      np.concatenate([wall, behind]), origin, att, mount, all_hit=True))
    return views


# ------------------------------------------------------------------------------------------------
# closed meshes seen from inside
# ------------------------------------------------------------------------------------------------
def box_views():
    lo, hi = np.array([-2, -2, 0.0]), np.array([2, 2, 2.5])
    box = closed_box(lo, hi)
    centre = 0.5 * (lo + hi)
    views = []
    # focal 16: the corners of the face ahead (2 m away, +-2 m, +-1.25 m) are pixels (0 | 32, 0 | 20) of a 33 x 21 image and
    # its four edges the image's border; focal 8: the same corners at (8 | 24, 5 | 15), the edges between the faces in view
    for cname, cam in (("f16", Cam(33, 21, focal=16.0, cx=16.0, cy=10.0)), ("f8", Cam(33, 21, focal=8.0, cx=16.0, cy=10.0))):
        for aname, att in AXIS_ATTITUDES[MOUNT.tobytes()] + [("up", pitch(-90))]:
            views.append(View("box centred %s %s" % (cname, aname), cam, box, centre, att, MOUNT, all_hit=True))
    # the camera of test_gpu_render.py::test_degenerate_meshes WITHOUT its step aside: pixel (0, 25) looks into a corner
    for aname, att in AXIS_ATTITUDES[MOUNT.tobytes()][:4]:
        views.append(View("box 40x30 from (0, 0, 1) %s" % aname, Cam(40, 30), box, (0.0, 0.0, 1.0), att, MOUNT, all_hit=True))
    return views


def degenerate_view():
    """the second mesh of test_gpu_render.py::test_degenerate_meshes from that test's camera: 300 coincident triangles, a zero-area
    one, and a sliver 1.2e-7 m high whose lower edge row 15 runs along, pixels (10, 15) and (30, 15) through its end vertices"""
    one = np.array([[3, -1, 0, 3, 1, 0, 3, 0, 2]], np.float32)
    many = np.concatenate([np.repeat(one, 300, 0), np.array([[2, -1, 1, 2, 1, 1, 2, 1, 1.0000001]], np.float32),
                           np.array([[4, 0, 0, 4, 0, 0, 4, 0, 0]], np.float32)])
    return View("degenerate meshes: coincident, sliver, zero area", Cam(40, 30), many, (0.0, 0.0, 1.0), IDENT, MOUNT)


def icosphere_views(scen):
    sv, sf = scen._icosphere(2)
    tris = (sv * 3.0 + [1.0, 2.0, 3.0])[sf].reshape(-1, 9).astype(np.float32)
    rng = np.random.default_rng(3)
    atts = [("yaw0", IDENT), ("down", pitch(90))] + [("tilt%d" % k, q) for k, q in enumerate(scen.random_attitudes(rng, 2, max_tilt_deg=80.0).T)]
    return [View("icosphere inside %s" % n, Cam(32, 24), tris, (1.0, 2.0, 3.0), q, MOUNT, all_hit=True) for n, q in atts]


# ------------------------------------------------------------------------------------------------
# generic views: nothing is aligned with anything
# ------------------------------------------------------------------------------------------------
def generic_views(scen):
    tris = scen.orchard_mesh(rows=2, cols=3, seed=9, canopy_subdiv=2)
    rng = np.random.default_rng(5)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    views = []
    for (w, h, f) in ((37, 23, 20.5), (16, 4, 8.0), (1, 1, 1.0), (130, 5, 200.0)):
        cam = Cam(w, h, focal=f, cx=0.37 * w, cy=0.61 * h, depth_scale=0.05, max_count=1000)
        n = 3
        pos = np.stack([rng.uniform(lo[0] * 0.5, hi[0] * 0.8, n), rng.uniform(lo[1] * 0.5, hi[1] * 0.8, n), rng.uniform(0.4, 3.0, n)])
        att = scen.random_attitudes(rng, n, max_tilt_deg=80.0)
        for i in range(n):
            views.append(View("orchard 2x3 %dx%d view %d" % (w, h, i), cam, tris, pos[:, i], att[:, i], IDENT if i == 2 else MOUNT))
    return views


# ------------------------------------------------------------------------------------------------
# quantisation: walls at and next to multiples of depth_scale, at and beyond the range, behind, through the origin
# ------------------------------------------------------------------------------------------------
def quantisation_views():
    cam = Cam(16, 12)
    wall = lambda x: quad((x, -50.0, -50.0), (0.0, 100.0, 0.0), (0.0, 0.0, 100.0))
    views = []
    for k in (1, 7, 77, 254):
        x = np.float32(k * SCALE)                          # exact: depth_scale = 10 / 256 is a binary fraction
        for name, xx in (("at", x), ("below", np.nextafter(x, np.float32(0))), ("above", np.nextafter(x, np.float32(100)))):
            views.append(View("wall %s count %d" % (name, k), cam, wall(xx), (0.0, 0.0, 0.0), IDENT, MOUNT))
    x = np.float32(255 * SCALE)
    for name, xx in (("at range", x), ("just inside range", np.nextafter(x, np.float32(0))), ("beyond range", np.float32(12.0)),
                     ("behind", np.float32(-3.0)), ("through the origin", np.float32(0.0))):
        views.append(View("wall %s" % name, cam, wall(xx), (0.0, 0.0, 0.0), IDENT, MOUNT))
    return views


# ------------------------------------------------------------------------------------------------
# grazing incidence and scale: where an absolute determinant cutoff could drop what the geometry says is hit
# ------------------------------------------------------------------------------------------------
def grazing_views():
    # a strip of ground in centimetre triangles seen from 2 cm up by a long lens pitched 0.5 deg down: rays meet it at 0.33 .. 0.67 deg
    cam = Cam(32, 24, focal=4000.0)
    strip = lattice_wall((2.6, 0.0, 0.0), (0, 1, 0), (1, 0, 0), (0, 0, 0), 0.0, 0.01, 0.03, 1.1)
    views = [View("grazing 0.5deg cm triangles", cam, strip, (0.0, 0.0, 0.02), pitch(0.5), MOUNT, all_hit=True),
             View("grazing 0.5deg cm triangles off lattice", cam, strip, (0.0013, 0.0007, 0.0203), pitch(0.5), MOUNT, all_hit=True)]
    # the closed box at 2^-24 of its size (a quarter of a micrometre across), camera at its centre: the same picture in other units
    s = 2.0 ** -24
    lo, hi = np.array([-2, -2, 0.0]) * s, np.array([2, 2, 2.5]) * s
    views.append(View("box centred scaled 2^-24", Cam(33, 21, focal=16.0, cx=16.0, cy=10.0, depth_scale=SCALE * s),
                      closed_box(lo, hi), 0.5 * (lo + hi), IDENT, MOUNT, all_hit=True))
    return views


def mirrored_views(scen):
    """the scenes the kernel is judged on as well as the checker"""
    return lattice_views() + box_views() + icosphere_views(scen) + quantisation_views() + grazing_views()
