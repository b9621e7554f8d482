"""The first-hit ray query in numpy float64 (test infrastructure): every ray against every triangle, the expression tree
of agri-fly_amd/csrc/afe_raycast.hip's header comment operation for operation (which is ray_triangle of
oracle/agrifly_oracle_render.c).  numpy rounds every elementwise operation separately (no contraction), and only
+ - * /, abs, maximum and comparisons appear, so the same tree gives the same bits as the kernel.  No hierarchy, no culling:
what the kernel's boxes may never change.
"""
import numpy as np

from tests import path_checker as pc

INF = np.inf
BEAM_DTYPE = np.dtype([("off", np.float64, 3), ("dir", np.float64, 3), ("t_max", np.float64), ("frame", np.int32), ("reserved", np.int32)])


def _dot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def _cross(u, v):
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def _norm1(u):
    return np.abs(u[0]) + np.abs(u[1]) + np.abs(u[2])


def tri_tables(triangles):
    """v0, e1, e2 [3, T] in double from float32 triangles [T, 9]"""
    t = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 3, 3).astype(np.float64)
    v0 = t[:, 0].T.copy()
    return v0, t[:, 1].T - v0, t[:, 2].T - v0


def ray_triangle(v0, e1, e2, o, d):
    """t of the definition for broadcastable operands ([3, ...] each); +inf: no hit"""
    with np.errstate(all="ignore"):
        p = _cross(d, e2)
        det = _dot(e1, p)
        tv = [o[k] - v0[k] for k in range(3)]
        en = np.maximum(_norm1(e1), _norm1(e2))
        dn = _norm1(d)
        k1 = 2.0 ** -48 * en
        cut = np.maximum(1.0, 32768.0 * en)
        tn = _norm1(tv)
        eps = (dn * k1) * (tn + en)
        hit = np.abs(det) > eps * cut
        s = np.where(det > 0.0, 1.0, -1.0)
        nu = _dot(tv, p) * s
        hit &= ~(nu < -eps)
        q = _cross(tv, e1)
        nv = _dot(d, q) * s
        hit &= ~(nv < -eps)
        hit &= ~((np.abs(det) - nu) - nv < -eps)
        inv = 1.0 / det
        t = _dot(e2, q) * inv
        hit &= (t > 0.0) & (t < INF)
    return np.where(hit, t, INF)


def pair_t(triangles, origin, dir):
    """t [n, T] of every ray against every triangle (+inf: no hit), nothing else applied"""
    v0, e1, e2 = tri_tables(triangles)
    o, d = np.asarray(origin, np.float64), np.asarray(dir, np.float64)
    return ray_triangle(v0[:, None, :], e1[:, None, :], e2[:, None, :], o[:, :, None], d[:, :, None])


def raycast(triangles, origin, dir, t_max=None, pairs_per_chunk=1 << 21):
    """origin, dir [3, n]; t_max None, a scalar or [n] -> (t [n], tri [n] int32): the WINNER of the definition"""
    v0, e1, e2 = tri_tables(triangles)
    o, d = np.asarray(origin, np.float64), np.asarray(dir, np.float64)
    n, T = o.shape[1], v0.shape[1]
    tm = np.full(n, INF) if t_max is None else np.broadcast_to(np.asarray(t_max, np.float64), (n,))
    t_out, tri_out = np.full(n, INF), np.full(n, -1, np.int32)
    step = max(1, pairs_per_chunk // max(T, 1))
    for lo in range(0, n, step):
        sl = slice(lo, min(n, lo + step))
        t = ray_triangle(v0[:, None, :], e1[:, None, :], e2[:, None, :], o[:, sl, None], d[:, sl, None])
        t = np.where(t <= tm[sl, None], t, INF)
        best = np.argmin(t, axis=1)                 # the first of equal minima: the lowest index
        tb = t[np.arange(t.shape[0]), best]
        found = tb < INF
        t_out[sl] = np.where(found, tb, INF)
        tri_out[sl] = np.where(found, best, -1)
    finite = np.isfinite(o).all(0) & np.isfinite(d).all(0)
    t_out[~finite] = INF
    tri_out[~finite] = -1
    return t_out, tri_out


def line_of_sight(triangles, p0, p1):
    """p0, p1 [3, n] -> blocked [n] uint8"""
    a, b = np.asarray(p0, np.float64), np.asarray(p1, np.float64)
    with np.errstate(all="ignore"):
        d = b - a
    t, _ = raycast(triangles, a, d, 1.0)
    return (t < INF).astype(np.uint8)


def pixel_rays(cam, pos, att, mount):
    """the rays of oracle/agrifly_oracle_render.c pixel_depth, in its operation order: origin [3, H*W], dir [3, H*W], row-major pixels"""
    o, R = pc.camera_pose(pos, att, mount)
    px, py = np.meshgrid(np.arange(cam.width, dtype=np.float64), np.arange(cam.height, dtype=np.float64))
    u = ((px - cam.cx) / cam.focal_length).reshape(-1)
    v = ((py - cam.cy) / cam.focal_length).reshape(-1)
    d = np.stack([R[3 * r] * u + R[3 * r + 1] * v + R[3 * r + 2] for r in range(3)])
    return np.repeat(o[:, None], u.size, 1), d


def sensor_rays(pos, att, beams, mount=None):
    """pos [3, n], att [4, n] in double (anchors added, as get_state returns them); beams: BEAM_DTYPE [B] ->
    origin, dir [B, 3, n] of the RANGE SENSOR rule"""
    pos, att = np.asarray(pos, np.float64), np.asarray(att, np.float64)
    ov, R = pc.camera_pose(pos, att, mount)              # vectorised over the vehicles: [3, n], [9, n]
    B, n = len(beams), pos.shape[1]
    origin, dirs = np.empty((B, 3, n)), np.empty((B, 3, n))
    with np.errstate(all="ignore"):
        for b in range(B):
            off, dr = beams["off"][b], beams["dir"][b]
            for r in range(3):
                if beams["frame"][b] == 0:
                    origin[b, r] = ov[r] + ((R[3 * r] * off[0] + R[3 * r + 1] * off[1]) + R[3 * r + 2] * off[2])
                    dirs[b, r] = (R[3 * r] * dr[0] + R[3 * r + 1] * dr[1]) + R[3 * r + 2] * dr[2]
                else:
                    origin[b, r] = ov[r] + off[r]
                    dirs[b, r] = np.full(n, dr[r])
    return origin, dirs


def range_sensor(triangles, pos, att, beams, mount=None):
    """-> (t [B, n], tri [B, n] int32)"""
    origin, dirs = sensor_rays(pos, att, beams, mount)
    B, n = origin.shape[0], origin.shape[2]
    t, tri = np.empty((B, n)), np.empty((B, n), np.int32)
    for b in range(B):
        t[b], tri[b] = raycast(triangles, origin[b], dirs[b], beams["t_max"][b])
    return t, tri


def assert_same_bits(got_t, got_tri, want_t, want_tri, what=""):
    got_t, want_t = np.ascontiguousarray(got_t, np.float64), np.ascontiguousarray(want_t, np.float64)
    bad = np.flatnonzero((got_t.view(np.uint64) != want_t.view(np.uint64)).reshape(-1) | (np.asarray(got_tri) != np.asarray(want_tri)).reshape(-1))
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got (%r, %d), want (%r, %d)" % (
        what, bad.size, got_t.size, bad[0], got_t.reshape(-1)[bad[0]], np.asarray(got_tri).reshape(-1)[bad[0]],
        want_t.reshape(-1)[bad[0]], np.asarray(want_tri).reshape(-1)[bad[0]])
