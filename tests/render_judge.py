"""An exact-geometry judge for depth images (CPU, plain Python / numpy).

The depth camera's CPU checker (oracle/agrifly_oracle_render.c) restates the kernel's ray / triangle
arithmetic operation for operation, so the two agree bit for bit whether or not that arithmetic
matches the geometry.  This module knows only the geometry and the image contract of
oracle/agrifly_oracle_render.h and shares no code or arithmetic with either:

  * pixel (px, py) looks along the camera-frame ray ((px - cx)/f, (py - cy)/f, 1);
  * camera-to-world rotation = att * mount (Hamilton product, the reference's convention), turned into
    a matrix by the usual polynomial in the quaternion's components -- NOT normalised, exactly as the
    contract has it: a quaternion of norm n scales every ray direction by n^2 and every depth by
    1 / n^2, for the judge as for the renderer (accounted for, not bounded);
  * the depth of a hit is the ray parameter t (the camera-frame z, the ray's z component being 1);
  * count = min(floor(z / depth_scale), max_count), and a miss reads max_count.

Exact arithmetic where decisions are made
-----------------------------------------
Every input is a binary floating-point number, hence a rational.  The rotation matrix is a
polynomial in the quaternion components; f times the ray direction, d' = R (px - cx, py - cy, f), is a
polynomial in those and the camera's numbers; and for a triangle (v0, e1 = v1 - v0, e2 = v2 - v0) seen
from o (tv = o - v0)

    det = e1 . (d x e2)      N_u = tv . (d x e2)      N_v = d . (tv x e1)      N_t = e2 . (tv x e1)
    N_w = det - N_u - N_v    u = N_u / det,  v = N_v / det,  w = N_w / det,  t = N_t / det

are polynomials in all of these.  They are evaluated in fractions.Fraction from the given doubles and
float32 vertices; since every one of those fractions has a power of two for its denominator (f cancels
out of every sign and is put back into t), the inner products run on the integer numerators over one
common denominator -- the same rationals, nothing rounded.

Triangles are CLOSED sets: u, v, w >= 0 (a ray along an edge or through a vertex hits), t > 0.  A
zero-area triangle, and a triangle seen exactly edge-on (det == 0), hit nothing.

Speed: a float64 pass over all (pixel, triangle) pairs evaluates the same five determinants (as
products of a [pixels x 3] and a [3 x triangles] matrix) together with a bound on its own rounding
error; only the pairs that the bound cannot decide -- some of u, v, w, t, det within it of a decision --
and that could still matter to their pixel are decided again exactly.

The tolerance: delta and tau
----------------------------
With u0 = 2^-53, |.| the 1-norm, E = max(|e1|, |e2|), T = |tv|, D = |d|, the per-pair condition is

    K   = D E (T + E)        for det, N_u, N_v, N_w        (the issue's |tv| |d| |e|, plus the E^2 of det)
    K_t = T E^2              for N_t.

Each of the determinants is six triple products of one component from each of its three vectors, so the
six together are at most the product of the three 1-norms (D E T or D E E).  Evaluated in fp64, a triple
product collects at most 7 roundings before the last sum is formed: the subtraction that formed tv or e
(one; e is usually exact), the two multiplications, the cross product's subtraction, and the dot product's
two additions, one to spare.  So |fl(N) - N| <= 7 u0 K for N_u, N_v, det and 7 u0 K_t for N_t, to first
order.  N_w adds the three errors and its own two subtractions, 2 u0 (|det| + |N_u| + |N_v|):
at most 9 u0 D E (E + 2 T) <= 18 u0 K.

    C_FLOAT = 2^-47 (64 u0)    bounds this module's OWN float pass: 18 u0 K and the rounding of K itself, and of
                               the direction d (rounded once from its exact value), with a factor 3 to spare.
                               A pair is sent to exact arithmetic unless it is decided by more than that.

A renderer that evaluates the test in fp64 differs from the exact geometry in three ways:
  (a) the roundings above: <= 18 u0 K on a numerator;
  (b) its own ray.  The quaternion product (4 terms, each component within 4 u0 |a||b|), the matrix (sums
      of four squares or two doubled products: another 4 u0 n^2 on top of the 2 x 4 u0 n^2 handed down by
      q), the pixel coordinate (a subtraction and a division, 2 u0) and the three-term sum R (u, v, 1)
      (3 u0) leave each component of d within 16 u0 n^2 (|u| + |v| + 1) <= 16 sqrt(3) u0 |d|_2, so the 1-norm of
      the error is at most 3 x 16 sqrt(3) u0 D < 84 u0 D, which moves a numerator by at most 84 u0 K;
  (c) a tolerance eps of its own, which a watertight test needs in order to accept every ray that lies in
      the closed triangle despite (a): eps >= 18 u0 K.  The engine's is 32 u0 K = 2^-48 K.
A count can therefore come from a point that is outside the triangle by (a) + (b) + (c) + (a) again (the
accepted numerator is itself rounded): (18 + 84 + 32 + 18) u0 K = 152 u0 K.

    C_TOL = 2^-45 (256 u0)     delta = C_TOL K / |det| per ray and triangle: the triangle grown to u, v >= -delta,
                               u + v <= 1 + delta.  Any renderer tolerance eps <= 2^-46 K stays inside it.

t = N_t / det carries 7 u0 K_t / |N_t| from its numerator, (7 + 84) u0 K / |det| from the determinant and
two roundings of its own (reciprocal, product), and floor(z / depth_scale) one more:

    tau = (C_TOL + C_FLOAT) (K_t / |N_t| + K / |det|) + 2^-50     per ray and triangle
          (the C_FLOAT share pays for the float pass where that supplied t).

What fp64 cannot resolve is not demanded.  A pair whose |det| is not above C_TOL K max(1, 2^15 E) has a
determinant whose sign rounding can flip, or a delta so large that the hit point is uncertain by more than
3 delta E = 3 x 2^-15 m (a tenth of a millimetre; the engine keeps it inside its 3e-4 m box inflation); a
pair whose N_t is not above C_TOL K_t has a t whose sign rounding can flip (the camera lies in the
triangle's plane).  Such a pair is left out of z_exact -- the renderer may miss it -- and stays in
z_dilated -- the renderer may also see it, at max(t, 0).  For the scenes judged here this excuses triangles
within about 1e-9 rad of edge-on and within about 1e-13 m of the camera; it excuses no shared edge.

Per pixel
---------
    z_exact    nearest hit of the closed triangles (those fp64 can be asked to resolve, see above)
    z_dilated  nearest hit of the delta-grown triangles; z_dilated <= z_exact by construction
A rendered count c passes iff some z in [z_dilated (1 - tau), z_exact (1 + tau)] has
min(floor(z / depth_scale), max_count) == c, a miss standing for z = +inf: the camera never sees farther
than the truth (no leak, no lost triangle), never nearer than a delta-grown silhouette, and a
quantisation tie may fall either way.  Both ends are taken per pair (min over pairs of t (1 +- tau)).
"""
from fractions import Fraction

import numpy as np

C_FLOAT = 2.0 ** -47
C_TOL = 2.0 ** -45
POS_RES = 2.0 ** 15          # 1 / metres: |det| must exceed C_TOL K max(1, POS_RES E) to be demanded
TAU_FLOOR = 2.0 ** -50
_CHUNK = 1 << 21             # (pixel, triangle) pairs per block of the float pass


# ------------------------------------------------------------------------------------------------
# exact helpers
# ------------------------------------------------------------------------------------------------
def _F(x):
    return Fraction(*float(x).as_integer_ratio())


def quat_mul_exact(a, b):
    """Hamilton product a * b of two quaternions (w, x, y, z), in Fractions."""
    a0, a1, a2, a3 = a
    b0, b1, b2, b3 = b
    return (a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3,
            a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
            a0 * b2 + a2 * b0 + a3 * b1 - a1 * b3,
            a0 * b3 + a3 * b0 + a1 * b2 - a2 * b1)


def rotation_exact(q):
    """The (unnormalised) rotation matrix of quaternion q: |q|^2 times a rotation."""
    w, x, y, z = q
    return ((w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)),
            (2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)),
            (2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z))


def _common_shift(fracs):
    """smallest s with every fraction * 2^s an integer (denominators are powers of two)"""
    s = 0
    for f in fracs:
        s = max(s, f.denominator.bit_length() - 1)
    return s


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


class Judged:
    """What judge() knows about every pixel of one view (arrays are height x width)."""

    def __init__(self, cam, h, w):
        self.width, self.height = w, h
        self.depth_scale, self.max_count = float(cam.depth_scale), int(cam.max_count)
        self.z_exact = np.full((h, w), np.inf)
        self.z_dilated = np.full((h, w), np.inf)
        self.z_hi = np.full((h, w), np.inf)      # min over demanded pairs of t (1 + tau)
        self.z_lo = np.full((h, w), np.inf)      # min over delta-grown pairs of max(t, 0) (1 - tau)
        self.tri = np.full((h, w), -1, np.int64)         # the triangle of z_exact
        self.bary = np.full((h, w, 2), np.nan)           # its (u, v)
        self.n_pairs = self.n_exact_pairs = 0

    def _count(self, z):
        with np.errstate(invalid="ignore", over="ignore"):
            c = np.floor(np.where(np.isfinite(z), z, 0.0) / self.depth_scale)
        return np.where(np.isfinite(z), np.minimum(c, self.max_count), self.max_count).astype(np.int64)

    @property
    def count_lo(self):
        return self._count(self.z_lo)

    @property
    def count_hi(self):
        return self._count(self.z_hi)

    def passes(self, image):
        img = np.asarray(image).astype(np.int64).reshape(self.height, self.width)
        return (img >= self.count_lo) & (img <= self.count_hi)

    def failures(self, image, limit=None):
        """[(px, py, got, z_dilated, z_exact, nearest triangle, (u, v))] of the pixels that do not pass."""
        img = np.asarray(image).reshape(self.height, self.width)
        bad = np.argwhere(~self.passes(img))
        out = [(int(px), int(py), int(img[py, px]), float(self.z_dilated[py, px]), float(self.z_exact[py, px]),
                int(self.tri[py, px]), tuple(float(x) for x in self.bary[py, px])) for py, px in bad]
        return out if limit is None else out[:limit]

    def explain(self, image, limit=8):
        f = self.failures(image)
        lines = ["%d of %d pixels fail the exact-geometry judge" % (len(f), self.width * self.height)]
        for px, py, got, zd, ze, tri, (u, v) in f[:limit]:
            lines.append("  pixel (%d, %d): count %d, z_dilated %.17g, z_exact %.17g (counts %d..%d), triangle %d at u=%.6g v=%.6g"
                         % (px, py, got, zd, ze, self.count_lo[py, px], self.count_hi[py, px], tri, u, v))
        return "\n".join(lines)


def assert_passes(judged, image, what=""):
    ok = judged.passes(image)
    assert ok.all(), (what + ": " if what else "") + judged.explain(image)


# ------------------------------------------------------------------------------------------------
# the judge
# ------------------------------------------------------------------------------------------------
def judge(cam, triangles, pos, att, mount=(1.0, 0.0, 0.0, 0.0)):
    """Judge one view.  cam: anything with width, height, focal_length, cx, cy, depth_scale, max_count;
    triangles: n x 9 float32 (v0 v1 v2); pos: camera origin; att, mount: quaternions (w, x, y, z)."""
    W, H = int(cam.width), int(cam.height)
    tris = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 9)
    out = Judged(cam, H, W)
    f_focal = _F(cam.focal_length)
    if not np.all(np.isfinite(np.asarray(pos, dtype=float))):     # a camera that is nowhere sees nothing
        return out

    # ---- the rays, exactly: d' = f d = R (px - cx, py - cy, f), integers over 2^sd
    R = rotation_exact(quat_mul_exact([_F(x) for x in att], [_F(x) for x in mount]))
    cx, cy = _F(cam.cx), _F(cam.cy)
    colx = [[R[k][0] * (px - cx) for k in range(3)] for px in range(W)]
    coly = [[R[k][1] * (py - cy) + R[k][2] * f_focal for k in range(3)] for py in range(H)]
    sd = _common_shift([x for c in colx for x in c] + [x for c in coly for x in c])
    colx = [[int(x * (1 << sd)) for x in c] for c in colx]
    coly = [[int(x * (1 << sd)) for x in c] for c in coly]
    d_den = f_focal * (1 << sd)                               # d = d_int / d_den
    d_int = [[tuple(colx[px][k] + coly[py][k] for k in range(3)) for px in range(W)] for py in range(H)]
    d_flt = np.array([[[float(Fraction(c) / d_den) for c in d_int[py][px]] for px in range(W)] for py in range(H)]).reshape(-1, 3)

    # ---- the geometry, exactly: integers over 2^sg
    o_fr = [_F(x) for x in np.asarray(pos, dtype=float).reshape(3)]
    uniq = np.unique(tris)
    sg = _common_shift(o_fr + [_F(x) for x in uniq])
    o_int = tuple(int(x * (1 << sg)) for x in o_fr)
    as_int = {float(x): int(_F(x) * (1 << sg)) for x in uniq}
    v_int = [[as_int[float(x)] for x in row] for row in tris]
    tv_i, e1_i, e2_i, keep = [], [], [], []
    for k, r in enumerate(v_int):
        e1 = (r[3] - r[0], r[4] - r[1], r[5] - r[2])
        e2 = (r[6] - r[0], r[7] - r[1], r[8] - r[2])
        tv_i.append((o_int[0] - r[0], o_int[1] - r[1], o_int[2] - r[2]))
        e1_i.append(e1)
        e2_i.append(e2)
        if any(_cross(e1, e2)):                               # zero-area triangles hit nothing
            keep.append(k)
    if not keep:
        return out
    keep = np.array(keep)

    def to_float(vecs):
        return np.array([[float(Fraction(c, 1 << sg)) for c in vecs[k]] for k in keep]).reshape(-1, 3)

    tv, e1, e2 = to_float(tv_i), to_float(e1_i), to_float(e2_i)
    n_vec = np.cross(e2, e1)          # det = d . (e2 x e1)
    m_vec = np.cross(e2, tv)          # N_u = d . (e2 x tv)
    q_vec = np.cross(tv, e1)          # N_v = d . (tv x e1)
    n_t = np.einsum("ij,ij->i", e2, q_vec)
    E = np.maximum(np.abs(e1).sum(1), np.abs(e2).sum(1))
    T = np.abs(tv).sum(1)
    K_tri = E * (T + E)               # times D per pixel
    K_t = T * E * E
    det_floor = np.maximum(1.0, POS_RES * E)

    # integer scales: det, N_u, N_v, N_w (true) = int / s_num ; N_t (true) = int / 2^(3 sg)
    s_num = d_den * (1 << (2 * sg))
    s_n, s_d = s_num.numerator, s_num.denominator
    sg3 = 1 << (3 * sg)

    def exact_pair(py, px, k):
        """None: not even the delta-grown triangle is hit.  Else (t (1 + tau) if the hit is demanded else None,
        max(t, 0) (1 - tau), max(t, 0), t if demanded else None, u, v)."""
        d = d_int[py][px]
        a, b, tvk = e1_i[k], e2_i[k], tv_i[k]
        p = _cross(d, b)
        det = _dot(a, p)
        if det == 0:
            return None
        s = 1 if det > 0 else -1
        nu = s * _dot(tvk, p)
        q = _cross(tvk, a)
        nv = s * _dot(d, q)
        nt = s * _dot(b, q)
        adet = s * det
        nw = adet - nu - nv
        kk = int(np.searchsorted(keep, k))
        D = float(np.abs(d_flt[py * W + px]).sum())
        K = D * K_tri[kk]
        # tolerances in the integers' units, as fractions a / b with b > 0: x < -tol  <=>  x b < -a
        ta, tb = float(C_TOL * K).as_integer_ratio()
        ta, tb = ta * s_n, tb * s_d
        tta, ttb = float(C_TOL * K_t[kk]).as_integer_ratio()
        tta *= sg3
        if nu * tb < -ta or nv * tb < -ta or nw * tb < -ta or nt * ttb <= -tta:
            return None
        t_f = float(Fraction(nt * (1 << sd), adet * (1 << sg)) * f_focal)
        nt_true, adet_true = abs(nt) / sg3, (adet * s_d) / s_n
        tau = np.inf if nt_true == 0.0 or adet_true == 0.0 else \
            (C_TOL + C_FLOAT) * (K_t[kk] / nt_true + K / adet_true) + TAU_FLOOR
        closed = nu >= 0 and nv >= 0 and nw >= 0 and nt > 0
        fa, fb = float(det_floor[kk]).as_integer_ratio()
        demanded = closed and adet * tb * fb > ta * fa and nt * ttb > tta
        t_pos = max(t_f, 0.0)
        lo = t_pos * max(1.0 - tau, 0.0) if tau < 1.0 else 0.0
        hi = t_f * (1.0 + tau) if demanded else None
        return (hi, lo, t_pos, t_f if demanded else None, nu / adet, nv / adet)

    # ---- the float pass, in blocks of pixels
    P = W * H
    D_all = np.abs(d_flt).sum(1)
    step = max(1, _CHUNK // max(1, len(keep)))
    for p0 in range(0, P, step):
        d = d_flt[p0:p0 + step]
        D = D_all[p0:p0 + step, None]
        det = d @ n_vec.T
        s = np.where(det < 0, -1.0, 1.0)
        adet = np.abs(det)
        a = s * (d @ m_vec.T)
        b = s * (d @ q_vec.T)
        c = (adet - a) - b
        h = s * n_t[None, :]
        K = D * K_tri[None, :]
        Ef, tol = C_FLOAT * K, C_TOL * K
        Eft, tolt = (C_FLOAT * K_t)[None, :], (C_TOL * K_t)[None, :]
        sign_known = adet > Ef
        resolved = (adet > tol * det_floor[None, :] + Ef) & (h > tolt + Eft)
        sure = (a > Ef) & (b > Ef) & (c > Ef) & resolved
        out_of_reach = sign_known & ((a < -tol - Ef) | (b < -tol - Ef) | (c < -tol - Ef) | (h < -tolt - Eft))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            t = h / adet
            tau = (C_TOL + C_FLOAT) * (K_t[None, :] / np.abs(h) + K / adet) + TAU_FLOOR
            hi = np.where(sure, t * (1.0 + tau), np.inf)
            lo = np.where(sure, t * np.maximum(1.0 - tau, 0.0), np.inf)
            tz = np.where(sure, t, np.inf)
        rows = np.arange(len(d))
        best = np.argmin(tz, axis=1)
        z_best = tz[rows, best]
        hi_min, lo_min = hi.min(1), lo.min(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            ub = np.where(np.isfinite(z_best), a[rows, best] / adet[rows, best], np.nan)
            vb = np.where(np.isfinite(z_best), b[rows, best] / adet[rows, best], np.nan)
        tri_best = np.where(np.isfinite(z_best), keep[best], -1)
        z_ex, z_di = z_best.copy(), z_best.copy()
        # undecided pairs that can still matter: anything whose t is not surely beyond the pixel's nearest sure hit
        with np.errstate(invalid="ignore"):
            surely_farther = resolved & (t * np.maximum(1.0 - tau, 0.0) * (1.0 - 2.0 ** -40) > hi_min[:, None])
        todo = np.argwhere(~sure & ~out_of_reach & ~surely_farther)
        out.n_pairs += det.size
        out.n_exact_pairs += len(todo)
        for r, kk in todo:
            pix = p0 + int(r)
            res = exact_pair(pix // W, pix % W, int(keep[kk]))
            if res is None:
                continue
            p_hi, p_lo, t_dil, t_dem, u_, v_ = res
            lo_min[r] = min(lo_min[r], p_lo)
            z_di[r] = min(z_di[r], t_dil)
            if p_hi is not None:
                hi_min[r] = min(hi_min[r], p_hi)
                if t_dem < z_ex[r]:
                    z_ex[r], tri_best[r], ub[r], vb[r] = t_dem, keep[kk], u_, v_
        sl = slice(p0, p0 + len(d))
        out.z_hi.reshape(-1)[sl] = hi_min
        out.z_lo.reshape(-1)[sl] = lo_min
        out.z_exact.reshape(-1)[sl] = z_ex
        out.z_dilated.reshape(-1)[sl] = z_di
        out.tri.reshape(-1)[sl] = tri_best
        out.bary.reshape(-1, 2)[sl, 0] = ub
        out.bary.reshape(-1, 2)[sl, 1] = vb
    return out
