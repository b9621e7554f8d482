"""The mesh-clearance definition in numpy float64 (test infrastructure): every point against every triangle, the
expression tree of agri-fly_amd/csrc/afe_clearance.hip's header comment operation for operation.  numpy rounds every
elementwise operation separately (no contraction), and only + - * / and comparisons appear, so the same tree gives the
same bits as the kernel.  No hierarchy, no pruning: what the kernel's boxes may never change.
"""
import numpy as np

INF = np.inf


def _dot(u, v):
    return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]


def _clamp(w):
    return np.where(w < 0.0, 0.0, np.where(w > 1.0, 1.0, w))


def tri_tables(triangles):
    """a, ab, ac [3, T] in double and the definition's degenerate flag [T], from float32 triangles [T, 9]"""
    t = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 3, 3).astype(np.float64)
    a = t[:, 0].T.copy()
    ab = t[:, 1].T - a
    ac = t[:, 2].T - a
    n0 = ab[1] * ac[2] - ab[2] * ac[1]
    n1 = ab[2] * ac[0] - ab[0] * ac[2]
    n2 = ab[0] * ac[1] - ab[1] * ac[0]
    nn = n0 * n0 + n1 * n1 + n2 * n2
    degenerate = ~(nn > 1e-24 * (_dot(ab, ab) * _dot(ac, ac)))
    return a, ab, ac, degenerate


def _tail(ab, ac, ap, s, t):
    m = [ab[k] * s + ac[k] * t for k in range(3)]
    q = [ap[k] - m[k] for k in range(3)]
    return _dot(q, q)


def evaluate(a, ab, ac, degenerate, p):
    """dist2, s, t of the definition for broadcastable operands (a, ab, ac, p: [3, ...]; degenerate: [...]).
    dist2 is +inf where the definition gives nothing that is < +inf."""
    with np.errstate(all="ignore"):
        ap = [p[k] - a[k] for k in range(3)]
        bp = [ap[k] - ab[k] for k in range(3)]
        cp = [ap[k] - ac[k] for k in range(3)]
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        shape = np.broadcast(d1, degenerate).shape
        zero, one = np.zeros(shape), np.ones(shape)
        r_a = (d1 <= 0.0) & (d2 <= 0.0)
        r_b = (d3 >= 0.0) & (d4 <= d3)
        vc = d1 * d4 - d3 * d2
        den_ab = d1 - d3
        r_ab = (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0) & (den_ab > 0.0)
        r_c = (d6 >= 0.0) & (d5 <= d6)
        vb = d5 * d2 - d1 * d6
        den_ac = d2 - d6
        r_ac = (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0) & (den_ac > 0.0)
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        den_bc = e43 + e56
        r_bc = (va <= 0.0) & (e43 >= 0.0) & (e56 >= 0.0) & (den_bc > 0.0)
        den = (va + vb) + vc
        r_in = den > 0.0
        r = 1.0 / den
        t_bc = e43 / den_bc
        conds = [r_a, r_b, r_ab, r_c, r_ac, r_bc, r_in]
        s = np.select(conds, [zero, one, d1 / den_ab, zero, zero, 1.0 - t_bc, vb * r], 0.0)
        t = np.select(conds, [zero, zero, zero, one, d2 / den_ac, t_bc, vc * r], 0.0)
        accepted = r_a | r_b | r_ab | r_c | r_ac | r_bc | r_in
        d = _tail(ab, ac, ap, s, t)
        d = np.where(accepted & ~degenerate & (d < INF), d, INF)
        d, s, t = (np.array(np.broadcast_to(x, shape)) for x in (d, s, t))
        # the segment rule for what is left
        todo = ~(d < INF)
        if todo.any():
            def pick(x):
                return np.broadcast_to(x, shape)[todo]
            fab, fac, fap, fbp = ([pick(v[k]) for k in range(3)] for v in (ab, ac, ap, bp))
            fd1, fd2 = pick(d1), pick(d2)
            e = [fac[k] - fab[k] for k in range(3)]
            l_ab, l_ac, l_bc = _dot(fab, fab), _dot(fac, fac), _dot(e, e)
            w_ab = np.where(l_ab > 0.0, _clamp(fd1 / l_ab), 0.0)
            w_ac = np.where(l_ac > 0.0, _clamp(fd2 / l_ac), 0.0)
            w_bc = np.where(l_bc > 0.0, _clamp(_dot(e, fbp) / l_bc), 0.0)
            fd = np.full(fd1.shape, INF)
            fs, ft = np.zeros(fd1.shape), np.zeros(fd1.shape)
            for ss, tt in ((w_ab, np.zeros_like(w_ab)), (np.zeros_like(w_ac), w_ac), (1.0 - w_bc, w_bc)):
                dd = _tail(fab, fac, fap, ss, tt)
                better = dd < fd
                fd = np.where(better, dd, fd)
                fs = np.where(better, ss, fs)
                ft = np.where(better, tt, ft)
            d[todo], s[todo], t[todo] = fd, fs, ft
        return d, s, t


def pair_dist2(triangles, points):
    """triangle k against point k: triangles [N, 9] float32, points [3, N] -> dist2 [N], closest [3, N]"""
    a, ab, ac, deg = tri_tables(triangles)
    p = np.asarray(points, np.float64)
    d, s, t = evaluate(a, ab, ac, deg, p)
    closest = np.stack([a[k] + (ab[k] * s + ac[k] * t) for k in range(3)])
    return d, closest


def query(triangles, pos, max_dist=INF, pairs_per_chunk=1 << 21):
    """The whole query: pos [3, n] -> dist2 [n], tri [n] int32, closest [3, n]; no triangle within max_dist (or a
    non-finite point): +inf, -1, NaN."""
    a, ab, ac, deg = tri_tables(triangles)
    p = np.ascontiguousarray(pos, dtype=np.float64)
    n, n_tri = p.shape[1], a.shape[1]
    max_dist2 = np.float64(max_dist) * np.float64(max_dist)
    dist2 = np.full(n, INF)
    tri = np.full(n, -1, np.int32)
    closest = np.full((3, n), np.nan)
    finite = np.isfinite(p).all(axis=0)
    step = max(1, pairs_per_chunk // max(n_tri, 1))
    A, AB, AC = a[:, None, :], ab[:, None, :], ac[:, None, :]
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        sel = np.nonzero(finite[lo:hi])[0] + lo
        if sel.size == 0:
            continue
        q = p[:, sel]
        d, s, t = evaluate(A, AB, AC, deg[None, :], q[:, :, None])
        win = np.argmin(d, axis=1)                      # the first (lowest-index) smallest
        rows = np.arange(sel.size)
        dw, sw, tw = d[rows, win], s[rows, win], t[rows, win]
        ok = (dw < INF) & (dw <= max_dist2)
        k = sel[ok]
        w = win[ok]
        dist2[k] = dw[ok]
        tri[k] = w
        for c in range(3):
            closest[c, k] = a[c, w] + (ab[c, w] * sw[ok] + ac[c, w] * tw[ok])
    return dist2, tri, closest


class MonitorTwin:
    """What afe_contact_monitor latches, from downloaded states and the checker."""

    NEVER = np.uint64(0xffffffffffffffff)

    def __init__(self, triangles, n, contact_radius, search_radius):
        self.triangles = triangles
        self.n = n
        self.contact2 = np.float64(contact_radius) * np.float64(contact_radius)
        self.search = search_radius
        self.reset(0, n, first_time=True)

    def reset(self, first=0, count=None, first_time=False):
        if first_time:
            self.min_dist2 = np.full(self.n, INF)
            self.first_us = np.full(self.n, self.NEVER, np.uint64)
            self.first_tri = np.full(self.n, -1, np.int32)
            return
        count = self.n - first if count is None else count
        self.min_dist2[first:first + count] = INF
        self.first_us[first:first + count] = self.NEVER
        self.first_tri[first:first + count] = -1

    def update(self, pos, now_us):
        d2, tri, _ = query(self.triangles, pos, self.search)
        self.min_dist2 = np.minimum(self.min_dist2, d2)
        now = d2 <= self.contact2
        fresh = now & (self.first_us == self.NEVER)
        self.first_us[fresh] = np.uint64(now_us)
        self.first_tri[fresh] = tri[fresh]
        return int(now.sum()), int((self.first_us != self.NEVER).sum())
