"""The swept-clearance definition in numpy float64 (test infrastructure), on top of tests/clearance_checker.py: the
expression tree of the SWEPT CLEARANCE part of agri-fly_amd/csrc/afe_clearance.hip's header comment, operation for
operation.  Every segment against every triangle: no hierarchy, no bound, no batches -- what the kernel's pruning may
never change.
"""
import numpy as np

from tests import clearance_checker as ck
from tests import path_checker as pc

INF = np.inf

SEGMENT_DTYPE = np.dtype([("dist2", np.float64), ("s", np.float64), ("closest", np.float64, (3,)), ("tri", np.int32),
                          ("kind", np.int32)])
SWEEP_DTYPE = np.dtype(pc.RECORD_DTYPE.descr + [("s_min", np.float64), ("s_first_hit", np.float64)])


def empty_segments(n):
    r = np.zeros(n, SEGMENT_DTYPE)
    r["dist2"] = INF
    r["s"] = np.nan
    r["closest"] = np.nan
    r["tri"] = -1
    r["kind"] = -1
    return r


def empty_sweeps(n):
    r = np.zeros(n, SWEEP_DTYPE)
    r["min_dist2"] = INF
    for k in ("closest", "t_min", "t_first_hit", "s_min", "s_first_hit"):
        r[k] = np.nan
    for k in ("k_min", "tri_min", "k_first_hit", "tri_first_hit"):
        r[k] = -1
    return r


def assert_equal(got, want):
    """field by field and bit for bit in value (a NaN equals a NaN)"""
    assert got.shape == want.shape
    for name in want.dtype.names:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)


def evaluate(a, ab, ac, degenerate, p0, p1):
    """One triangle against one segment, broadcastable operands (a, ab, ac, p0, p1: [3, ...]; degenerate: [...]) ->
    dist2 (+inf: nothing below +inf), s, kind, closest [3, ...]."""
    with np.errstate(all="ignore"):
        d = [p1[k] - p0[k] for k in range(3)]
        A = ck._dot(d, d)
        u0 = [p0[k] - a[k] for k in range(3)]
        shape = np.broadcast(A, degenerate, u0[0]).shape
        moving = np.broadcast_to(A > 0.0, shape)
        best = np.full(shape, INF)
        best_s = np.zeros(shape)
        kind = np.zeros(shape, np.int32)
        closest = [np.zeros(shape) for _ in range(3)]

        def take(better, dd, s, k, c):
            nonlocal best, best_s, kind
            best = np.where(better, dd, best)
            best_s = np.where(better, s, best_s)
            kind = np.where(better, np.int32(k), kind)
            for axis in range(3):
                closest[axis] = np.where(better, c[axis], closest[axis])

        def point(x, s, k, allowed):
            dd, ss, tt = ck.evaluate(a, ab, ac, degenerate, x)
            c = [a[axis] + (ab[axis] * ss + ac[axis] * tt) for axis in range(3)]
            take(allowed & (dd < best), dd, s, k, c)

        # candidates 0, 1: the end points
        point(p0, 0.0, 0, np.ones(shape, bool))
        point(p1, 1.0, 1, moving)
        # candidate 2: where the segment crosses the triangle's plane
        u1 = [p1[k] - a[k] for k in range(3)]
        n = [ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]]
        h0, h1 = ck._dot(n, u0), ck._dot(n, u1)
        crossing = moving & ~degenerate & (((h0 > 0.0) & (h1 < 0.0)) | ((h0 < 0.0) & (h1 > 0.0)))
        s2 = h0 / (h0 - h1)
        x = [np.where(crossing, p0[k] + d[k] * s2, p0[k]) for k in range(3)]      # (elsewhere: any finite point, not taken)
        point(x, s2, 2, crossing)
        # candidates 3, 4, 5: the segment against AB, AC, BC in the a-frame
        zero = [0.0, 0.0, 0.0]
        for side, (o, g) in enumerate(((zero, ab), (zero, ac), (ab, [ac[k] - ab[k] for k in range(3)]))):
            r = [u0[k] - o[k] for k in range(3)]
            E, F, Cc, B = ck._dot(g, g), ck._dot(g, r), ck._dot(d, r), ck._dot(d, g)
            s_end0 = ck._clamp(-Cc / A)
            s_end1 = ck._clamp((B - Cc) / A)
            den = A * E - B * B
            s_in = np.where(den > 0.0, ck._clamp((B * F - Cc * E) / den), 0.0)
            t_in = (B * s_in + F) / E
            has_len = E > 0.0
            t = np.where(has_len, np.where(t_in < 0.0, 0.0, np.where(t_in > 1.0, 1.0, t_in)), 0.0)
            s = np.where(has_len, np.where(t_in < 0.0, s_end0, np.where(t_in > 1.0, s_end1, s_in)), s_end0)
            q = [(r[k] + d[k] * s) - g[k] * t for k in range(3)]
            dd = ck._dot(q, q)
            c = [a[k] + (o[k] + g[k] * t) for k in range(3)]
            take(moving & (dd < best), dd, s, 3 + side, c)
        return best, best_s, kind, np.stack([np.broadcast_to(x, shape) for x in closest])


def _near_pairs(tlo, thi, P0, P1):
    """(segment, triangle) pairs that can win or tie, sorted by segment, then triangle.  U = the smallest, over the
    triangles, of the largest distance between the segment's box and the triangle's box is at least the segment's distance
    to the mesh; a triangle whose box is farther from the segment's box than that (by 1e-6 of it and 1e-9 m^2, a million
    times the rounding of the definition at these scales) is farther than the winner."""
    slo, shi = np.minimum(P0, P1), np.maximum(P0, P1)
    lb, ub = 0.0, 0.0
    for k in range(3):
        gap = np.maximum(np.maximum(tlo[k][None, :] - shi[k][:, None], 0.0), slo[k][:, None] - thi[k][None, :])
        far = np.maximum(thi[k][None, :] - slo[k][:, None], shi[k][:, None] - tlo[k][None, :])
        lb = lb + gap * gap
        ub = ub + far * far
    u = ub.min(axis=1)
    return np.nonzero(lb <= (u * (1.0 + 1e-6) + 1e-9)[:, None])


def query(triangles, p0, p1, max_dist=INF, pairs_per_chunk=1 << 19, cull=False):
    """The whole query: p0, p1 [3, n] -> records [n] (SEGMENT_DTYPE); no triangle within max_dist (or a non-finite
    coordinate): +inf, NaN, NaN, -1, -1.  cull=False is the definition as it stands, every segment against every triangle.
    cull=True leaves out the pairs _near_pairs proves irrelevant, for the audits of thousands of chords (the two are compared
    bit for bit in tests/test_swept_cpu.py)."""
    a, ab, ac, deg = ck.tri_tables(triangles)
    P0 = np.ascontiguousarray(p0, dtype=np.float64)
    P1 = np.ascontiguousarray(p1, dtype=np.float64)
    n, n_tri = P0.shape[1], a.shape[1]
    rec = empty_segments(n)
    finite = np.isfinite(P0).all(axis=0) & np.isfinite(P1).all(axis=0)
    step = max(1, (8 if cull else 1) * pairs_per_chunk // max(n_tri, 1))
    Aa, AB, AC = a[:, None, :], ab[:, None, :], ac[:, None, :]
    if cull:
        v = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 3, 3).astype(np.float64)
        tlo, thi = v.min(axis=1).T, v.max(axis=1).T
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        sel = np.nonzero(finite[lo:hi])[0] + lo
        if sel.size == 0:
            continue
        if cull:
            si, ti = _near_pairs(tlo, thi, P0[:, sel], P1[:, sel])
            d, s, kind, closest = evaluate(a[:, ti], ab[:, ti], ac[:, ti], deg[ti], P0[:, sel[si]], P1[:, sel[si]])
            starts = np.searchsorted(si, np.arange(sel.size))
            assert (si[starts] == np.arange(sel.size)).all()          # every segment kept a triangle
            dmin = np.minimum.reduceat(d, starts)
            at = np.minimum.reduceat(np.where(d == dmin[si], np.arange(d.size), d.size), starts)     # the first of the smallest
            at = np.minimum(at, d.size - 1)
            dw, sw_, kw, win, cw = d[at], s[at], kind[at], ti[at], closest[:, at].T
        else:
            d, s, kind, closest = evaluate(Aa, AB, AC, deg[None, :], P0[:, sel, None], P1[:, sel, None])
            win = np.argmin(d, axis=1)                      # the first (lowest-index) smallest
            rows = np.arange(sel.size)
            dw, sw_, kw, cw = d[rows, win], s[rows, win], kind[rows, win], closest[:, rows, win].T
        ok = dw < INF
        k = sel[ok]
        rec["dist2"][k] = dw[ok]
        rec["s"][k] = sw_[ok]
        rec["kind"][k] = kw[ok]
        rec["tri"][k] = win[ok]
        rec["closest"][k] = cw[ok]
    return bounded(rec, max_dist)


def bounded(rec, max_dist):
    """the definition's rule for max_dist on unbounded records: a winner with dist2 <= max_dist^2 stays what it is, any
    other segment has no triangle"""
    max_dist2 = np.float64(max_dist) * np.float64(max_dist)
    out = rec.copy()
    out[~(rec["dist2"] <= max_dist2)] = empty_segments(1)[0]
    return out


class SweptMonitorTwin(ck.MonitorTwin):
    """What the swept afe_contact_monitor latches, from downloaded states and the checker: the segment from the position
    of the vehicle's last update to the current one; none yet (creation, reset, a non-finite position): the point."""

    def __init__(self, triangles, n, contact_radius, search_radius):
        super().__init__(triangles, n, contact_radius, search_radius)
        self.prev = np.zeros((3, n))
        self.prev_valid = np.zeros(n, bool)

    def reset(self, first=0, count=None, first_time=False):
        super().reset(first, count, first_time)
        if not first_time:
            count = self.n - first if count is None else count
            self.prev_valid[first:first + count] = False

    def update(self, pos, now_us):
        p1 = np.ascontiguousarray(pos, dtype=np.float64)
        p0 = np.where(self.prev_valid[None, :], self.prev, p1)
        rec = query(self.triangles, p0, p1, self.search)
        self.prev = p1.copy()
        self.prev_valid = np.isfinite(p1).all(axis=0)
        d2, tri = rec["dist2"], rec["tri"]
        self.min_dist2 = np.minimum(self.min_dist2, d2)
        now = d2 <= self.contact2
        fresh = now & (self.first_us == self.NEVER)
        self.first_us[fresh] = np.uint64(now_us)
        self.first_tri[fresh] = tri[fresh]
        self.last = rec
        return int(now.sum()), int((self.first_us != self.NEVER).sum())


def chord_answers(triangles, coeffs, t_range, origin=None, rot=None, n_samples=64):
    """The per-chord part, once for any radius and max_dist: dict of t [n, K], finite [n, K-1] and the unbounded segment
    query's records [n, K-1].  Arguments as path_checker.sample_answers."""
    c = np.asarray(coeffs, np.float64)
    n, K = c.shape[0], int(n_samples)
    tr = np.asarray(t_range, np.float64)
    ts, ws = np.empty((n, K)), np.empty((n, 3, K))
    for i in range(n):
        o = None if origin is None else np.asarray(origin, np.float64)[:, i]
        R = None if rot is None else np.asarray(rot, np.float64)[:, i]
        ts[i], ws[i] = pc.sample_points(c[i], tr[0, i], tr[1, i], o, R, K)
    p0 = ws[:, :, :-1].transpose(1, 0, 2).reshape(3, n * (K - 1))
    p1 = ws[:, :, 1:].transpose(1, 0, 2).reshape(3, n * (K - 1))
    rec = query(triangles, p0, p1, cull=True).reshape(n, K - 1)
    return dict(t=ts, finite=np.isfinite(ws[:, :, :-1]).all(axis=1) & np.isfinite(ws[:, :, 1:]).all(axis=1), rec=rec)


def reduce_records(ans, radius, max_dist=INF, sampled=None):
    """records [n] (SWEEP_DTYPE) and n_colliding from chord_answers' output; sampled [n] bool: False = the empty record"""
    n = ans["rec"].shape[0]
    radius2 = np.float64(radius) * np.float64(radius)
    max_dist2 = np.float64(max_dist) * np.float64(max_dist)
    out = empty_sweeps(n)
    for i in range(n):
        if sampled is not None and not sampled[i]:
            continue
        rec, t = ans["rec"][i], ans["t"][i]
        d2, tri = rec["dist2"], rec["tri"]
        with np.errstate(all="ignore"):
            time = t[:-1] + (t[1:] - t[:-1]) * rec["s"]
        r = out[i]
        r["n_nonfinite"] = int((~ans["finite"][i]).sum())
        hit = d2 <= radius2
        r["n_hit"] = int(hit.sum())
        if hit.any():
            k = int(np.nonzero(hit)[0][0])
            r["k_first_hit"], r["tri_first_hit"], r["t_first_hit"], r["s_first_hit"] = k, tri[k], time[k], rec["s"][k]
        near = (d2 < INF) & (d2 <= max_dist2)
        if near.any():
            k = int(np.argmin(np.where(near, d2, INF)))        # the first (lowest k) of the smallest
            if near[k]:
                r["min_dist2"], r["k_min"], r["tri_min"], r["t_min"], r["s_min"] = d2[k], k, tri[k], time[k], rec["s"][k]
                r["closest"] = rec["closest"][k]
    return out, int((out["n_hit"] > 0).sum())


def audit(triangles, coeffs, t_range, origin=None, rot=None, n_samples=64, radius=0.116, max_dist=INF, sampled=None):
    """the whole swept audit: records [n], n_colliding"""
    return reduce_records(chord_answers(triangles, coeffs, t_range, origin, rot, n_samples), radius, max_dist, sampled)


def recipe_segments(triangles, n=1536, seed=11, n_ground=2):
    """the test recipe: start = centroid of a random non-ground triangle + normal(0, 0.3 m), direction uniform on the
    sphere, length log-uniform in [0.02, 1] m -> p0, p1 [3, n].  The order of the draws is this function's own: on the
    2 x 3 orchard it gives a hit share of 0.45 at 0.116 m, winners by kind 692 / 501 / 218 / 31 / 34 / 60, 52 hits with both
    ends clear and 325 interior s (printed by tests/test_swept_cpu.py) -- this implementation's figures, close to but not
    those of the prototype the recipe was first tried with (0.44; 659 / 563 / 224 / 17 / 22 / 51; 63; 296)."""
    rng = np.random.default_rng(seed)
    v = np.asarray(triangles, np.float32).reshape(-1, 3, 3).astype(np.float64)
    pick = rng.integers(n_ground, len(v), n)
    p0 = v[pick].mean(axis=1) + rng.normal(0.0, 0.3, (n, 3))
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    length = np.exp(rng.uniform(np.log(0.02), np.log(1.0), n))
    p1 = p0 + u * length[:, None]
    return np.ascontiguousarray(p0.T), np.ascontiguousarray(p1.T)
