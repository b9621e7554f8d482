"""The path-clearance definition in numpy float64 (test infrastructure), on top of tests/clearance_checker.py: the
expression tree of the PATH CLEARANCE part of agri-fly_amd/csrc/afe_clearance.hip's header comment, operation for
operation.  Every sample is answered by the checker's unbounded point query (every point against every triangle): no
hierarchy, no bound, no batches -- what the kernel's pruning may never change.
"""
import numpy as np

from tests import clearance_checker as ck

INF = np.inf

RECORD_DTYPE = np.dtype([("min_dist2", np.float64), ("closest", np.float64, (3,)), ("t_min", np.float64),
                         ("t_first_hit", np.float64), ("k_min", np.int64), ("tri_min", np.int64),
                         ("k_first_hit", np.int64), ("tri_first_hit", np.int64), ("n_hit", np.int64),
                         ("n_nonfinite", np.int64)])


def empty_records(n):
    r = np.zeros(n, RECORD_DTYPE)
    r["min_dist2"] = INF
    r["closest"] = np.nan
    r["t_min"] = np.nan
    r["t_first_hit"] = np.nan
    for k in ("k_min", "tri_min", "k_first_hit", "tri_first_hit"):
        r[k] = -1
    return r


def assert_records_equal(got, want):
    """field by field and bit for bit in value (a NaN equals a NaN, which a comparison of whole records would not grant)"""
    assert got.shape == want.shape
    for name in RECORD_DTYPE.names:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)


def sample_times(t_begin, t_end, n_samples):
    """t [K]: t_begin + (t_end - t_begin) * (k / (K - 1)) for k < K - 1, t_end itself for the last"""
    K = int(n_samples)
    assert K >= 2
    tb, te = np.float64(t_begin), np.float64(t_end)
    with np.errstate(all="ignore"):
        k = np.arange(K, dtype=np.float64)
        t = tb + (te - tb) * (k / np.float64(K - 1))
    t[K - 1] = te
    return t


def sample_points(coeffs, t_begin, t_end, origin=None, rot=None, n_samples=64):
    """one path: coeffs [6, 3] (t^5 .. t^0 per axis), origin [3] or None, rot [9] row-major or None -> t [K], w [3, K]"""
    c = np.asarray(coeffs, np.float64)
    t = sample_times(t_begin, t_end, n_samples)
    with np.errstate(all="ignore"):
        p = []
        for axis in range(3):
            v = np.full(t.shape, c[0, axis])
            for j in range(1, 6):
                v = v * t + c[j, axis]
            p.append(v)
        if rot is not None:
            assert origin is not None
            R, o = np.asarray(rot, np.float64).reshape(9), np.asarray(origin, np.float64)
            w = [o[r] + ((R[3 * r] * p[0] + R[3 * r + 1] * p[1]) + R[3 * r + 2] * p[2]) for r in range(3)]
        elif origin is not None:
            o = np.asarray(origin, np.float64)
            w = [o[r] + p[r] for r in range(3)]
        else:
            w = p
    return t, np.stack(w)


def camera_pose(pos, att, mount=None):
    """afe_camera_pose_kernel's arithmetic (afe_render.hip) for one vehicle: pos [3] and att [4] already in double (the
    anchors added) -> origin [3], row-major camera-to-world matrix [9] of att * mount"""
    q = [np.float64(x) for x in att]
    m = [np.float64(x) for x in ((1.0, 0.0, 0.0, 0.0) if mount is None else mount)]
    two = np.float64(2.0)
    with np.errstate(all="ignore"):
        c0 = m[0] * q[0] - m[1] * q[1] - m[2] * q[2] - m[3] * q[3]
        c1 = m[1] * q[0] + m[0] * q[1] + m[3] * q[2] - m[2] * q[3]
        c2 = m[2] * q[0] - m[3] * q[1] + m[0] * q[2] + m[1] * q[3]
        c3 = m[3] * q[0] + m[2] * q[1] - m[1] * q[2] + m[0] * q[3]
        r0, r1, r2, r3 = c0 * c0, c1 * c1, c2 * c2, c3 * c3
        R = [r0 + r1 - r2 - r3, two * c1 * c2 - two * c0 * c3, two * c1 * c3 + two * c0 * c2,
             two * c1 * c2 + two * c0 * c3, r0 - r1 + r2 - r3, two * c2 * c3 - two * c0 * c1,
             two * c1 * c3 - two * c0 * c2, two * c2 * c3 + two * c0 * c1, r0 - r1 - r2 + r3]
    return np.array([np.float64(x) for x in pos]), np.array(R)


def sample_answers(triangles, coeffs, t_range, origin=None, rot=None, n_samples=64):
    """The per-sample part, once for any radius and max_dist: dict of t [n, K], finite [n, K] and the unbounded point
    query's d2 [n, K], tri [n, K], closest [n, 3, K].  coeffs [n, 6, 3]; t_range [2, n]; origin [3, n]; rot [9, n]."""
    c = np.asarray(coeffs, np.float64)
    n, K = c.shape[0], int(n_samples)
    tr = np.asarray(t_range, np.float64)
    ts, ws = np.empty((n, K)), np.empty((n, 3, K))
    for i in range(n):
        o = None if origin is None else np.asarray(origin, np.float64)[:, i]
        R = None if rot is None else np.asarray(rot, np.float64)[:, i]
        ts[i], ws[i] = sample_points(c[i], tr[0, i], tr[1, i], o, R, K)
    pts = ws.transpose(1, 0, 2).reshape(3, n * K)
    d2, tri, closest = ck.query(triangles, pts)
    return dict(t=ts, finite=np.isfinite(ws).all(axis=1), d2=d2.reshape(n, K), tri=tri.reshape(n, K),
                closest=closest.reshape(3, n, K).transpose(1, 0, 2))


def reduce_records(ans, radius, max_dist=INF, sampled=None):
    """records [n] (RECORD_DTYPE) and n_colliding from sample_answers' output; sampled [n] bool: False = the empty record"""
    n, K = ans["d2"].shape
    radius2 = np.float64(radius) * np.float64(radius)
    max_dist2 = np.float64(max_dist) * np.float64(max_dist)
    rec = empty_records(n)
    for i in range(n):
        if sampled is not None and not sampled[i]:
            continue
        d2, tri, t = ans["d2"][i], ans["tri"][i], ans["t"][i]
        r = rec[i]
        r["n_nonfinite"] = int((~ans["finite"][i]).sum())
        hit = d2 <= radius2
        r["n_hit"] = int(hit.sum())
        if hit.any():
            k = int(np.nonzero(hit)[0][0])
            r["k_first_hit"], r["tri_first_hit"], r["t_first_hit"] = k, tri[k], t[k]
        near = (d2 < INF) & (d2 <= max_dist2)        # (a non-finite sample's +inf is no distance, whatever max_dist)
        if near.any():
            k = int(np.argmin(np.where(near, d2, INF)))        # the first (lowest k) of the smallest
            if near[k]:
                r["min_dist2"], r["k_min"], r["tri_min"], r["t_min"] = d2[k], k, tri[k], t[k]
                r["closest"] = ans["closest"][i][:, k]
    return rec, int((rec["n_hit"] > 0).sum())


def audit(triangles, coeffs, t_range, origin=None, rot=None, n_samples=64, radius=0.116, max_dist=INF, sampled=None):
    """the whole definition: records [n], n_colliding"""
    return reduce_records(sample_answers(triangles, coeffs, t_range, origin, rot, n_samples), radius, max_dist, sampled)
