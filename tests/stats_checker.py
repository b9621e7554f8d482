"""The definition of the ensemble statistics (agri-fly_amd/csrc/afe_stats.hip states it; this is the same, operation for
operation, in numpy float64).  It works from what Ensemble.get_state() returns plus the engine time.  Device and checker may
differ in the sign of a zero and in nothing else, so compare with numpy.testing.assert_array_equal."""
import numpy as np

NEVER = np.uint64(0xffffffffffffffff)
INT_FIELDS = ("count", "n_invalid", "n_grounded", "n_ever_invalid", "n_ever_grounded", "sum_n_valid", "argmax_h2", "argmax_peak_h2")
FLOAT_FIELDS = ("sum_h2", "sum_dz", "sum_dz2", "sum_v2", "sum_w2", "max_h2", "min_dz", "max_dz", "max_v2", "max_w2", "min_up",
                "sum_peak_h2", "sum_acc_h2", "max_peak_h2", "min_min_up")
DTYPE = np.dtype([(k, np.int64) for k in INT_FIELDS] + [(k, np.float64) for k in FLOAT_FIELDS])


def tree_sum(leaves):
    """THE tree: at level s = 1, 2, 4, ... while s < n, for every j that is a multiple of 2s with j + s < n:
    a[j] = a[j] + a[j+s]; the sum is a[0]; an empty array sums to +0.0"""
    a = np.array(leaves, dtype=np.float64)
    n = a.size
    if n == 0:
        return np.float64(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        s = 1
        while s < n:
            j = np.arange(0, n - s, 2 * s)
            a[j] = a[j] + a[j + s]
            s *= 2
    return a[0]


def chunked_tree_sum(leaves, width=256):
    """the form the kernels compute: the tree over each aligned run of `width` leaves, then the same over the run totals"""
    a = np.array(leaves, dtype=np.float64)
    while a.size > width:
        a = np.array([tree_sum(a[k:k + width]) for k in range(0, a.size, width)])
    return tree_sum(a)


def quantities(state, ref):
    """per-vehicle quantities from get_state()'s dict (float64, planar) and the reference points [3, n]"""
    pos, vel, att, w = (np.asarray(state[k], np.float64) for k in ("pos", "vel", "att", "ang_vel"))
    ref = np.asarray(ref, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = pos[0] - ref[0], pos[1] - ref[1], pos[2] - ref[2]
        h2 = dx * dx + dy * dy
        dz2 = dz * dz
        v2 = (vel[0] * vel[0] + vel[1] * vel[1]) + vel[2] * vel[2]
        w2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
        up = ((att[0] * att[0] - att[1] * att[1]) - att[2] * att[2]) + att[3] * att[3]
    valid = (np.isfinite(pos).all(0) & np.isfinite(vel).all(0) & np.isfinite(att).all(0) & np.isfinite(w).all(0) &
             np.isfinite(dx) & np.isfinite(dy) & np.isfinite(dz))
    grounded = valid & (pos[2] <= 0)
    return dict(h2=h2, dz=dz, dz2=dz2, v2=v2, w2=w2, up=up, valid=valid, grounded=grounded)


class Latches:
    def __init__(self, n):
        self.peak_h2 = np.zeros(n)
        self.min_up = np.full(n, np.inf)
        self.acc_h2 = np.zeros(n)
        self.n_valid = np.zeros(n, np.int64)
        self.first_grounded_us = np.full(n, NEVER, np.uint64)
        self.first_invalid_us = np.full(n, NEVER, np.uint64)

    def reset(self, first, count):
        sl = slice(first, first + count)
        self.peak_h2[sl] = 0.0
        self.min_up[sl] = np.inf
        self.acc_h2[sl] = 0.0
        self.n_valid[sl] = 0
        self.first_grounded_us[sl] = NEVER
        self.first_invalid_us[sl] = NEVER

    def as_dict(self, first=0, count=None):
        sl = slice(first, None if count is None else first + count)
        return {k: getattr(self, k)[sl] for k in ("peak_h2", "min_up", "acc_h2", "n_valid", "first_grounded_us", "first_invalid_us")}


def _max(x):     # a candidate replaces only if strictly greater, from -inf: a NaN never replaces
    x = x[~np.isnan(x)]
    return np.max(x, initial=-np.inf)


def _min(x):
    x = x[~np.isnan(x)]
    return np.min(x, initial=np.inf)


def _argmax(x, first):   # the lowest index holding the maximum, -1 with no candidate
    return -1 if x.size == 0 else first + int(np.flatnonzero(x == _max(x))[0])


def update(state, ref, latches, edges, now_us, hist_edges=None):
    """one afe_stats_update: updates `latches` (grouped vehicles only) and returns (records [n_groups] of DTYPE,
    histogram int64 [n_groups, len(hist_edges) + 1] or None)"""
    q = quantities(state, ref)
    edges = np.asarray(edges, np.int64)
    n_groups = edges.size - 1
    rec = np.zeros(n_groups, DTYPE)
    e2 = None
    if hist_edges is not None and len(hist_edges):
        e = np.asarray(hist_edges, np.float64)
        e2 = e * e
    hist = None if e2 is None else np.zeros((n_groups, e2.size + 1), np.int64)
    L = latches
    for g in range(n_groups):
        a, b = int(edges[g]), int(edges[g + 1])
        sl = slice(a, b)
        ok, gr = q["valid"][sl], q["grounded"][sl]
        h2, up = q["h2"][sl], q["up"][sl]
        with np.errstate(over="ignore", invalid="ignore"):
            L.peak_h2[sl] = np.where(ok & (h2 > L.peak_h2[sl]), h2, L.peak_h2[sl])
            L.min_up[sl] = np.where(ok & (up < L.min_up[sl]), up, L.min_up[sl])
            L.acc_h2[sl] = np.where(ok, L.acc_h2[sl] + h2, L.acc_h2[sl])
        L.n_valid[sl] += ok
        L.first_grounded_us[sl] = np.where(gr & (L.first_grounded_us[sl] == NEVER), np.uint64(now_us), L.first_grounded_us[sl])
        L.first_invalid_us[sl] = np.where(~ok & (L.first_invalid_us[sl] == NEVER), np.uint64(now_us), L.first_invalid_us[sl])
        r = rec[g]
        r["count"] = b - a
        r["n_invalid"] = int((~ok).sum())
        r["n_grounded"] = int(gr.sum())
        r["n_ever_invalid"] = int((L.first_invalid_us[sl] != NEVER).sum())
        r["n_ever_grounded"] = int((L.first_grounded_us[sl] != NEVER).sum())
        r["sum_n_valid"] = int(L.n_valid[sl].sum())
        for k in ("h2", "dz", "dz2", "v2", "w2"):
            r["sum_" + k] = tree_sum(np.where(ok, q[k][sl], 0.0))
        r["max_h2"], r["argmax_h2"] = _max(h2[ok]), (-1 if not ok.any() else a + int(np.flatnonzero(ok & (h2 == _max(h2[ok])))[0]))
        r["min_dz"], r["max_dz"] = _min(q["dz"][sl][ok]), _max(q["dz"][sl][ok])
        r["max_v2"], r["max_w2"] = _max(q["v2"][sl][ok]), _max(q["w2"][sl][ok])
        r["min_up"] = _min(up[ok])
        r["sum_peak_h2"], r["sum_acc_h2"] = tree_sum(L.peak_h2[sl]), tree_sum(L.acc_h2[sl])
        r["max_peak_h2"], r["argmax_peak_h2"] = _max(L.peak_h2[sl]), _argmax(L.peak_h2[sl], a)
        r["min_min_up"] = _min(L.min_up[sl])
        if hist is not None:
            bins = (e2[:, None] <= h2[ok][None, :]).sum(0)
            hist[g] = np.bincount(bins, minlength=e2.size + 1)
    return rec, hist
