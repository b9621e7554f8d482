"""Mesh clearance, the part that needs no GPU: the ABI additions, the host-side hierarchy, and the numpy statement of
the definition (tests/clearance_checker.py) against an independent formulation and on the triangles the textbook
region test divides 0 by 0 for."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

from tests import clearance_checker as ck

afa = importlib.import_module("agri-fly_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_NAMES = ["afe_clearance_map_create", "afe_clearance_map_destroy", "afe_clearance_map_info", "afe_clearance_check_hierarchy",
             "afe_clearance_query", "afe_clearance_query_engine", "afe_contact_monitor_create", "afe_contact_monitor_update",
             "afe_contact_monitor_get", "afe_contact_monitor_reset", "afe_contact_monitor_destroy"]

# |dist2(checker) - dist2(independent)| / (|ap|^2 + |ab|^2 + |ac|^2), worst of the 2 000 seeded pairs below, measured
# on the CPU: 3.18e-16 (both sides round about 40 operations on operands of that scale; a wrong region shows as 1e-3 or
# more).  The assertion allows ten times that.
MEASURED_WORST = 3.2e-16
BOUND = 10 * MEASURED_WORST


def test_abi_additions():
    text = open(os.path.join(ROOT, "include", "agrifly_engine.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(afe_[a-z0-9_]+)\s*\(", text))
    lib = C.CDLL(afa.library_path())
    for name in NEW_NAMES:
        assert name in declared, name
        assert name in afa.ABI_FUNCTIONS, name
        assert hasattr(lib, name), "missing export: " + name
    L = afa.library()
    assert L.afe_abi_version() == 3
    # both destroyers answer NULL with a status instead of dereferencing
    assert L.afe_clearance_map_destroy(None) == 1 and L.afe_contact_monitor_destroy(None) == 1


def _degenerate_meshes():
    one = np.array([[3, -1, 0, 3, 1, 0, 3, 0, 2]], np.float32)
    many = np.concatenate([np.repeat(one, 300, 0), np.array([[2, -1, 1, 2, 1, 1, 2, 1, 1.0000001]], np.float32),
                           np.array([[4, 0, 0, 4, 0, 0, 4, 0, 0]], np.float32)])
    return one, many


def test_hierarchy_on_orchard_and_degenerate_meshes():
    tris = afa.scenarios.orchard_mesh(rows=6, cols=8, seed=3)
    n_nodes, depth, max_leaf = afa.clearance_check_hierarchy(tris)
    # leaves hold 1..4 triangles and every inner node has two children: at least n/4 leaves, at most n
    assert len(tris) / 4 - 1 <= n_nodes <= len(tris)
    assert depth <= 32 and 1 <= max_leaf <= 4
    # median splits by count: the depth is that of a balanced tree (two levels of grace)
    assert depth <= np.ceil(np.log2(len(tris) / 4)) + 2
    one, many = _degenerate_meshes()
    assert afa.clearance_check_hierarchy(one) == (0, 1, 1)
    n_nodes, depth, max_leaf = afa.clearance_check_hierarchy(many)
    assert depth <= 32 and max_leaf <= 4 and depth <= np.ceil(np.log2(len(many) / 4)) + 2
    with pytest.raises(afa.AfeError) as ei:
        afa.clearance_check_hierarchy(np.zeros((0, 9), np.float32))
    assert ei.value.status == 1
    with pytest.raises(afa.AfeError):
        afa.clearance_check_hierarchy(np.full((1, 9), np.nan, np.float32))


def _segment_dist2(p, P, Q):
    e = Q - P
    l = (e * e).sum(1)
    w = np.where(l > 0, np.clip(((p - P) * e).sum(1) / np.where(l > 0, l, 1.0), 0.0, 1.0), 0.0)
    c = P + e * w[:, None]
    return ((p - c) ** 2).sum(1)


def _independent_dist2(tri, p):
    """min over the three sides by clamped projection, and the plane's foot point when it lies inside all three edge
    half-planes; vertices taken in the rotated order b, c, a.  tri [N, 3, 3] float64, p [N, 3]."""
    A, B, Cc = tri[:, 1], tri[:, 2], tri[:, 0]
    d = np.minimum(np.minimum(_segment_dist2(p, A, B), _segment_dist2(p, B, Cc)), _segment_dist2(p, Cc, A))
    n = np.cross(B - A, Cc - A)
    nn = (n * n).sum(1)
    ok = nn > 0
    safe = np.where(ok, nn, 1.0)
    h = ((p - A) * n).sum(1)
    foot = p - n * (h / safe)[:, None]
    inside = ok.copy()
    for P, Q in ((A, B), (B, Cc), (Cc, A)):
        inside &= (np.cross(Q - P, foot - P) * n).sum(1) >= 0
    return np.where(inside, np.minimum(d, h * h / safe), d)


def _scale(tri, p):
    a, ab, ac = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    ap = p - a
    return (ap * ap).sum(1) + (ab * ab).sum(1) + (ac * ac).sum(1)


def _seeded_pairs(n=2000, seed=5):
    rng = np.random.default_rng(seed)
    out = np.empty((0, 9), np.float32)
    while len(out) < n:
        t = rng.uniform(-2, 2, (n, 3, 3)).astype(np.float32)
        t64 = t.astype(np.float64)
        edges = np.stack([t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 1], t64[:, 0] - t64[:, 2]], 1)
        longest2 = (edges * edges).sum(2).max(1)
        area2 = np.linalg.norm(np.cross(edges[:, 0], -edges[:, 2]), axis=1)
        keep = area2 / longest2 >= 1e-3                     # aspect ratio; slivers are covered by the totality cases
        out = np.concatenate([out, t[keep].reshape(-1, 9)])
    return out[:n], rng.uniform(-3, 3, (3, n))


def test_checker_against_independent_formulation():
    tris, pts = _seeded_pairs()
    d, closest = ck.pair_dist2(tris, pts)
    t64 = tris.reshape(-1, 3, 3).astype(np.float64)
    want = _independent_dist2(t64, pts.T)
    err = np.abs(d - want) / _scale(t64, pts.T)
    print("worst |d dist2| / scale over %d pairs: %.3g" % (len(d), err.max()))
    assert np.isfinite(d).all() and (d >= 0).all()
    assert err.max() <= BOUND
    # the closest point is where the distance says it is
    back = ((pts - closest) ** 2).sum(0)
    assert (np.abs(back - d) / _scale(t64, pts.T)).max() <= BOUND


def test_points_on_the_surface():
    tris, _ = _seeded_pairs(500, seed=6)
    v = tris.reshape(-1, 3, 3).astype(np.float64)
    for pts in (v[:, 0], v[:, 1], v[:, 2], (v[:, 0] + v[:, 1]) / 2, (v[:, 1] + v[:, 2]) / 2, (v[:, 0] + v[:, 2]) / 2,
                (v[:, 0] + v[:, 1] + v[:, 2]) / 3, 0.2 * v[:, 0] + 0.3 * v[:, 1] + 0.5 * v[:, 2]):
        d, _ = ck.pair_dist2(tris, pts.T)
        assert (d >= 0).all() and (d / _scale(v, pts) <= BOUND).all(), (d / _scale(v, pts)).max()


def test_totality_on_degenerate_triangles():
    """the textbook region test gives NaN for a == b (edge AB is selected and divides 0 by 0); the definition's segment
    rule measures such a triangle as the segment or point it is.  Integer coordinates: exactly degenerate in float32."""
    cases = {"a==b": [1, 1, 1, 1, 1, 1, 2, 3, 4], "b==c": [1, 1, 1, 2, 3, 4, 2, 3, 4], "a==c": [1, 1, 1, 2, 3, 4, 1, 1, 1],
             "point": [1, 1, 1, 1, 1, 1, 1, 1, 1], "collinear": [1, 1, 1, 2, 3, 4, 4, 7, 10],
             "collinear, a in the middle": [2, 3, 4, 1, 1, 1, 4, 7, 10]}
    ends = {"a==b": ([1, 1, 1], [2, 3, 4]), "b==c": ([1, 1, 1], [2, 3, 4]), "a==c": ([1, 1, 1], [2, 3, 4]),
            "point": ([1, 1, 1], [1, 1, 1]), "collinear": ([1, 1, 1], [4, 7, 10]),
            "collinear, a in the middle": ([1, 1, 1], [4, 7, 10])}
    rng = np.random.default_rng(7)
    n = 5000
    pts = rng.uniform(-3, 12, (3, n))
    for name, t in cases.items():
        tris = np.tile(np.array(t, np.float32), (n, 1))
        assert ck.tri_tables(tris[:1])[3][0], name + ": not flagged degenerate"
        d, closest = ck.pair_dist2(tris, pts)
        assert np.isfinite(d).all() and (d >= 0).all(), name
        P, Q = (np.tile(np.array(x, float), (n, 1)) for x in ends[name])
        want = _segment_dist2(pts.T, P, Q)
        scale = _scale(tris.reshape(-1, 3, 3).astype(np.float64), pts.T)
        assert (np.abs(d - want) / scale).max() <= BOUND, (name, (np.abs(d - want) / scale).max())
        assert np.isfinite(closest).all()
    # the whole query over a mesh of them: a NaN never wins, the winner is the lowest index among equals
    mesh = np.array(list(cases.values()), np.float32)
    d2, tri, cl = ck.query(mesh, pts[:, :200])
    assert np.isfinite(d2).all() and (tri >= 0).all() and np.isfinite(cl).all()
    d2b, trib, _ = ck.query(np.concatenate([mesh, mesh]), pts[:, :200])
    assert np.array_equal(d2, d2b) and np.array_equal(tri, trib)


def test_checker_radius_and_non_finite_rules():
    tris = afa.scenarios.orchard_mesh(rows=2, cols=2, seed=1)
    rng = np.random.default_rng(8)
    pts = rng.uniform(-2, 6, (3, 300))
    pts[2] = rng.uniform(0.3, 3, 300)
    pts[0, 5], pts[1, 6], pts[2, 7] = np.nan, np.inf, -np.inf
    full = ck.query(tris, pts)
    near = ck.query(tris, pts, 0.5)
    inside = full[0] <= 0.25
    assert 0 < inside.sum() < 300
    for k in range(3):
        assert np.array_equal(near[k][..., inside], full[k][..., inside])
    assert np.isinf(near[0][~inside]).all() and (near[1][~inside] == -1).all() and np.isnan(near[2][:, ~inside]).all()
    for k in (5, 6, 7):
        assert np.isinf(full[0][k]) and full[1][k] == -1 and np.isnan(full[2][:, k]).all()


def test_no_device_means_loud_failure_not_fallback():
    import torch
    tris = afa.scenarios.orchard_mesh(rows=2, cols=2, seed=1)
    if torch.cuda.is_available():
        afa.ClearanceMap(tris).close()
        return
    with pytest.raises(afa.AfeError) as ei:
        afa.ClearanceMap(tris)
    assert ei.value.status == 2  # AFE_ERR_NO_DEVICE
