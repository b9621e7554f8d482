"""Swept clearance, the part that needs no GPU: the ABI additions, the numpy statement of the definition
(tests/swept_checker.py) against dense sampling and on hand-built cases, and the host-side chord deviation bound."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

from tests import clearance_checker as ck
from tests import path_checker as pc
from tests import swept_checker as sw
from tests.test_gpu_path_clearance import random_paths

afa = importlib.import_module("agri-fly_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIUS = 0.116

NEW_NAMES = ["afe_clearance_segments", "afe_clearance_segments_stats", "afe_contact_monitor_create_swept", "afe_clearance_paths_swept",
             "afe_clearance_paths_swept_stats", "afe_clearance_plans_engine_swept", "afe_path_chord_deviation"]


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
    assert afa.SEGMENT_CLEARANCE_DTYPE.itemsize == 48 and afa.PATH_SWEEP_DTYPE.itemsize == 112 <= 128
    assert afa.SEGMENT_CLEARANCE_DTYPE == sw.SEGMENT_DTYPE and afa.PATH_SWEEP_DTYPE == sw.SWEEP_DTYPE
    for name in ("path_chord_deviation",):
        assert hasattr(afa, name)
    for name in ("segments", "segments_stats", "paths_swept", "paths_swept_stats", "plans_engine_swept"):
        assert hasattr(afa.ClearanceMap, name)
    # NULL handles are refused with a status, without a GPU
    p = np.zeros((3, 1))
    out = np.zeros(1, afa.SEGMENT_CLEARANCE_DTYPE)
    st = np.zeros(4, np.uint64)
    assert L.afe_clearance_segments(None, 1, p.ctypes.data, p.ctypes.data, 1.0, out.ctypes.data, None) == 1
    assert L.afe_clearance_segments_stats(None, 1, p.ctypes.data, p.ctypes.data, 1.0, st.ctypes.data, None) == 1
    h = C.c_void_p()
    assert L.afe_contact_monitor_create_swept(None, None, 0.1, 0.2, C.byref(h)) == 1 and not h
    c, tr = np.zeros((1, 6, 3)), np.array([[0.0], [1.0]])
    rec = np.zeros(1, afa.PATH_SWEEP_DTYPE)
    assert L.afe_clearance_paths_swept(None, 1, c.ctypes.data, tr.ctypes.data, None, None, 8, 0.1, 1.0, rec.ctypes.data, None, None) == 1
    assert L.afe_clearance_paths_swept_stats(None, 1, c.ctypes.data, tr.ctypes.data, None, None, 8, 0.1, 1.0, st.ctypes.data, None) == 1
    plans = np.zeros(1, afa.PLAN_DTYPE)
    assert L.afe_clearance_plans_engine_swept(None, None, 0, 1, None, plans.ctypes.data, 8, 0.1, 1.0, rec.ctypes.data, None, None) == 1
    b = C.c_double(-1.0)
    assert L.afe_path_chord_deviation(None, 0.0, 1.0, None, 8, C.byref(b)) == 1
    assert L.afe_path_chord_deviation(c.ctypes.data, 0.0, 1.0, None, 8, None) == 1
    for K in (1, 0, -3, 4097):
        assert L.afe_path_chord_deviation(c.ctypes.data, 0.0, 1.0, None, K, C.byref(b)) == 4
    assert b.value == -1.0


@pytest.fixture(scope="module")
def recipe():
    tris = afa.scenarios.orchard_mesh(rows=2, cols=3, seed=3)
    p0, p1 = sw.recipe_segments(tris)
    return tris, p0, p1, sw.query(tris, p0, p1)


def test_recipe_exercises_every_candidate(recipe):
    tris, p0, p1, rec = recipe
    assert len(tris) == 578
    hit = rec["dist2"] <= RADIUS * RADIUS
    kinds = np.bincount(rec["kind"], minlength=6)
    ends_clear = (ck.query(tris, p0)[0] > RADIUS * RADIUS) & (ck.query(tris, p1)[0] > RADIUS * RADIUS)
    interior = (rec["s"] > 0) & (rec["s"] < 1)
    print("hit share %.2f, winners by kind %s, hits with both ends clear %d, interior s %d" %
          (hit.mean(), kinds.tolist(), (hit & ends_clear).sum(), interior.sum()))
    assert 0.2 <= hit.mean() <= 0.8 and (kinds >= 10).all() and (hit & ends_clear).sum() >= 20
    assert np.isfinite(rec["dist2"]).all() and (rec["dist2"] >= 0).all() and ((rec["s"] >= 0) & (rec["s"] <= 1)).all()


def test_never_larger_than_dense_sampling(recipe):
    tris, p0, p1, rec = recipe
    w = np.linspace(0.0, 1.0, 257)
    n = p0.shape[1]
    # 257 point queries per segment.  A triangle whose box is farther from the segment's box than the nearer end point is
    # from the mesh cannot hold any sample's nearest point, so it is left out of that segment's queries (exactly, with 1 mm
    # to spare): 1 536 small queries instead of one of 228 million pairs
    v = tris.reshape(-1, 3, 3).astype(np.float64)
    tlo, thi = v.min(axis=1), v.max(axis=1)
    ends = np.minimum(ck.query(tris, p0)[0], ck.query(tris, p1)[0])
    slo, shi = np.minimum(p0, p1).T, np.maximum(p0, p1).T
    dense = np.empty(n)
    for i in range(n):
        gap = np.maximum(np.maximum(tlo - shi[i], 0.0), slo[i] - thi)
        near = np.nonzero((gap * gap).sum(axis=1) <= (np.sqrt(ends[i]) + 1e-3) ** 2)[0]
        pts = p0[:, i, None] + (p1 - p0)[:, i, None] * w[None, :]
        dense[i] = ck.query(tris[near], pts)[0].min()
        assert dense[i] <= ends[i]
    excess = rec["dist2"] - dense
    print("swept - dense: max %.3g (never positive), min %.3g (what 257 samples miss)" % (excess.max(), excess.min()))
    assert (excess <= 0).all()
    # the closest point and s are where the distance says they are
    x = p0 + (p1 - p0) * rec["s"]
    back = ((x - rec["closest"].T) ** 2).sum(axis=0)
    assert np.abs(back - rec["dist2"]).max() <= 1e-12


def test_culled_checker_is_the_checker(recipe):
    """swept_checker.query(cull=True), which the audits of thousands of chords use, against the definition as it stands"""
    tris, p0, p1, rec = recipe
    sw.assert_equal(sw.query(tris, p0, p1, cull=True), rec)
    long0, long1 = p0[:, :64], p0[:, 64:128]                       # segments across the scene, and points
    sw.assert_equal(sw.query(tris, long0, long1, cull=True), sw.query(tris, long0, long1))
    sw.assert_equal(sw.query(tris, long0, long0, 0.5, cull=True), sw.query(tris, long0, long0, 0.5))


def test_zero_length_segments_are_the_point_query(recipe):
    tris, p0, _, _ = recipe
    p = p0[:, :300].copy()
    p[0, 3], p[1, 4], p[2, 5] = np.nan, np.inf, -np.inf
    for max_dist in (np.inf, 0.5):
        rec = sw.query(tris, p, p, max_dist)
        d2, tri, closest = ck.query(tris, p, max_dist)
        np.testing.assert_array_equal(rec["dist2"], d2)
        np.testing.assert_array_equal(rec["tri"], tri)
        np.testing.assert_array_equal(rec["closest"], closest.T)
        found = tri >= 0
        assert (rec["kind"][found] == 0).all() and (rec["s"][found] == 0).all() and (rec["kind"][~found] == -1).all()
        assert 0 < found.sum() < 300 or max_dist == np.inf


def _one(tri, p0, p1):
    rec = sw.query(np.array([tri], np.float32), np.array(p0, float)[:, None], np.array(p1, float)[:, None])
    return rec[0]


FACE = [0, 0, 0, 4, 0, 0, 0, 4, 0]          # a = origin, b on x, c on y, in the plane z = 0


def test_hand_built_cases():
    r = _one(FACE, [1, 1, 1], [1.5, 1.2, -2])                     # pierces the face
    assert r["kind"] == 2 and r["dist2"] < 1e-20 and 0 < r["s"] < 1 and abs(r["closest"][2]) == 0
    r = _one(FACE, [0.5, 1, 0.25], [2, 1.5, 0.25])                # parallel above the face: every point ties, the first wins
    assert r["kind"] == 0 and r["dist2"] == 0.0625 and r["s"] == 0 and tuple(r["closest"]) == (0.5, 1.0, 0.0)
    r = _one(FACE, [1, 1, 0.5], [2, 1.5, 0.25])                   # descending over the face: the lower end
    assert r["kind"] == 1 and r["dist2"] == 0.0625 and r["s"] == 1
    # crossing over an edge outside the face, nearest to the edge away from where it meets the plane: AB (y < 0), AC (x < 0),
    # BC (beyond the hypotenuse).  Seen along the edge the segment runs from (2 out, 1 up) to (0.5 in, 1 down): it passes the
    # edge at |(-2, 1) x (2.5, -2)|^2 / |(2.5, -2)|^2 = 2.25 / 10.25
    want = 2.25 / 10.25
    r = _one(FACE, [2, -2, 1], [2, 0.5, -1])
    assert r["kind"] == 3 and abs(r["dist2"] - want) < 1e-15 and 0 < r["s"] < 1 and tuple(r["closest"]) == (2.0, 0.0, 0.0)
    r = _one(FACE, [-2, 2, 1], [0.5, 2, -1])
    assert r["kind"] == 4 and abs(r["dist2"] - want) < 1e-15 and 0 < r["s"] < 1 and tuple(r["closest"]) == (0.0, 2.0, 0.0)
    h = np.sqrt(0.5)
    r = _one(FACE, [2 + 2 * h, 2 + 2 * h, 1], [2 - 0.5 * h, 2 - 0.5 * h, -1])
    assert r["kind"] == 5 and abs(r["dist2"] - want) < 1e-14 and 0 < r["s"] < 1 and np.allclose(r["closest"], [2, 2, 0], atol=1e-14)
    # lying in the triangle's plane: through the face (it meets AC at (0, 1, 0) first in the candidates' order: AB is a
    # metre away, BC also gives 0 but comes later), and past it
    r = _one(FACE, [-1, 1, 0], [5, 1, 0])
    assert r["dist2"] == 0.0 and r["kind"] == 4 and tuple(r["closest"]) == (0.0, 1.0, 0.0)
    r = _one(FACE, [-2, -1, 0], [6, -1, 0])
    assert r["dist2"] == 1.0 and r["kind"] == 3
    # degenerate triangles: coincident vertices (a point, a side) and collinear ones are what they are.  The point: all
    # three sides are that point and tie, the first (AB) holds the answer
    r = _one([1, 1, 1, 1, 1, 1, 1, 1, 1], [0, 1, 1], [2, 1, 3])
    assert abs(r["dist2"] - 0.5) < 1e-15 and r["kind"] == 3 and r["s"] == 0.25 and tuple(r["closest"]) == (1.0, 1.0, 1.0)
    r = _one([0, 0, 0, 0, 0, 0, 4, 0, 0], [1, -1, 1], [3, 1, 1])           # a == b: the side AC carries it
    assert r["dist2"] == 1.0 and r["kind"] == 4 and r["s"] == 0.5
    r = _one([0, 0, 0, 2, 0, 0, 4, 0, 0], [3, -1, 2], [3, 1, 2])           # collinear: AB ends at x = 2, AC reaches x = 3, BC ties later
    assert r["dist2"] == 4.0 and r["kind"] == 4 and r["s"] == 0.5 and tuple(r["closest"]) == (3.0, 0.0, 0.0)
    assert ck.tri_tables(np.array([[0, 0, 0, 2, 0, 0, 4, 0, 0]], np.float32))[3][0]


def test_totality():
    """finite dist2 >= 0 for every finite input of the families above: random segments, in-plane ones, parallel ones, against
    good, sliver and exactly degenerate triangles"""
    rng = np.random.default_rng(13)
    n = 4000
    shapes = {"good": FACE, "sliver": [0, 0, 0, 4, 0, 0, 2, 1e-6, 0], "a==b": [1, 1, 1, 1, 1, 1, 2, 3, 4], "b==c": [1, 1, 1, 2, 3, 4, 2, 3, 4],
              "a==c": [1, 1, 1, 2, 3, 4, 1, 1, 1], "point": [1, 1, 1, 1, 1, 1, 1, 1, 1], "collinear": [1, 1, 1, 2, 3, 4, 4, 7, 10]}
    for name, t in shapes.items():
        tris = np.tile(np.array(t, np.float32), (n, 1))
        a, ab, ac, deg = ck.tri_tables(tris)
        p0 = rng.uniform(-3, 8, (3, n))
        p1 = rng.uniform(-3, 8, (3, n))
        flat = slice(0, n // 4)                     # in the plane z = 0 (the good triangle's and the sliver's)
        p0[2, flat] = 0.0
        p1[2, flat] = 0.0
        level = slice(n // 4, n // 2)               # parallel to that plane
        p1[2, level] = p0[2, level]
        short = slice(n // 2, 5 * n // 8)           # zero length
        p1[:, short] = p0[:, short]
        d, s, kind, closest = sw.evaluate(a, ab, ac, deg, p0, p1)
        assert np.isfinite(d).all() and (d >= 0).all(), name
        assert ((s >= 0) & (s <= 1)).all() and np.isfinite(closest).all() and ((kind >= 0) & (kind <= 5)).all(), name
        assert (kind[short] == 0).all(), name
        # None misses what sampling the same pair finds.  Unlike the recipe's segments, these are up to 19 m long against
        # one triangle up to 15 m away, and an exact "<=" does fail here (the good triangle: 4.4e-16 on a dist2 of 8.6, an
        # inner sample whose rounded point lies an ulp nearer than the segment).  Both sides carry the roundings the
        # definition's own argument budgets: about 40 of 2^-53 on terms bounded by |u0|^2 + |d|^2 + |ab|^2 + |ac|^2.
        w = np.linspace(0, 1, 33)
        dense = np.min([ck.evaluate(a, ab, ac, deg, p0 + (p1 - p0) * x)[0] for x in w], axis=0)
        scale = ((p0 - a) ** 2).sum(axis=0) + ((p1 - p0) ** 2).sum(axis=0) + (ab ** 2).sum(axis=0) + (ac ** 2).sum(axis=0)
        print("%s: (swept - dense) / scale: max %.3g" % (name, ((d - dense) / scale).max()))
        assert (d - dense <= 40 * 2.0 ** -53 * scale).all(), (name, ((d - dense) / scale).max())


def test_chord_deviation_bounds_the_measured_one():
    tris = afa.scenarios.orchard_mesh(rows=6, cols=8, seed=3)
    c, tr = random_paths(tris, 240)
    c, tr = c[:48], tr[:, :48]
    rng = np.random.default_rng(3)
    rot = rng.normal(0, 0.7, (9, 48))
    origin = rng.normal(0, 5.0, (3, 48))
    w = np.linspace(0.0, 1.0, 65)[None, :]
    for K in (8, 64, 200):
        for i in range(48):
            for R in (None, rot[:, i]):
                o = None if R is None else origin[:, i]
                bound = afa.path_chord_deviation(c[i], tr[0, i], tr[1, i], R, K)
                t, pts = pc.sample_points(c[i], tr[0, i], tr[1, i], o, R, K)
                # 64 sub-samples per chord: the curve there against the chord's own point at the same fraction
                fine_t = (t[:-1, None] + (t[1:] - t[:-1])[:, None] * w).reshape(-1)
                curve = np.stack([np.polyval(c[i][:, axis], fine_t) for axis in range(3)])
                if R is not None:
                    curve = o[:, None] + R.reshape(3, 3) @ curve
                chord = (pts[:, :-1, None] + (pts[:, 1:] - pts[:, :-1])[:, :, None] * w[None]).reshape(3, -1)
                measured = np.sqrt(((curve - chord) ** 2).sum(axis=0)).max()
                assert measured <= bound, (K, i, measured, bound)
                assert bound > 0 and np.isfinite(bound)
    # the spacing enters squared: K - 1 doubled, a quarter of the bound
    for i in range(48):
        b1 = afa.path_chord_deviation(c[i], tr[0, i], tr[1, i], None, 65)
        b2 = afa.path_chord_deviation(c[i], tr[0, i], tr[1, i], None, 129)
        assert abs(b2 / b1 - 0.25) <= 1e-14
