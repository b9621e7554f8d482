"""Scenes and rays for the ray-query tests (tests/test_raycast_cpu.py, tests/test_gpu_raycast.py): small meshes (every
brute-force comparison stays far below 2e7 ray-triangle pairs) and rays aimed at what a hierarchy can get wrong."""
import importlib

import numpy as np

from tests import render_scenes as rs

scen = importlib.import_module("agri-fly_amd").scenarios


def lattice_scene():
    """a wall at x = 3 on a 1/4 m lattice (alternating diagonals) and a wall behind it: 514 triangles, axis-parallel rays
    run along shared edges and through vertices"""
    wall = rs.lattice_wall((0.0, 0.0, 1.0), (0, -1, 0), (0, 0, -1), (1, 0, 0), 3.0, 0.25, 2.0, 2.0)
    behind = rs.quad((5.0, -40.0, -40.0), (0.0, 80.0, 0.0), (0.0, 0.0, 80.0))
    return np.concatenate([wall, behind]).astype(np.float32)


def hanging_scene():
    """rectangles hanging at 2.3 .. 8 m in front of an empty background, at every tilt, and one far wall: 34 triangles"""
    rng = np.random.default_rng(17)
    tris = []
    for _ in range(16):
        c = np.array([rng.uniform(2.3, 8.0), rng.uniform(-3, 3), rng.uniform(0.2, 3.0)])
        a, b = rng.normal(size=3), rng.normal(size=3)
        a *= rng.uniform(0.3, 1.5) / np.linalg.norm(a)
        b = np.cross(a, b)
        b *= rng.uniform(0.3, 1.5) / np.linalg.norm(b)
        tris.append(rs.quad(c - 0.5 * a - 0.5 * b, a, b))
    tris.append(rs.quad((12.0, -10.0, -2.0), (0.0, 20.0, 0.0), (0.0, 0.0, 9.0)))
    return np.concatenate(tris).astype(np.float32)


def orchard_scene():
    return scen.orchard_mesh(rows=2, cols=2, seed=5)


def coincident_scene():
    """300 copies of one triangle (every hit ties 300 ways: index 0 must win) in front of a wall"""
    one = np.array([[3, -1, 0, 3, 1, 0, 3, 0, 2]], np.float32)
    return np.concatenate([np.repeat(one, 300, 0), rs.quad((4.0, -3.0, -1.0), (0.0, 6.0, 0.0), (0.0, 0.0, 5.0)).astype(np.float32)])


def degenerate_scene():
    """a closed box whose list is interleaved with triangles that hit nothing: coincident vertices (all three, two of
    three), collinear ones, and a sliver 1.2e-7 m high, which is NOT degenerate"""
    box = rs.closed_box((-2, -2, 0.0), (2, 2, 2.5))
    junk = np.array([[0, 0, 1, 0, 0, 1, 0, 0, 1],                  # a point
                     [1, 0, 1, 1, 0, 1, 1, 1, 1.5],                # two vertices coincide
                     [-1, -1, 0.5, 0, 0, 1.0, 1, 1, 1.5],          # collinear
                     [0.5, -1, 1, 0.5, 1, 1, 0.5, 0, 1],           # collinear, the third vertex between the others
                     [1.5, -1, 1, 1.5, 1, 1, 1.5, 1, 1.0000001]], np.float32)
    out = []
    for k in range(len(box)):
        out.append(box[k])
        out.append(junk[k % len(junk)])
    return np.array(out, np.float32)


SCENES = {"lattice": lattice_scene, "hanging": hanging_scene, "orchard": orchard_scene, "coincident": coincident_scene,
          "degenerate": degenerate_scene}
_CACHE = {}


def scene(name):
    if name not in _CACHE:
        _CACHE[name] = np.ascontiguousarray(SCENES[name](), dtype=np.float32).reshape(-1, 9)
    return _CACHE[name]


def _bounds(tris):
    v = tris.reshape(-1, 3).astype(np.float64)
    return v.min(0), v.max(0)


def random_rays(tris, n=4096, seed=1):
    """origins inside the scene's box (half) and up to one box size outside it (half); directions of any length, a third
    of them aimed at a point of the box.  -> origin, dir [3, n]"""
    rng = np.random.default_rng(seed)
    lo, hi = _bounds(tris)
    size = np.maximum(hi - lo, 0.5)
    inside = rng.uniform(lo, hi, (n, 3))
    outside = rng.uniform(lo - size, hi + size, (n, 3))
    o = np.where((np.arange(n) % 2 == 0)[:, None], inside, outside)
    d = rng.normal(size=(n, 3)) * rng.choice([1e-3, 1.0, 50.0], (n, 1))
    aim = rng.uniform(lo, hi, (n, 3)) - o
    d = np.where((np.arange(n) % 3 == 0)[:, None], aim, d)
    return np.ascontiguousarray(o.T), np.ascontiguousarray(d.T)


def structured_rays(tris, n_tri=64, seed=2):
    """Rays at what culling can get wrong, for up to n_tri triangles chosen at random: towards every vertex, edge midpoint
    and centroid; along the edges; along and inside the faces of the triangles' boxes (every face of a node's box is a
    face of one of these); through box corners; axis-parallel with +0 and -0 components; starting inside the boxes.
    Origins lie on a 1/8 m lattice, so for lattice meshes the differences are exact.  -> origin, dir [3, n]"""
    rng = np.random.default_rng(seed)
    lo_s, hi_s = _bounds(tris)
    pick = rng.choice(len(tris), min(n_tri, len(tris)), replace=False)
    O, D = [], []

    def ray(o, d):
        O.append(np.asarray(o, np.float64))
        D.append(np.asarray(d, np.float64))

    for k in pick:
        v = tris[k].reshape(3, 3).astype(np.float64)
        lo, hi = v.min(0), v.max(0)
        mid = 0.5 * (lo + hi)
        eye = np.round(rng.uniform(lo_s - 1.0, hi_s + 1.0) * 8.0) / 8.0
        for target in (v[0], v[1], v[2], 0.5 * (v[0] + v[1]), 0.5 * (v[1] + v[2]), 0.5 * (v[2] + v[0]), (v[0] + v[1] + v[2]) / 3.0):
            ray(eye, target - eye)
        for i, j in ((0, 1), (1, 2), (2, 0)):                  # along the edge, from before its start
            e = v[j] - v[i]
            ray(v[i] - 1.5 * e, e)
        for ax in range(3):
            u, w = (ax + 1) % 3, (ax + 2) % 3
            for face in (lo, hi):
                o = mid.copy(); o[ax] = face[ax]; o[u] = lo[u] - 1.0       # in the face's plane, from outside the box, along u
                d = np.zeros(3); d[u] = 1.0
                ray(o, d)
                o = mid.copy(); o[ax] = face[ax]                           # inside the face, along w, a -0 beside the +0
                d = np.array([0.0, 0.0, 0.0]); d[w] = -1.0; d[u] = -0.0
                ray(o, d)
            o = mid.copy(); o[ax] -= 2.0                                    # axis-parallel through the box's middle
            d = np.array([-0.0, 0.0, -0.0]); d[ax] = 1.0
            ray(o, d)
            d = np.array([0.0, -0.0, 0.0]); d[ax] = -0.5
            ray(o + 4.0 * np.eye(3)[ax], d)
        ray(eye, lo - eye)                                                  # through the box's corners
        ray(eye, hi - eye)
        ray(lo - (hi - lo), hi - lo)                                        # along its diagonal: every slab entered at once
        ray(mid, rng.normal(size=3))                                        # from inside the box
        ray(mid, v[rng.integers(3)] - mid)
        ray((v[0] + v[1] + v[2]) / 3.0, rng.normal(size=3))                 # from ON the triangle: it does not hit itself
    return np.ascontiguousarray(np.array(O).T), np.ascontiguousarray(np.array(D).T)
