"""Mesh clearance query and contact monitor on the device against the numpy statement of the definition
(tests/clearance_checker.py): bit for bit -- distances, triangle indices and closest points."""
import ctypes as C
import importlib
import threading

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from tests import clearance_checker as ck
from tests import scenarios as tscen
from tests.scenarios import random_ensemble

afa = importlib.import_module("agri-fly_amd")
scen = afa.scenarios
pytestmark = pytest.mark.gpu

AFE_F32, AFE_F64 = afa.AFE_F32, afa.AFE_F64
NEVER = np.uint64(0xffffffffffffffff)


def _same(got, want):
    assert_array_equal(got[0], want[0])
    assert_array_equal(got[1], want[1])
    assert_array_equal(got[2], want[2])


@pytest.fixture(scope="module")
def orchard():
    tris = scen.orchard_mesh(rows=6, cols=8, seed=3)
    return tris, afa.ClearanceMap(tris)


@pytest.fixture(scope="module")
def points(orchard):
    tris, _ = orchard
    v = tris.reshape(-1, 3)
    lo, hi = v.min(0).astype(float), v.max(0).astype(float)
    rng = np.random.default_rng(21)
    n = 8000
    return np.stack([rng.uniform(lo[0] - 3, hi[0] + 3, n), rng.uniform(lo[1] - 3, hi[1] + 3, n), rng.uniform(-1, 4.5, n)])


def test_bit_parity_unbounded(orchard, points):
    tris, cmap = orchard
    info = cmap.info()
    assert info["n_tri"] == len(tris) and info["depth"] <= 32
    assert (info["n_nodes"], info["depth"]) == afa.clearance_check_hierarchy(tris)[:2]
    got = cmap.query(points)
    want = ck.query(tris, points)
    assert (want[1] >= 0).all()
    _same(got, want)
    d2_only = cmap.query(points, want_closest=False)
    assert d2_only[2] is None
    assert_array_equal(d2_only[0], want[0])
    assert_array_equal(d2_only[1], want[1])


@pytest.mark.parametrize("max_dist,lo,hi", [(0.116, 0.02, 1.0), (0.5, 0.15, 0.85), (2.0, 0.15, 0.85)])
def test_radius(orchard, points, max_dist, lo, hi):
    tris, cmap = orchard
    want = ck.query(tris, points, max_dist)
    share = (want[1] >= 0).mean()
    print("share of points within %.3f m: %.1f %%" % (max_dist, 100 * share))
    assert lo <= share <= hi          # neither branch can hide
    got = cmap.query(points, max_dist)
    _same(got, want)
    out = want[1] < 0
    assert np.isinf(got[0][out]).all() and np.isnan(got[2][:, out]).all()


def test_ties_and_surfaces():
    tris = scen.orchard_mesh(rows=2, cols=3, seed=3)
    cmap = afa.ClearanceMap(tris)
    v = tris.reshape(-1, 3, 3).astype(np.float64)
    pts = np.concatenate([v.reshape(-1, 3), (v[:, 0] + v[:, 1]) / 2, (v[:, 1] + v[:, 2]) / 2, (v[:, 0] + v[:, 2]) / 2,
                          (v[:, 0] + v[:, 1] + v[:, 2]) / 3]).T
    want = ck.query(tris, pts)
    got = cmap.query(pts)
    _same(got, want)
    # a vertex belongs to several triangles at distance exactly 0: the lowest index wins (a trunk's foot also lies in a
    # ground triangle, which comes before every triangle that names the vertex)
    n_vert = 3 * len(tris)
    assert (want[0][:n_vert] == 0).all()
    first_owner = {}
    for t, tri in enumerate(tris.reshape(-1, 3, 3)):
        for vert in tri:
            first_owner.setdefault(vert.tobytes(), t)
    owners = np.array([first_owner[x.tobytes()] for x in tris.reshape(-1, 3)])
    assert (got[1][:n_vert] <= owners).all() and (got[1][:n_vert] == owners).mean() > 0.9
    # points on box faces and corners: the scene's bounds and the triangles' own boxes
    b = cmap.info()["bounds"]
    corners = np.array([[b[0 + 3 * i], b[1 + 3 * j], b[2 + 3 * k]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    faces = np.array([[b[0], (b[1] + b[4]) / 2, 1.0], [b[3], (b[1] + b[4]) / 2, 1.0], [(b[0] + b[3]) / 2, b[1], 1.0],
                      [(b[0] + b[3]) / 2, b[4], 1.0], [(b[0] + b[3]) / 2, (b[1] + b[4]) / 2, b[5]]])
    tlo, thi = v.min(1), v.max(1)
    boxes = np.concatenate([tlo, thi, np.stack([tlo[:, 0], thi[:, 1], tlo[:, 2]], 1), np.stack([thi[:, 0], tlo[:, 1], (tlo[:, 2] + thi[:, 2]) / 2], 1)])
    p2 = np.concatenate([corners, faces, boxes]).T
    for md in (np.inf, 0.05):
        _same(cmap.query(p2, md), ck.query(tris, p2, md))
    cmap.close()


def test_degenerate_meshes():
    rng = np.random.default_rng(4)
    pts = rng.uniform(-1, 6, (3, 600))
    one = np.array([[3, -1, 0, 3, 1, 0, 3, 0, 2]], np.float32)
    many = np.concatenate([np.repeat(one, 300, 0), np.array([[2, -1, 1, 2, 1, 1, 2, 1, 1.0000001]], np.float32),
                           np.array([[4, 0, 0, 4, 0, 0, 4, 0, 0]], np.float32)])
    lo, hi = np.array([-2, -2, 0.0]), np.array([2, 2, 2.5])
    c = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], float)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    box = np.array([np.concatenate([c[a], c[b], c[d]]) for a, b, d, e in quads] +
                   [np.concatenate([c[a], c[d], c[e]]) for a, b, d, e in quads], np.float32)
    # a == b, b == c, a == c, a point, collinear: the triangles the textbook region test fails on
    broken = np.array([[1, 1, 1, 1, 1, 1, 2, 3, 4], [1, 1, 1, 2, 3, 4, 2, 3, 4], [1, 1, 1, 2, 3, 4, 1, 1, 1], [1, 1, 1, 1, 1, 1, 1, 1, 1],
                       [1, 1, 1, 2, 3, 4, 4, 7, 10]], np.float32)
    for mesh in (one, many, box, broken, broken[:1], broken[4:]):
        cmap = afa.ClearanceMap(mesh)
        assert cmap.info()["depth"] <= 32
        for md in (np.inf, 1.0):
            got = cmap.query(pts, md)
            _same(got, ck.query(mesh, pts, md))
            hit = got[1] >= 0
            assert np.isfinite(got[0][hit]).all() and (got[0][hit] >= 0).all()
        cmap.close()
    with pytest.raises(afa.AfeError):
        afa.ClearanceMap(np.full((1, 9), np.nan, np.float32))
    with pytest.raises(afa.AfeError):
        afa.ClearanceMap(np.zeros((0, 9), np.float32))


def test_non_finite_points(orchard, points):
    tris, cmap = orchard
    pts = points[:, :700].copy()
    bad = {3: (0, np.nan), 64: (1, np.inf), 65: (2, -np.inf), 255: (0, -np.inf), 256: (2, np.nan), 699: (1, np.nan)}
    for k, (axis, val) in bad.items():
        pts[axis, k] = val
    for md in (np.inf, 0.5):
        got = cmap.query(pts, md)
        for k in bad:
            assert np.isinf(got[0][k]) and got[1][k] == -1 and np.isnan(got[2][:, k]).all()
        _same(got, ck.query(tris, pts, md))            # the neighbours are what they would be alone


def _orchard_ensemble(tris, precision, n=4096, seed=11, offset=(0.0, 0.0), **kw):
    ens = random_ensemble(n, seed=seed, **kw)
    v = tris.reshape(-1, 3)
    lo, hi = v.min(0).astype(float), v.max(0).astype(float)
    rng = np.random.default_rng(seed + 1)
    ens.data.pos[0] = rng.uniform(lo[0], hi[0], n)
    ens.data.pos[1] = rng.uniform(lo[1], hi[1], n)
    ens.data.pos[2] = rng.uniform(0.2, 4.0, n)
    return ens.to_engine(precision)


@pytest.mark.parametrize("precision", [AFE_F32, AFE_F64])
def test_from_the_engine(orchard, precision):
    tris, cmap = orchard
    e = _orchard_ensemble(tris, precision)
    e.step(1000, 25)
    pos = e.get_state()["pos"]
    for md in (np.inf, 0.5):
        got = cmap.query_engine(e, md)
        _same(got, cmap.query(pos, md))
        _same(got, ck.query(tris, pos, md))
    # a sub-range, and an empty one
    first, count = 1234, 777
    sub = cmap.query_engine(e, 2.0, first=first, count=count)
    _same(sub, ck.query(tris, pos[:, first:first + count], 2.0))
    empty = cmap.query_engine(e, 2.0, first=e.n, count=0)
    assert empty[0].shape == (0,)
    with pytest.raises(afa.AfeError):
        cmap.query_engine(e, 2.0, first=e.n - 5, count=6)
    # answers kept on the device
    bufs = (afa.DeviceBuffer(count * 8), afa.DeviceBuffer(count * 4), afa.DeviceBuffer(count * 24))
    ms = cmap.query_engine(e, 2.0, first=first, count=count, out=bufs)
    assert ms >= 0
    assert_array_equal(bufs[0].download(np.float64, (count,)), sub[0])
    assert_array_equal(bufs[1].download(np.int32, (count,)), sub[1])
    assert_array_equal(bufs[2].download(np.float64, (3, count)), sub[2])
    for b in bufs:
        b.close()
    e.close()


def test_from_the_engine_far_from_the_origin():
    """fp32 state 4 km out: x and y live in the slabs relative to their anchors, the query adds them in double"""
    shift = np.array([4000.0, 4000.0, 0.0], np.float32)
    tris = (scen.orchard_mesh(rows=3, cols=4, seed=5).reshape(-1, 3) + shift).reshape(-1, 9).astype(np.float32)
    cmap = afa.ClearanceMap(tris)
    e = _orchard_ensemble(tris, AFE_F32, n=2048, seed=13)
    e.step(1000, 25)
    pos = e.get_state()["pos"]
    assert pos[0].min() > 3900
    for md in (np.inf, 1.0):
        got = cmap.query_engine(e, md)
        want = ck.query(tris, pos, md)
        _same(got, want)
    assert (want[1] >= 0).any() and (want[1] < 0).any()
    e.close()
    cmap.close()


def test_from_the_engine_in_persistent_mode(orchard):
    tris, cmap = orchard
    e = _orchard_ensemble(tris, AFE_F32, seed=17, type_ids=(5,))
    e.set_split_stepping(1)
    e.set_step_mode(afa.AFE_STEP_PERSISTENT)
    e.step(1000, 25)
    got = cmap.query_engine(e, 2.0)              # the grid ends here ...
    before = e.get_state()
    _same(got, ck.query(tris, before["pos"], 2.0))
    again = cmap.query_engine(e, 2.0)
    after = e.get_state()
    for k in before:
        assert_array_equal(before[k], after[k])   # the query does not touch the state
    _same(again, got)
    e.step(1000, 10)                              # ... and starts again
    _same(cmap.query_engine(e, 2.0), ck.query(tris, e.get_state()["pos"], 2.0))
    e.close()


def _check_latches(mon, twin, first=0, count=None):
    got = mon.get(first, count)
    count = twin.n - first if count is None else count
    assert_array_equal(got["min_dist2"], twin.min_dist2[first:first + count])
    assert_array_equal(got["first_contact_us"], twin.first_us[first:first + count])
    assert_array_equal(got["first_contact_tri"], twin.first_tri[first:first + count])


def test_monitor_scripted_crash(orchard):
    tris, cmap = orchard
    _, layout = scen.orchard_mesh(rows=6, cols=8, seed=3, return_layout=True)
    tree = layout[2 * 8 + 3]                            # a trunk inside the orchard
    n = 64
    params = afa.params_from_type(5)
    w_h = scen.hover_speed(params)
    offsets = np.linspace(-0.6, 0.6, n)
    pos0 = np.stack([np.full(n, tree[0] - 1.0), tree[1] + offsets, np.full(n, 0.5)])
    vel0 = np.stack([np.full(n, 2.0), np.zeros(n), np.zeros(n)])
    att0 = np.tile(np.array([[1.0], [0.0], [0.0], [0.0]]), (1, n))
    e = afa.Ensemble(n, precision=AFE_F32)
    e.set_type_table([params])
    e.set_state(pos0, vel0, att0, np.zeros((3, n)), np.full((4, n), w_h))
    e.set_motor_cmds(np.full((4, n), w_h, np.float32))
    mon = afa.ContactMonitor(e, cmap, 0.116, 1.0)
    twin = ck.MonitorTwin(tris, n, 0.116, 1.0)
    _check_latches(mon, twin)
    for tick in range(120):
        e.step(1000, 10)
        counts = mon.update()
        want = twin.update(e.get_state()["pos"], e.time_us)
        assert counts == want, (tick, counts, want)
        if tick % 10 == 9:
            _check_latches(mon, twin)
    _check_latches(mon, twin)
    ever = int((twin.first_us != NEVER).sum())
    print("vehicles that ever made contact: %d of %d" % (ever, n))
    assert 10 <= ever <= 54                              # both outcomes are present
    assert np.isfinite(twin.min_dist2).all()
    # a sub-range back to "nothing seen": exactly that range
    mon.reset(20, 9)
    twin.reset(20, 9)
    _check_latches(mon, twin)
    got = mon.get(20, 9)
    assert np.isinf(got["min_dist2"]).all() and (got["first_contact_us"] == NEVER).all() and (got["first_contact_tri"] == -1).all()
    counts = mon.update()
    assert counts == twin.update(e.get_state()["pos"], e.time_us)
    _check_latches(mon, twin)
    mon.close()
    e.close()


def test_monitor_in_the_real_loop():
    from tests.orchard_flight import fly_orchard
    tris, layout = scen.orchard_mesh(rows=6, cols=10, seed=0, return_layout=True)
    cmap = afa.ClearanceMap(tris)
    n, seconds = 48, 4.0
    n_ticks = int(round(seconds / 0.01))
    twin = ck.MonitorTwin(tris, n, 0.116, 1.0)
    box = {}

    def on_tick(tick, t, engine, state):
        if "mon" not in box:
            box["mon"] = afa.ContactMonitor(engine, cmap, 0.116, 1.0)
        counts = box["mon"].update()
        want = twin.update(state["pos"], engine.time_us)
        assert counts == want, (tick, counts, want)
        if tick % 50 == 0 or tick == n_ticks:
            _check_latches(box["mon"], twin)
        if tick == n_ticks:
            box["mon"].close()                       # before the engine goes

    watched = fly_orchard(afa, n=n, seconds=seconds, on_tick=on_tick)
    alone = fly_orchard(afa, n=n, seconds=seconds)
    assert_array_equal(watched["pos"], alone["pos"])     # it observes, it does not disturb
    assert_array_equal(watched["vel"], alone["vel"])
    assert np.isfinite(twin.min_dist2).any()

    # not through the checker: the trunks alone against the analytic cylinders they are inscribed in
    n_trees = len(layout)
    trunk_ix = (2 + 96 * np.arange(n_trees)[:, None] + np.arange(16)[None, :]).ravel()
    trunks = afa.ClearanceMap(tris[trunk_ix])
    pos = np.concatenate(list(watched["pos"]), axis=1)
    d2, _, _, _ = trunks.query(pos)
    dx = pos[0][None, :] - layout[:, 0][:, None]
    dy = pos[1][None, :] - layout[:, 1][:, None]
    horiz = np.sqrt(dx * dx + dy * dy) - layout[:, 2][:, None]
    nearest = horiz.argmin(0)
    margin = horiz.min(0)
    r = layout[nearest, 2]
    ok = (pos[2] >= 0) & (pos[2] <= layout[nearest, 3]) & (margin <= 1.0) & (margin > 0)
    print("logged samples within 1 m of a trunk and below its top: %d" % ok.sum())
    assert ok.sum() >= 100
    dist = np.sqrt(d2[ok])
    assert (dist >= margin[ok] - 1e-6).all(), (dist - margin[ok]).min()
    assert (dist <= margin[ok] + r[ok] * (1 - np.cos(np.pi / 8)) + 1e-6).all(), (dist - margin[ok] - r[ok] * (1 - np.cos(np.pi / 8))).max()
    trunks.close()
    cmap.close()


def test_boundary_abuse_with_live_handles(orchard, points):
    tris, cmap = orchard
    L = afa.library()
    e = _orchard_ensemble(tris, AFE_F32, n=512, seed=19)
    n = 256
    pts = np.ascontiguousarray(points[:, :n])
    d2, ti, cl = np.empty(n), np.empty(n, np.int32), np.empty((3, n))
    h, eh = cmap.handle, e.handle
    q = L.afe_clearance_query
    inf = float("inf")
    assert q(h, n, None, inf, d2.ctypes.data, ti.ctypes.data, cl.ctypes.data, None) == 1
    assert q(h, n, pts.ctypes.data, inf, None, ti.ctypes.data, cl.ctypes.data, None) == 1
    assert q(h, n, pts.ctypes.data, inf, d2.ctypes.data, None, cl.ctypes.data, None) == 1
    assert q(h, -1, pts.ctypes.data, inf, d2.ctypes.data, ti.ctypes.data, None, None) == 1
    assert q(h, -2 ** 63, pts.ctypes.data, inf, d2.ctypes.data, ti.ctypes.data, None, None) == 1
    assert q(h, 2 ** 62, pts.ctypes.data, inf, d2.ctypes.data, ti.ctypes.data, None, None) == 4
    for bad in (float("nan"), 0.0, -1.0, -inf):
        assert q(h, n, pts.ctypes.data, bad, d2.ctypes.data, ti.ctypes.data, None, None) == 1
    assert q(h, 0, pts.ctypes.data, inf, d2.ctypes.data, ti.ctypes.data, None, None) == 0
    qe = L.afe_clearance_query_engine
    out = (d2.ctypes.data, ti.ctypes.data, cl.ctypes.data)
    assert qe(eh, h, 0, n, 1.0, None, ti.ctypes.data, None, 0, None) == 1
    assert qe(eh, h, -1, n, 1.0, *out, 0, None) == 1
    assert qe(eh, h, 0, -1, 1.0, *out, 0, None) == 1
    assert qe(eh, h, 2 ** 63 - 1, 2, 1.0, *out, 0, None) == 4          # first + count would wrap
    assert qe(eh, h, 2, 2 ** 63 - 1, 1.0, *out, 0, None) == 4
    assert qe(eh, h, e.n - 1, 2, 1.0, *out, 0, None) == 4
    assert qe(eh, h, 0, n, float("nan"), *out, 0, None) == 1
    assert qe(None, h, 0, n, 1.0, *out, 0, None) == 1
    assert qe(eh, None, 0, n, 1.0, *out, 0, None) == 1
    mh = C.c_void_p()
    mc = L.afe_contact_monitor_create
    assert mc(eh, h, 0.5, 0.2, C.byref(mh)) == 1                       # radii out of order
    assert mc(eh, h, 0.0, 0.2, C.byref(mh)) == 1
    assert mc(eh, h, -0.1, 0.2, C.byref(mh)) == 1
    assert mc(eh, h, 0.1, inf, C.byref(mh)) == 1
    assert mc(eh, h, float("nan"), 1.0, C.byref(mh)) == 1
    assert mc(eh, h, 0.1, 1.0, None) == 1
    assert mc(None, h, 0.1, 1.0, C.byref(mh)) == 1 and mc(eh, None, 0.1, 1.0, C.byref(mh)) == 1
    assert not mh.value
    mon = afa.ContactMonitor(e, cmap, 0.116, 1.0)
    g, r = L.afe_contact_monitor_get, L.afe_contact_monitor_reset
    assert g(mon._h, -1, 4, d2.ctypes.data, None, None) == 1
    assert g(mon._h, 0, -4, d2.ctypes.data, None, None) == 1
    assert g(mon._h, 2 ** 63 - 1, 2, d2.ctypes.data, None, None) == 4
    assert g(mon._h, 1, 2 ** 63 - 1, d2.ctypes.data, None, None) == 4
    assert g(mon._h, e.n, 1, d2.ctypes.data, None, None) == 4
    assert r(mon._h, -1, 1) == 1 and r(mon._h, 0, e.n + 1) == 4 and r(mon._h, 2 ** 63 - 1, 2 ** 63 - 1) == 4
    assert L.afe_contact_monitor_update(None, None, None) == 1
    # everything still works
    assert L.afe_contact_monitor_update(mon._h, None, None) == 0
    now, ever = mon.update()
    pos = e.get_state()["pos"]
    twin = ck.MonitorTwin(tris, e.n, 0.116, 1.0)
    assert (now, ever) == twin.update(pos, e.time_us)
    _check_latches(mon, twin)
    _same(cmap.query_engine(e, 1.0), ck.query(tris, pos, 1.0))
    mon.close()
    e.close()

    # four host threads on one map: the answers of the calls made alone
    chunks = [np.ascontiguousarray(points[:, 1000 * k:1000 * (k + 1)]) for k in range(4)]
    alone = [cmap.query(c, 2.0) for c in chunks]
    results, errors = [None] * 4, []

    def work(k):
        try:
            for _ in range(3):
                results[k] = cmap.query(chunks[k], 2.0)
        except Exception as ex:      # noqa: BLE001
            errors.append(ex)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    for k in range(4):
        _same(results[k], alone[k])


def test_at_size_once():
    """config 3's ensemble (bench.py places it west of the orchard) moved 12 m east, among the trees"""
    rows, cols, altitude, n = 6, 10, 1.2, 65536
    tris = scen.orchard_mesh(rows=rows, cols=cols, seed=0)
    cmap = afa.ClearanceMap(tris)
    rng = np.random.default_rng(0)
    lane = rng.integers(0, rows - 1, n)
    on_row = rng.random(n) < 0.5
    y0 = np.where(on_row, lane * 4.0 + rng.uniform(-0.3, 0.3, n), lane * 4.0 + 2.0 + rng.uniform(-0.8, 0.8, n))
    pos0 = np.stack([np.full(n, -4.0) + rng.uniform(-1, 0, n) + 12.0, y0, np.full(n, altitude)])
    att0 = np.tile(np.array([[1.0], [0.0], [0.0], [0.0]]), (1, n))
    params = afa.params_from_type(5)
    e = afa.Ensemble(n, precision=AFE_F32)
    e.set_type_table([params])
    e.set_state(pos0, np.zeros((3, n)), att0, np.zeros((3, n)), np.full((4, n), scen.hover_speed(params)))
    d2, tri, closest, ms = cmap.query_engine(e, 2.0)
    tscen.MEASUREMENTS["clearance_65536_ms"] = ms
    pos = e.get_state()["pos"]
    pick = np.random.default_rng(1).choice(n, 512, replace=False)
    want = ck.query(tris, pos[:, pick], 2.0)
    share = (want[1] >= 0).mean()
    print("65 536 vehicles, max_dist 2 m: %.3f ms, %.1f %% of the subsample within the radius" % (ms, 100 * share))
    assert 0.15 <= share <= 1.0
    _same((d2[pick], tri[pick], closest[:, pick]), want)
    mon = afa.ContactMonitor(e, cmap, 0.116, 2.0)
    now, ever = mon.update()
    assert now == ever == int((d2 <= np.float64(0.116) * np.float64(0.116)).sum())
    assert_array_equal(mon.get()["min_dist2"], d2)
    mon.close()
    e.close()
    cmap.close()
