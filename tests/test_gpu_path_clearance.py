"""Path clearance on the device (afe_clearance_paths, afe_clearance_plans_engine) against the numpy statement of the
definition (tests/path_checker.py): every field of every record, bit for bit."""
import ctypes as C
import importlib

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from tests import path_checker as pc
from tests.test_gpu_persistent import assert_same

afa = importlib.import_module("agri-fly_amd")
scen = afa.scenarios
pytestmark = pytest.mark.gpu

AFE_F32, AFE_F64 = afa.AFE_F32, afa.AFE_F64
RADIUS = 0.116
INF = np.inf


def random_paths(tris, n, seed=5):
    """world-frame quintics starting inside the mesh's xy box +- 1 m: coeffs [n, 6, 3], t_range [2, n]"""
    rng = np.random.default_rng(seed)
    v = tris.reshape(-1, 3)
    lo, hi = v.min(0).astype(float), v.max(0).astype(float)
    c = np.zeros((n, 6, 3))
    c[:, 5, 0] = rng.uniform(lo[0] - 1, hi[0] + 1, n)
    c[:, 5, 1] = rng.uniform(lo[1] - 1, hi[1] + 1, n)
    c[:, 5, 2] = rng.uniform(0.3, 3, n)
    d = rng.normal(size=(n, 3))
    d[:, 2] *= 0.3
    d /= np.linalg.norm(d, axis=1)[:, None]
    c[:, 4] = d * rng.uniform(0.5, 4, n)[:, None]
    c[:, 3] = rng.normal(0, 1, (n, 3))
    c[:, 2] = rng.normal(0, 0.3, (n, 3))
    c[:, 1] = rng.normal(0, 0.05, (n, 3))
    c[:, 0] = rng.normal(0, 0.01, (n, 3))
    return c, np.stack([np.zeros(n), rng.uniform(0.5, 3, n)])


@pytest.fixture(scope="module")
def orchard():
    tris = scen.orchard_mesh(rows=6, cols=8, seed=3)
    cmap = afa.ClearanceMap(tris)
    yield tris, cmap
    cmap.close()


@pytest.fixture(scope="module")
def small():
    tris = scen.orchard_mesh(rows=2, cols=3, seed=3)
    cmap = afa.ClearanceMap(tris)
    yield tris, cmap
    cmap.close()


@pytest.fixture(scope="module")
def world_paths(orchard):
    """the first 48 of the recipe's 240 paths at K = 200, and the checker's per-sample answers (computed once)"""
    tris, _ = orchard
    c, tr = random_paths(tris, 240)
    c, tr = c[:48], tr[:, :48]
    return c, tr, 200, pc.sample_answers(tris, c, tr, n_samples=200)


# ---- 1. bit parity, world-frame paths ----------------------------------------------------------------------------

def test_bit_parity_world_frame(orchard, world_paths):
    tris, cmap = orchard
    c, tr, K, ans = world_paths
    want, want_col = pc.reduce_records(ans, RADIUS)
    share = (want["n_hit"] > 0).mean()
    first_batch, later = (want["k_min"] < 64).mean(), (want["k_min"] >= 64).mean()
    print("paths with a hit at %.3f m: %.0f %%; closest approach in batch 0: %.0f %%, later: %.0f %%" %
          (RADIUS, 100 * share, 100 * first_batch, 100 * later))
    assert 0.2 <= share <= 0.8                      # neither outcome can hide
    assert first_batch >= 0.1 and later >= 0.1      # nor the carry of the minimum across batches
    got, n_col, ms = cmap.paths(c, tr, n_samples=K, radius=RADIUS)
    pc.assert_records_equal(got, want)
    assert n_col == want_col == int((got["n_hit"] > 0).sum())
    assert ms >= 0


# ---- 2. shapes ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("placed", ["origin", "origin+rot"])
@pytest.mark.parametrize("K", [2, 64, 65, 100, 4096])
def test_shapes(small, K, placed):
    tris, cmap = small
    n = 5                                           # one block and a wave of a second
    rng = np.random.default_rng(1000 + K)
    c, tr = random_paths(tris, n, seed=K)
    origin = c[:, 5].T.copy()
    c[:, 5] = rng.normal(0, 0.01, (n, 3))
    rot = rng.normal(0, 0.7, (9, n)) if placed == "origin+rot" else None
    ans = pc.sample_answers(tris, c, tr, origin, rot, K)
    for m in (1, 3, 5):
        sub = {k: v[:m] for k, v in ans.items()}
        want, want_col = pc.reduce_records(sub, RADIUS)
        got, n_col, _ = cmap.paths(c[:m], tr[:, :m], origin[:, :m], None if rot is None else rot[:, :m], n_samples=K, radius=RADIUS)
        pc.assert_records_equal(got, want)
        assert n_col == want_col
    assert np.isfinite(want["min_dist2"]).all() and (want["k_min"] < K).all()


# ---- 3. pruning changes nothing --------------------------------------------------------------------------------------

def test_max_dist_changes_nothing_it_may_not(orchard, world_paths):
    tris, cmap = orchard
    c, tr, K, ans = world_paths
    free, free_col, _ = cmap.paths(c, tr, n_samples=K, radius=RADIUS, max_dist=INF)
    assert np.isfinite(free["min_dist2"]).all()
    shares = []
    for max_dist in (2.0, 0.5, RADIUS):
        got, n_col, _ = cmap.paths(c, tr, n_samples=K, radius=RADIUS, max_dist=max_dist)
        pc.assert_records_equal(got, pc.reduce_records(ans, RADIUS, max_dist)[0])
        within = free["min_dist2"] <= np.float64(max_dist) * np.float64(max_dist)
        shares.append(within.mean())
        for f in ("min_dist2", "k_min", "tri_min", "closest", "t_min"):
            assert_array_equal(got[f][within], free[f][within], err_msg=f)
        out = got[~within]
        assert np.isinf(out["min_dist2"]).all() and (out["k_min"] == -1).all() and (out["tri_min"] == -1).all()
        assert np.isnan(out["closest"]).all() and np.isnan(out["t_min"]).all()
        for f in ("n_hit", "k_first_hit", "tri_first_hit", "t_first_hit", "n_nonfinite"):
            assert_array_equal(got[f], free[f], err_msg=f)
        assert n_col == free_col
    print("paths whose closest approach is within 2 / 0.5 / %.3f m: %s" % (RADIUS, ["%.0f %%" % (100 * s) for s in shares]))
    assert 0 < shares[-1] < 1                       # both sides of the bound are present


# ---- 4. ties ----------------------------------------------------------------------------------------------------------

def test_ties(small):
    tris, cmap = small
    K = 200
    # a level path over the open ground south of the trees: every d2 is z*z with the same bits, in every lane and batch
    level = np.zeros((1, 6, 3))
    level[0, 5] = [-9.0, -8.5, 0.5]
    level[0, 4] = [3.0, 0.2, 0.0]
    tr = np.array([[0.0], [2.5]])
    ans = pc.sample_answers(tris, level, tr, n_samples=K)
    assert (ans["d2"] == 0.25).all() and (ans["tri"] <= 1).all()
    got, _, _ = cmap.paths(level, tr, n_samples=K, radius=RADIUS)
    pc.assert_records_equal(got, pc.reduce_records(ans, RADIUS)[0])
    assert got["k_min"][0] == 0 and got["min_dist2"][0] == 0.25 and got["t_min"][0] == 0.0 and got["n_hit"][0] == 0
    # the same path, hit everywhere: the first hit is sample 0 too
    got, n_col, _ = cmap.paths(level, tr, n_samples=K, radius=0.5, max_dist=0.5)
    assert got["k_first_hit"][0] == 0 and got["n_hit"][0] == K and got["k_min"][0] == 0 and n_col == 1
    # a constant path above the diagonal the two ground triangles share: the same distance to both, the lower index wins
    v = tris[0].reshape(3, 3).astype(np.float64)
    shared = [p for p in v if any((p == q).all() for q in tris[1].reshape(3, 3).astype(np.float64))]
    assert len(shared) == 2
    rest = np.zeros((1, 6, 3))
    rest[0, 5] = 0.5 * shared[0] + 0.5 * shared[1] + [0.0, 0.0, 0.25]
    both = pc.ck.pair_dist2(tris[:2], np.repeat(rest[0, 5][:, None], 2, axis=1))[0]
    assert both[0] == both[1]
    for k in (2, 65):
        got, _, _ = cmap.paths(rest, tr, n_samples=k, radius=RADIUS)
        pc.assert_records_equal(got, pc.audit(tris, rest, tr, n_samples=k, radius=RADIUS)[0])
        assert got["tri_min"][0] == 0 and got["k_min"][0] == 0 and got["min_dist2"][0] == both[0]
    # towards a trunk (minimum in the last batch) and away from it (minimum in the first)
    _, layout = scen.orchard_mesh(rows=2, cols=3, seed=3, return_layout=True)
    tree = layout[0]
    pair = np.zeros((2, 6, 3))
    pair[0, 5] = [tree[0] - 6.0, tree[1], 0.7]
    pair[0, 4] = [2.0, 0.0, 0.0]
    pair[1, 5] = [tree[0] - 6.0 + 2.0 * 2.8, tree[1], 0.7]
    pair[1, 4] = [-2.0, 0.0, 0.0]
    tr2 = np.array([[0.0, 0.0], [2.8, 2.8]])
    want, want_col = pc.audit(tris, pair, tr2, n_samples=K, radius=RADIUS)
    assert want["k_min"][0] >= 192 and want["k_min"][1] < 64
    got, n_col, _ = cmap.paths(pair, tr2, n_samples=K, radius=RADIUS)
    pc.assert_records_equal(got, want)
    assert n_col == want_col


# ---- 5. non-finite inputs -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [65, 200])
def test_non_finite_inputs(small, K):
    tris, cmap = small
    n = 9
    c, tr = random_paths(tris, n, seed=77)
    origin = np.zeros((3, n))
    clean, clean_col, _ = cmap.paths(c, tr, origin, n_samples=K, radius=RADIUS)
    c[1, 2, 0] = np.nan               # a coefficient
    origin[2, 4] = np.inf             # an origin
    tr[1, 6] = np.nan                 # a time
    bad = [1, 4, 6]
    got, n_col, _ = cmap.paths(c, tr, origin, n_samples=K, radius=RADIUS)       # AFE_OK: a NaN is data
    want = pc.empty_records(3)
    want["n_nonfinite"] = K
    pc.assert_records_equal(got[bad], want)
    good = [i for i in range(n) if i not in bad]
    pc.assert_records_equal(got[good], clean[good])                              # the others are what they were
    pc.assert_records_equal(got, pc.audit(tris, c, tr, origin, None, K, RADIUS)[0])
    assert n_col == int((got["n_hit"] > 0).sum()) <= clean_col


# ---- 6. from the engine -----------------------------------------------------------------------------------------------

CAM_W, CAM_H = 160, 120


def _engine_with_plans(tris, precision, persistent=False, n=64, seed=9):
    """n vehicles on the 2 x 3 orchard -- three quarters flying level among the trees, a quarter nose down 0.4 m above the
    ground (nothing to plan there) -- and one real render -> plan round"""
    rng = np.random.default_rng(seed)
    v = tris.reshape(-1, 3)
    lo, hi = v.min(0).astype(float), v.max(0).astype(float)
    pos = np.stack([rng.uniform(lo[0] + 1, hi[0] - 6, n), rng.uniform(lo[1] + 1, hi[1] - 1, n), rng.uniform(0.8, 2.0, n)])
    yaw = rng.uniform(-0.5, 0.5, n)
    att = np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)])
    down = np.arange(n) % 4 == 3
    pos[2, down] = 0.4
    att[:, down] = np.array([np.cos(np.pi / 4), 0.0, np.sin(np.pi / 4), 0.0])[:, None]
    params = afa.params_from_type(5)
    e = afa.Ensemble(n, precision=precision)
    e.set_type_table([params])
    w_h = scen.hover_speed(params)
    e.set_state(pos, np.zeros((3, n)), att, np.zeros((3, n)), np.full((4, n), w_h))
    e.set_motor_cmds(np.full((4, n), w_h, np.float32))
    if persistent:
        e.set_split_stepping(1)
        e.set_step_mode(afa.AFE_STEP_PERSISTENT)
    scene = afa.Scene(tris)
    cam = afa.camera_default(CAM_W, CAM_H)
    mount = afa.camera_default_mount()
    imgs, _ = scene.render_engine(e, cam, mount)
    cfg = afa.planner_default_config(CAM_W, CAM_H, cam.depth_scale, cam.focal_length, RADIUS, 0.174, 0.5)
    vel0 = np.stack([np.zeros(n), np.zeros(n), rng.uniform(0.2, 1.5, n)])
    grav = np.tile(np.array([[0.0], [9.81], [0.0]]), (1, n))
    plans, _, _ = afa.rappids_plan(cfg, imgs, vel0, np.zeros((3, n)), grav, afa.planner_samples(3, CAM_W, CAM_H, 64))
    scene.close()
    return e, mount, afa.plans_as_array(plans).copy()


def _check_engine_audit(tris, cmap, e, mount, plans, K=65):
    n = e.n
    found = plans["found"] != 0
    print("plans found: %d of %d" % (found.sum(), n))
    assert found.any() and (~found).any()                    # both kinds of record are asked for
    assert (plans["coeffs"][found][:, 5] == 0).all()         # a plan starts at the camera
    st = e.get_state()
    origin, rot = np.empty((3, n)), np.empty((9, n))
    for i in range(n):
        origin[:, i], rot[:, i] = pc.camera_pose(st["pos"][:, i], st["att"][:, i], mount)
    tr = np.stack([np.zeros(n), plans["tf"]])
    want, want_col = pc.audit(tris, plans["coeffs"], tr, origin, rot, K, RADIUS, sampled=found)
    got, n_col, ms = cmap.plans_engine(e, plans, mount, n_samples=K, radius=RADIUS)
    pc.assert_records_equal(got, want)
    pc.assert_records_equal(got[~found], pc.empty_records(int((~found).sum())))
    assert n_col == want_col and ms >= 0
    # a sub-range: plans[i] belongs to vehicle first + i
    first, count = 5, 42
    sub, sub_col, _ = cmap.plans_engine(e, plans[first:first + count], mount, first=first, count=count, n_samples=K, radius=RADIUS)
    pc.assert_records_equal(sub, want[first:first + count])
    assert sub_col == int((want["n_hit"][first:first + count] > 0).sum())
    # sample 0 is the vehicle itself: over the one-point range [0, 0] the record's minimum is the vehicle query's answer
    still = plans.copy()
    still["tf"] = 0.0
    at0, _, _ = cmap.plans_engine(e, still, mount, n_samples=2, radius=RADIUS, max_dist=INF)
    d2, tri, closest, _ = cmap.query_engine(e, INF)
    assert (at0["k_min"][found] == 0).all()
    assert_array_equal(at0["min_dist2"][found], d2[found])
    assert_array_equal(at0["tri_min"][found], tri[found])
    assert_array_equal(at0["closest"][found], closest[:, found].T)
    return got


@pytest.mark.parametrize("precision", [AFE_F32, AFE_F64])
def test_from_the_engine(small, precision):
    tris, cmap = small
    e, mount, plans = _engine_with_plans(tris, precision)
    _check_engine_audit(tris, cmap, e, mount, plans)
    # without a mount the camera attitude is the body's
    st = e.get_state()
    n = e.n
    origin, rot = np.empty((3, n)), np.empty((9, n))
    for i in range(n):
        origin[:, i], rot[:, i] = pc.camera_pose(st["pos"][:, i], st["att"][:, i], None)
    found = plans["found"] != 0
    want, _ = pc.audit(tris, plans["coeffs"], np.stack([np.zeros(n), plans["tf"]]), origin, rot, 7, RADIUS, sampled=found)
    got, _, _ = cmap.plans_engine(e, plans, None, n_samples=7, radius=RADIUS)
    pc.assert_records_equal(got, want)
    e.close()


def test_from_the_engine_far_from_the_origin():
    """fp32 state 4 km out: x and y live in the slabs relative to their anchors, the audit adds them in double"""
    shift = np.array([4000.0, 4000.0, 0.0], np.float32)
    tris = (scen.orchard_mesh(rows=2, cols=3, seed=3).reshape(-1, 3) + shift).reshape(-1, 9).astype(np.float32)
    cmap = afa.ClearanceMap(tris)
    e, mount, plans = _engine_with_plans(tris, AFE_F32)
    assert e.get_state()["pos"][0].min() > 3900
    _check_engine_audit(tris, cmap, e, mount, plans)
    e.close()
    cmap.close()


def test_from_the_engine_in_persistent_mode(small):
    tris, cmap = small
    a, mount, plans = _engine_with_plans(tris, AFE_F32, persistent=True)
    b, _, plans_b = _engine_with_plans(tris, AFE_F32, persistent=True)
    assert_array_equal(plans.view(np.uint8), plans_b.view(np.uint8))
    a.step(1000, 20); b.step(1000, 20)
    for _ in range(20):                            # (a grid left waiting > 200 us leaves by itself: allowed, try again)
        a.step(1000, 1); b.step(1000, 1)
        a.sync()
        if a.persistent_running:
            break
    assert a.persistent_running
    cmap.plans_engine(a, plans, mount, n_samples=65, radius=RADIUS)                 # parks the grid ...
    assert not a.persistent_running
    _check_engine_audit(tris, cmap, a, mount, plans)                                # ... and reads the state after its last step
    a.step(1000, 15); b.step(1000, 15)                                              # the grid starts again
    assert_same(a, b, "steps after an audit")
    a.close(); b.close()


# ---- 7. the boundary, with live handles ----------------------------------------------------------------------------

def test_boundary_with_live_handles(small):
    tris, cmap = small
    L = afa.library()
    e, mount, plans = _engine_with_plans(tris, AFE_F32, persistent=True)
    n = 5
    c, tr = random_paths(tris, n, seed=3)
    c, tr = np.ascontiguousarray(c), np.ascontiguousarray(tr)
    origin, rot = np.zeros((3, n)), np.tile(np.eye(3).reshape(9, 1), (1, n))
    out = np.empty(e.n, afa.PATH_CLEARANCE_DTYPE)
    nc = C.c_int64(-7)
    h, eh = cmap.handle, e.handle
    P, O = out.ctypes.data, C.byref(nc)
    inf, nan = float("inf"), float("nan")

    def paths(**kw):
        a = dict(m=h, n=n, c=c.ctypes.data, t=tr.ctypes.data, o=origin.ctypes.data, r=rot.ctypes.data, K=64, radius=RADIUS, max_dist=inf, out=P, nc=O)
        a.update(kw)
        return L.afe_clearance_paths(a["m"], a["n"], a["c"], a["t"], a["o"], a["r"], a["K"], a["radius"], a["max_dist"], a["out"], a["nc"], None)

    def plans_engine(**kw):
        a = dict(e=eh, m=h, first=0, count=e.n, mount=mount.ctypes.data, p=plans.ctypes.data, K=64, radius=RADIUS, max_dist=inf, out=P, nc=O)
        a.update(kw)
        return L.afe_clearance_plans_engine(a["e"], a["m"], a["first"], a["count"], a["mount"], a["p"], a["K"], a["radius"], a["max_dist"],
                                            a["out"], a["nc"], None)

    e.step(1000, 5)
    e.sync()
    # every refusal comes before the engine is touched: the grid stays where it is (it may idle out by itself, that is all)
    for call in (paths, plans_engine):
        assert call(m=None) == 1 and call(out=None) == 1
        for K in (1, 0, -3, 4097):
            assert call(K=K) == 4
        for radius in (0.0, -1.0, nan, inf):
            assert call(radius=radius) == 1
        assert call(radius=0.5, max_dist=0.4) == 1 and call(max_dist=nan) == 1
        assert call(nc=None) == 0                     # n_colliding is optional
    assert paths(c=None) == 1 and paths(t=None) == 1
    assert paths(o=None) == 1                          # rot without origin
    assert paths(o=None, r=None) == 0 and paths(r=None) == 0
    assert paths(n=-1) == 1 and paths(n=-2 ** 63) == 1 and paths(n=2 ** 62) == 4
    nc.value = -7
    assert paths(n=0) == 0 and nc.value == 0
    assert paths(n=0, c=None, t=None, out=None) == 0
    assert plans_engine(e=None) == 1 and plans_engine(p=None) == 1
    assert plans_engine(first=-1) == 1 and plans_engine(count=-1) == 1
    assert plans_engine(first=2 ** 63 - 1, count=2) == 4            # first + count would wrap
    assert plans_engine(first=2, count=2 ** 63 - 1) == 4
    assert plans_engine(first=e.n - 1, count=2) == 4 and plans_engine(first=e.n + 1, count=0) == 4
    e.step(1000, 1)
    e.sync()
    kept = 0
    for _ in range(50):
        e.step(1000, 1)
        e.sync()
        before = e.persistent_running
        nc.value = -7
        assert plans_engine(count=0) == 0 and plans_engine(first=e.n, count=0, p=None, out=None) == 0
        assert nc.value == 0
        kept += int(before and e.persistent_running)
    assert kept >= 40, "an audit of nothing parks the resident grid (%d of 50 found it still resident)" % kept
    # everything still works
    assert plans_engine() == 0
    assert not e.persistent_running
    want, want_col, _ = cmap.plans_engine(e, plans, mount, n_samples=64, radius=RADIUS)
    pc.assert_records_equal(out, want)
    assert nc.value == want_col
    e.close()


def test_map_and_engine_on_different_devices_are_refused(small):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    tris, _ = small
    other = afa.ClearanceMap(tris, device=1)
    e, mount, plans = _engine_with_plans(tris, AFE_F32)
    with pytest.raises(afa.AfeError) as ei:
        other.plans_engine(e, plans, mount, n_samples=8, radius=RADIUS)
    assert ei.value.status == 1
    e.close()
    other.close()


# ---- 8. one pose function --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [AFE_F32, AFE_F64])
def test_camera_and_audit_place_a_vehicle_with_the_same_pose(small, ora, precision):
    """afe_render_depth_engine and afe_clearance_plans_engine form origin and matrix with one function (afe_pose.h), and it is
    the one both judges state: large turns, the camera's mount, fp32 slabs with anchors.  Neither entry hands its pose out, so
    each is taken through what it does with it.  The audit: plans whose polynomial is constant -- zero and the three unit
    vectors -- are sampled at o and at o + column j of R, and the records of those points must be the checker's at its pose.
    The camera: 64 views of one triangle must be the camera checker's images, which it renders at its pose.  The two
    judges' poses are compared directly, bit for bit."""
    tris, cmap = small
    n = 64
    rng = np.random.default_rng(41)
    pos = np.stack([rng.uniform(-60, 60, n), rng.uniform(-60, 60, n), rng.uniform(0.5, 3.0, n)])
    att = scen.random_attitudes(rng, n, max_tilt_deg=180.0)
    assert (np.abs(att[0]) < 0.5).sum() >= n // 4           # turns by more than 120 degrees are there
    params = afa.params_from_type(5)
    e = afa.Ensemble(n, precision=precision)
    e.set_type_table([params])
    e.set_state(pos, rng.normal(0, 2.0, (3, n)), att, np.zeros((3, n)), np.full((4, n), scen.hover_speed(params)))
    e.set_motor_cmds(np.full((4, n), scen.hover_speed(params), np.float32))
    e.step(1000, 5)                                          # fp32: x and y are now anchor + a non-zero offset
    mount = afa.camera_default_mount()
    assert np.abs(mount - [1.0, 0.0, 0.0, 0.0]).max() > 0.4
    st = e.get_state()
    assert (st["pos"][:2] != pos[:2]).any()
    # the judges' poses
    L = ora.render_lib()
    origin, rot = np.empty((3, n)), np.empty((9, n))
    for i in range(n):
        origin[:, i], rot[:, i] = pc.camera_pose(st["pos"][:, i], st["att"][:, i], mount)
        q, R = np.empty(4), np.empty(9)
        L.ora_quat_mul(ora._dp(np.ascontiguousarray(st["att"][:, i], dtype=float)), ora._dp(np.ascontiguousarray(mount, dtype=float)), ora._dp(q))
        L.ora_quat_to_matrix(ora._dp(q), ora._dp(R))
        assert_array_equal(R.view(np.uint64), rot[:, i].view(np.uint64))
    assert_array_equal(origin.view(np.uint64), np.ascontiguousarray(st["pos"], dtype=np.float64).view(np.uint64))
    # the camera
    one = np.array([[40.0, -90.0, -20.0, 40.0, 90.0, -20.0, 40.0, 0.0, 60.0]], np.float32)
    scene = afa.Scene(one)
    cam = afa.camera_default(16, 12)
    cam.depth_scale, cam.max_count = 0.01, 65535
    imgs, _ = scene.render_engine(e, cam, mount)
    oc = ora.render_camera(cam.width, cam.height, cam.focal_length, cam.depth_scale, cam.max_count)
    seen = 0
    for i in range(n):
        want = ora.render_depth(oc, one, st["pos"][:, i], st["att"][:, i], mount)
        assert_array_equal(imgs[i], want, err_msg="view %d" % i)
        seen += int((want < cam.max_count).any())
    assert seen >= 8                                         # the triangle is in sight of some views, out of sight of others
    assert seen <= n - 8
    scene.close()
    # the audit
    K = 2
    tr = np.stack([np.zeros(n), np.ones(n)])
    for axis in (None, 0, 1, 2):
        plans = np.zeros(n, afa.PLAN_DTYPE)
        plans["found"] = 1
        plans["tf"] = 1.0
        if axis is not None:
            plans["coeffs"][:, 5, axis] = 1.0
        want, want_col = pc.audit(tris, plans["coeffs"], tr, origin, rot, K, RADIUS)
        assert np.isfinite(want["min_dist2"]).all()
        got, n_col, _ = cmap.plans_engine(e, plans, mount, n_samples=K, radius=RADIUS)
        pc.assert_records_equal(got, want)
        assert n_col == want_col
    e.close()
