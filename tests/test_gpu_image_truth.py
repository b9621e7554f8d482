"""Image ground truth on the device (afe_image_truth_paths / _plans / _candidates) against the numpy statement of the
definition (tests/truth_checker.py, which visits every pixel): every field of every record, bit for bit."""
import ctypes as C
import importlib

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from tests import truth_checker as tc

afa = importlib.import_module("agri-fly_amd")
pytestmark = pytest.mark.gpu

SIZES = [(72, 40), (200, 150), (201, 151), (320, 240)]            # 72: not a multiple of 64; 201 x 151: odd in both
N_RANDOM = {72: 40, 200: 24, 201: 24, 320: 12}
SCALE = 10.0 / 256.0


def _cfg(w, h, true_radius=0.116, planning_radius=0.174):
    return afa.planner_default_config(w, h, SCALE, w / 2.0, true_radius, planning_radius, 0.5)


def _images(w, h):
    """[3, h, w]: trunks and ground; empty sky; sky with sparse very near pixels whose counts straddle `ignore` (2 and 0)"""
    rng = np.random.default_rng(w)
    syn = afa.scenarios.synthetic_depth_image(width=w, height=h, seed=11, n_trunks=5)
    far = np.full((h, w), 255, np.uint16)
    noise = rng.integers(120, 256, (h, w)).astype(np.uint16)
    near = rng.random((h, w)) < 0.004
    noise[near] = rng.integers(0, 5, int(near.sum()))
    return np.stack([syn, far, noise])


def _line(p0, v):
    c = np.zeros((6, 3))
    c[4], c[5] = v, p0
    return c


def _random_paths(n, rng):
    c = np.zeros((n, 6, 3))
    c[:, 5] = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.2, 0.2, n), rng.uniform(0.2, 1.0, n)], 1)
    c[:, 4] = np.stack([rng.normal(0, 0.3, n), rng.normal(0, 0.2, n), rng.uniform(0.3, 1.2, n)], 1)
    c[:, 3] = rng.normal(0, 0.1, (n, 3))
    c[:, 2] = rng.normal(0, 0.03, (n, 3))
    c[:, 1] = rng.normal(0, 0.005, (n, 3))
    c[:, 0] = rng.normal(0, 0.001, (n, 3))
    return c, np.stack([np.zeros(n), rng.uniform(0.5, 3.0, n)])


def _plain_batch(w, h):
    """the reference vehicle's radii: random quintics and the special ranges and values"""
    rng = np.random.default_rng(100 + w)
    c, tr = _random_paths(N_RANDOM[w], rng)
    special = [
        (_line([0, 0, 1.0], [0, 0, 0.5]), 1.0, 1.0),                 # K = 0
        (_line([0, 0, 1.0], [0, 0, 0.5]), 2.0, 1.0),                 # K = 0
        (_line([0, 0, 1.0], [0, 0, 0.5]), 0.0, 0.05),                # K = 1
        (_line([0.05, 0, 0.6], [0, 0, 0.5]), 0.3, 1.7),              # a range that does not start at 0
        (_line([0, 0, 0.2], [0, 0, 0.0]), 0.0, 1.0),                 # every sample nearer than the minimum distance
        (_line([0, 0, 0.1], [0, 0, 0.4]), 0.0, 2.5),                 # the first samples skipped, then looked at
        (_line([0, 0, 0.8], [0, 0, 0.3]), 0.0, 1.5),                 # straight ahead
        (_line([0, 0, 1.0], [0.5, 0, 0]), 0.0, 3.0),                 # drifts out of view to the right
        (_line([0, 0, 1.0], [0, -0.4, 0]), 0.0, 3.0),                # ... and upwards
    ]
    for bad in (np.nan, np.inf, -np.inf, 1e200):
        q = _line([0, 0, 1.0], [0, 0, 0.2])
        q[2, 1] = bad
        special.append((q, 0.0, 1.0))
    q = _line([0, 0, 1.0], [0, 0, 0.2])
    q[3, 2] = np.nan                                                  # z itself a NaN: not skipped, not out of view, never occluded
    special.append((q, 0.0, 1.0))
    c = np.concatenate([c, np.stack([s[0] for s in special])])
    tr = np.concatenate([tr, np.array([[s[1] for s in special], [s[2] for s in special]])], 1)
    return c, tr


def _wide_batch(w, h):
    """a small true radius (edge 0, ignore 0) and a 0.6 m planning sphere: its image crosses every border of the image,
    covers all of it, or (p.z <= r) has no bounding rectangle at all"""
    f, cx, cy = w / 2.0, w / 2.0, h / 2.0
    z = 1.5
    paths = []
    for ix, iy in [(1.0, cy), (w - 1.0, cy), (cx, 1.0), (cx, h - 1.0), (1.0, 1.0), (w - 1.0, h - 1.0), (w - 0.5, 0.75), (cx, cy)]:
        paths.append((_line([(ix - cx) / f * z, (iy - cy) / f * z, z], [0, 0, 0.05]), 0.0, 0.35))
    for zz in (0.55, 0.6, 0.6000000001, 0.61, 0.7):                   # p.z <= r, at r, and barely beyond it
        paths.append((_line([0.02, -0.01, zz], [0, 0, 0]), 0.0, 0.15))
    paths.append((_line([0.3, 0.1, 0.5], [0, 0, 0.3]), 0.0, 1.0))     # grows out of the sphere
    rng = np.random.default_rng(200 + w)
    c, tr = _random_paths(6, rng)
    c = np.concatenate([c, np.stack([p[0] for p in paths])])
    tr = np.concatenate([tr, np.array([[p[1] for p in paths], [p[2] for p in paths]])], 1)
    return c, tr


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: "%dx%d" % s)
def batch(request):
    """per image size: the two configurations, the images, the paths and the checker's records (computed once)"""
    w, h = request.param
    images = _images(w, h)
    out = {"w": w, "h": h, "images": images}
    for name, cfg, (c, tr) in (("plain", _cfg(w, h), _plain_batch(w, h)), ("wide", _cfg(w, h, 0.002, 0.6), _wide_batch(w, h))):
        rng = np.random.default_rng(len(c))
        idx = rng.integers(0, 3, len(c)).astype(np.int32)
        idx[:3] = [0, 1, 2]
        out[name] = dict(cfg=cfg, coeffs=c, t_range=tr, index=idx, want=tc.judge_batch(cfg, images, c, tr, idx))
    return out


def _same(records, want):
    bad = tc.records_equal(records, want)
    assert not bad, bad[:10]


@pytest.mark.parametrize("which", ["plain", "wide"])
def test_paths_equal_the_checker_in_every_field(batch, which):
    b = batch[which]
    verdicts = {r["verdict"] for r in b["want"]}
    if which == "plain":
        assert verdicts == {0, 1, 2}, verdicts
        assert {0, 1} <= {r["n_samples"] for r in b["want"]}
        assert any(r["n_checked"] == 0 and r["verdict"] == 0 and r["n_samples"] > 0 for r in b["want"])     # all skipped
    else:
        assert tc.scalars(b["cfg"]) == (0, 0) and {0, 2} <= verdicts
    # host images, image_index
    got, n_free, ms = afa.image_truth_paths(b["cfg"], batch["images"], b["coeffs"], b["t_range"], image_index=b["index"])
    _same(got, b["want"])
    assert n_free == sum(r["verdict"] == 0 for r in b["want"]) and ms > 0
    # the same images in HBM
    buf = afa.DeviceBuffer(batch["images"].nbytes)
    buf.upload(batch["images"])
    on_dev, n_free_dev, _ = afa.image_truth_paths(b["cfg"], buf, b["coeffs"], b["t_range"], image_index=b["index"])
    buf.close()
    assert on_dev.tobytes() == got.tobytes() and n_free_dev == n_free
    # without image_index: path i sees image i
    own = afa.image_truth_paths(b["cfg"], batch["images"], b["coeffs"][:3], b["t_range"][:, :3])[0]
    _same(own, [b["want"][i] for i in range(3)])                     # (index[:3] is 0, 1, 2)


def test_other_timesteps(batch):
    b = batch["plain"]
    n = 10
    for dt in (0.25, 0.03):
        want = tc.judge_batch(b["cfg"], batch["images"], b["coeffs"][:n], b["t_range"][:, :n], b["index"][:n], timestep=dt)
        got = afa.image_truth_paths(b["cfg"], batch["images"], b["coeffs"][:n], b["t_range"][:, :n], image_index=b["index"][:n], timestep=dt)[0]
        _same(got, want)


def test_stats_and_repeatability(batch):
    for which in ("plain", "wide"):
        b = batch[which]
        args = (b["cfg"], batch["images"], b["coeffs"], b["t_range"])
        st, ms = afa.image_truth_paths(*args, image_index=b["index"], want_stats=True)
        assert st["samples"] == sum(r["n_checked"] for r in b["want"])
        assert st["pixels_brute_force"] == batch["w"] * batch["h"] * st["samples"]
        assert st["pixels_meeting_sphere"] <= st["pixels_tested"] <= st["pixels_brute_force"]
        assert st["pixels_tested"] > 0
        first = afa.image_truth_paths(*args, image_index=b["index"])[0]
        again = afa.image_truth_paths(*args, image_index=b["index"])[0]
        assert first.tobytes() == again.tobytes()
    # the rectangle does its work where it can: the reference vehicle's sphere is a small part of the image
    st, _ = afa.image_truth_paths(batch["plain"]["cfg"], batch["images"], batch["plain"]["coeffs"][:8], batch["plain"]["t_range"][:, :8],
                                  image_index=np.ones(8, np.int32), want_stats=True)
    print("pixels tested / brute force:", st["pixels_tested"], st["pixels_brute_force"])


def test_plans_equal_the_paths_entry(batch):
    b = batch["plain"]
    n = len(b["coeffs"])
    plans = np.zeros(n, afa.PLAN_DTYPE)
    plans["coeffs"] = b["coeffs"]
    plans["tf"] = b["t_range"][1]
    plans["found"] = 1
    plans["found"][1::5] = 0
    tr = np.stack([np.zeros(n), b["t_range"][1]])
    want, _, _ = afa.image_truth_paths(b["cfg"], batch["images"], b["coeffs"], tr, image_index=b["index"])
    got, n_free, _ = afa.image_truth_plans(b["cfg"], batch["images"], plans, image_index=b["index"])
    found = plans["found"] != 0
    assert got[found].tobytes() == want[found].tobytes()
    _same(got[~found], [tc.EMPTY_RECORD] * int((~found).sum()))
    assert n_free == int((got["verdict"] == 0).sum())
    # a PlanOutput array as rappids_plan returns it
    arr = (afa.PlanOutput * n).from_buffer_copy(plans.tobytes())
    assert afa.image_truth_plans(b["cfg"], batch["images"], arr, image_index=b["index"])[0].tobytes() == got.tobytes()


# ---- candidates ---------------------------------------------------------------------------------------------------------
GRAV = [0.0, 9.81, 0.0]


def test_candidates_verdicts_coefficients_and_tally():
    w, h, n, m = 200, 150, 5, 32
    cfg = _cfg(w, h)
    images = np.stack([afa.scenarios.synthetic_depth_image(width=w, height=h, seed=40 + k, n_trunks=4 + k) for k in range(3)])
    rng = np.random.default_rng(9)
    index = np.array([0, 1, 2, 1, 0], np.int32)
    vel0 = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.2, 0.2, n), rng.uniform(0.2, 1.5, n)])
    acc0 = rng.normal(0, 0.3, (3, n))
    grav = np.tile(np.array(GRAV)[:, None], (1, n))
    samples = np.stack([afa.planner_samples(s, w, h, m) for s in range(2)])
    table = np.array([0, 1, 0, 1, 1], np.int32)
    plans, flags, _ = afa.rappids_plan(cfg, images, vel0, acc0, grav, samples, image_index=index, sample_table=table, want_flags=True)
    verdict, coeffs, tally, per, ms = afa.image_truth_candidates(cfg, images, vel0, acc0, samples, flags, image_index=index, sample_table=table,
                                                                want_coeffs=True, want_per_planner=True)
    assert ms > 0
    # the winner's row of coeffs_out IS the plan's polynomial
    plans = afa.plans_as_array(plans)
    assert plans["found"].sum() >= 1
    for i in range(n):
        if plans["found"][i]:
            assert coeffs[i, plans["best_index"][i]].tobytes() == plans["coeffs"][i].tobytes()
            assert plans["tf"][i] == samples[table[i], plans["best_index"][i], 3]
    # the verdicts are the checker's on what was judged
    rays = [tc.ImageRays(cfg, img) for img in images]
    want = np.array([[tc.judge(rays[index[i]], coeffs[i, c], 0.0, samples[table[i], c, 3])["verdict"] for c in range(m)] for i in range(n)])
    assert_array_equal(verdict, want)
    assert len(set(want.reshape(-1))) >= 2
    # the tallies are numpy's from the flags and the verdicts
    assert {k: int(tally[k]) for k in tally.dtype.names} == tc.tally(flags, verdict)
    for i in range(n):
        assert {k: int(per[k][i]) for k in per.dtype.names} == tc.tally(flags[i], verdict[i])
    assert tally["n_checked"] > 0
    # without the optional outputs
    v2, c2, t2, p2, _ = afa.image_truth_candidates(cfg, images, vel0, acc0, samples, flags, image_index=index, sample_table=table)
    assert c2 is None and p2 is None and v2.tobytes() == verdict.tobytes() and t2 == tally


def test_what_the_planner_calls_free_is_free():
    """the reference's MeasureConservativeness on 4 images x 120 candidates, one candidate per planner (no cost pruning)"""
    cfg = _cfg(320, 240)
    images = np.stack([afa.scenarios.synthetic_depth_image(seed=100 + s, n_trunks=8) for s in range(4)])
    samples = np.concatenate([afa.planner_samples(s, 320, 240, 240)[0:240:2] for s in range(4)])[:, None, :]      # [480 tables][1][4]
    n = len(samples)
    index = np.repeat(np.arange(4, dtype=np.int32), 120)
    table = np.arange(n, dtype=np.int32)
    vel0 = np.tile(np.array([0.2, -0.1, 0.8])[:, None], (1, n))
    acc0 = np.zeros((3, n))
    grav = np.tile(np.array(GRAV)[:, None], (1, n))
    _, flags, _ = afa.rappids_plan(cfg, images, vel0, acc0, grav, samples, image_index=index, sample_table=table, want_flags=True)
    verdict, _, tally, _, _ = afa.image_truth_candidates(cfg, images, vel0, acc0, samples, flags, image_index=index, sample_table=table)
    free = flags[:, 0] == 15
    print("planner-free %d of %d, tally %s" % (free.sum(), n, tally))
    assert free.sum() >= 100
    assert np.all(verdict[free, 0] == 0), np.flatnonzero(free & (verdict[:, 0] != 0))
    assert tally["n_free_but_out_of_view"] == 0 and tally["n_free_but_occluded"] == 0
    assert tally["n_planner_free"] == free.sum()
    assert min(np.mean(verdict == v) for v in (0, 1, 2)) >= 0.05


# ---- refusals -----------------------------------------------------------------------------------------------------------
def _copy(cfg, **changes):
    c = afa.PlannerConfig()
    C.memmove(C.byref(c), C.byref(cfg), C.sizeof(cfg))
    for k, v in changes.items():
        setattr(c, k, v)
    return c


def test_refusals_leave_the_outputs_untouched():
    L = afa.library()
    w, h, n = 72, 40, 4
    cfg = _cfg(w, h)
    images = _images(w, h)
    coeffs = np.ascontiguousarray(np.stack([_line([0, 0, 1.0], [0, 0, 0.2])] * n))
    tr = np.ascontiguousarray(np.stack([np.zeros(n), np.ones(n)]))
    idx = np.array([0, 1, 2, 0], np.int32)
    sentinel = np.full(n, 0x5A, np.uint8).repeat(afa.IMAGE_TRUTH_DTYPE.itemsize)

    def paths(cfg_=cfg, images_=images.ctypes.data, n_images=3, on_device=0, index=idx, coeffs_=coeffs.ctypes.data, tr_=tr, dt=0.1, with_out=True):
        out = sentinel.copy()
        n_free, ms = C.c_int64(-5), C.c_float(-5)
        rc = L.afe_image_truth_paths(-1, None if cfg_ is None else C.byref(cfg_), n, images_, n_images, on_device,
                                     None if index is None else index.ctypes.data, coeffs_, None if tr_ is None else tr_.ctypes.data, dt,
                                     out.ctypes.data if with_out else None, C.byref(n_free), C.byref(ms))
        assert np.all(out == 0x5A) and n_free.value == -5 and ms.value == -5, "a refused call wrote something"
        return rc

    INVALID, RANGE = 1, 4
    assert paths(cfg_=None) == INVALID and paths(images_=None) == INVALID and paths(coeffs_=None) == INVALID
    assert paths(tr_=None) == INVALID and paths(with_out=False) == INVALID and paths(n_images=0) == INVALID
    assert paths(index=None, n_images=3) == INVALID                               # four paths, three images, no index
    for dt in (0.0, -0.1, float("nan"), float("inf")):
        assert paths(dt=dt) == INVALID
    assert paths(cfg_=_copy(cfg, width=0)) == INVALID
    long_range = np.ascontiguousarray(np.stack([np.zeros(n), np.array([1.0, 1.0, 500.0, 1.0])]))
    assert paths(tr_=long_range) == RANGE                                          # K > 4096
    assert paths(index=np.array([0, 1, 3, 0], np.int32)) == RANGE and paths(index=np.array([0, -1, 2, 0], np.int32)) == RANGE
    assert paths(cfg_=_copy(cfg, min_checking_dist=0.0)) == RANGE and paths(cfg_=_copy(cfg, min_checking_dist=-1.0)) == RANGE
    assert paths(cfg_=_copy(cfg, depth_scale=0.116 / 65537.0)) == RANGE            # the ignore quotient passes 65 536
    assert paths(cfg_=_copy(cfg, depth_scale=0.0)) == RANGE
    assert paths(cfg_=_copy(cfg, width=8192, height=4096)) == RANGE                # an image the call cannot take
    buf = afa.DeviceBuffer(images.nbytes + 16)
    assert paths(images_=C.c_void_p(buf.ptr.value + 2), on_device=1) == INVALID    # not 16-byte aligned
    buf.close()

    # plans
    plans = np.zeros(n, afa.PLAN_DTYPE)
    plans["found"], plans["tf"] = 1, [1.0, 500.0, 1.0, 1.0]
    out = sentinel.copy()
    n_free = C.c_int64(-5)
    for rc_want, p_ptr, dt in ((RANGE, plans.ctypes.data, 0.1), (INVALID, None, 0.1), (INVALID, plans.ctypes.data, 0.0)):
        assert L.afe_image_truth_plans(-1, C.byref(cfg), n, images.ctypes.data, 3, 0, idx.ctypes.data, p_ptr, dt, out.ctypes.data,
                                       C.byref(n_free), None) == rc_want
    assert np.all(out == 0x5A) and n_free.value == -5
    plans["found"][1] = 0                                                          # a plan that was not found is not sampled
    assert afa.image_truth_plans(cfg, images, plans, image_index=idx)[0]["verdict"][1] == -1

    # candidates
    m = 4
    vel0, acc0 = np.tile(np.array([0.0, 0.0, 0.8])[:, None], (1, n)), np.zeros((3, n))
    samples = afa.planner_samples(0, w, h, m)
    flags = np.full((n, m), 7, np.uint8)
    verdict = np.full((n, m), 0x5A, np.uint8)
    tally = np.full(6, -5, np.int64)

    def cands(samples_=samples, flags_=flags.ctypes.data, dt=0.1, index=idx, verdict_ptr=verdict.ctypes.data):
        return L.afe_image_truth_candidates(-1, C.byref(cfg), n, images.ctypes.data, 3, 0, index.ctypes.data, vel0.ctypes.data, acc0.ctypes.data,
                                            samples_.ctypes.data, 1, None, m, flags_, dt, verdict_ptr, None, tally.ctypes.data, None, None)

    slow = samples.copy()
    slow[2, 3] = 500.0
    assert cands(samples_=slow) == RANGE and cands(flags_=None) == INVALID and cands(dt=-1.0) == INVALID and cands(verdict_ptr=None) == INVALID
    assert cands(index=np.array([0, 1, 2, 7], np.int32)) == RANGE
    assert np.all(verdict == 0x5A) and np.all(tally == -5)
    assert cands() == 0 and np.all(verdict <= 2) and tally[0] == n * m
