"""A live handle whose device scratch is replaced under it: every case asks one handle for little, then for more than its
headroom holds (the scratch goes back and a larger one comes), then for little again, and every answer is judged by the
checker of its area -- the brute-force definition for the neighbour query, tests/path_checker.py for the plan audit,
tests/stats_checker.py for the statistics, the oracle for the planner.  (What a REFUSED growth does to a buffer is
tested on the CPU, tests/test_devmem.py.)  Needs an MI355X."""
import numpy as np
import pytest
from numpy.testing import assert_array_equal

from tests import path_checker as pc
from tests import stats_checker as ck
from tests.scenarios import afa, random_ensemble
from tests.test_gpu_path_clearance import RADIUS, _engine_with_plans
from tests.test_gpu_planner import _cfg, _compare
from tests.test_gpu_sharedworld import _nn
from tests.test_gpu_stats import same_records

pytestmark = pytest.mark.gpu


def test_world_scratch_is_replaced_under_a_live_engine(ora):
    import torch
    n, n_big = 256, 2048                                   # per-point headroom after the first query: 256 + 32 + 1024 < 2048
    rng = np.random.default_rng(41)
    big = rng.uniform(-10.5, 10.5, (3, n_big)).astype(np.float32)
    small = np.ascontiguousarray(big[:, :n])
    with afa.Ensemble(n) as e:
        e.set_type_table([afa.params_from_type(5)])
        e.set_state(pos=small.astype(np.float64))
        for k, pos in enumerate((small, big, small)):
            world = torch.from_numpy(np.ascontiguousarray(pos)).cuda()
            d2, idx = _nn(e, world, pos.shape[1])
            ref_d, ref_i = ora.nearest_neighbour(pos, 0, n)
            assert_array_equal(idx, ref_i, err_msg="query %d" % k)
            assert_array_equal(d2, ref_d, err_msg="query %d" % k)
        # the same points, cells of 2 m, of 0.5 m (past the per-cell headroom of 4 096) and of 2 m again
        ref_d, ref_i = ora.nearest_neighbour(small, 0, n)
        cells = []
        for cell_size in (2.0, 0.5, 2.0):
            d2, idx = _nn(e, world, n, cell_size)
            cells.append(e.neighbour_grid_info()["n_cells"])
            assert_array_equal(idx, ref_i, err_msg="cells of %g m" % cell_size)
            assert_array_equal(d2, ref_d, err_msg="cells of %g m" % cell_size)
        assert 500 <= cells[0] <= 2000 and cells[1] > 60000 and cells[2] == cells[0], cells


def test_clearance_map_scratch_is_replaced_between_audits():
    tris = afa.scenarios.orchard_mesh(rows=2, cols=3, seed=3)
    cmap = afa.ClearanceMap(tris)                          # its own map: the plan scratch starts empty
    e, mount, plans = _engine_with_plans(tris, afa.AFE_F32)
    n, K = e.n, 65
    assert n == 64
    found = plans["found"] != 0
    st = e.get_state()
    origin, rot = np.empty((3, n)), np.empty((9, n))
    for i in range(n):
        origin[:, i], rot[:, i] = pc.camera_pose(st["pos"][:, i], st["att"][:, i], mount)
    want, _ = pc.audit(tris, plans["coeffs"], np.stack([np.zeros(n), plans["tf"]]), origin, rot, K, RADIUS, sampled=found)
    for first, count in ((0, 8), (0, 64), (40, 8)):
        assert found[first:first + count].any()
        got, n_col, _ = cmap.plans_engine(e, plans[first:first + count], mount, first=first, count=count, n_samples=K, radius=RADIUS)
        pc.assert_records_equal(got, want[first:first + count])
        assert n_col == int((want["n_hit"][first:first + count] > 0).sum())
    e.close()
    cmap.close()


def test_stats_result_is_replaced_when_a_histogram_comes():
    n = 3000
    edges = [10, 1000, 1000, 2990]
    ens = random_ensemble(n, seed=6, type_ids=(5,))
    ref = ens.data.pos + np.random.default_rng(8).normal(0, 3.0, (3, n))
    hist_edges = 0.5 + 0.6 * np.arange(16)
    with ens.to_engine(afa.AFE_F32) as e:
        mon = afa.StatsMonitor(e, edges)
        mon.set_reference(ref)
        lat = ck.Latches(n)
        st, now = e.get_state(), e.time_us
        for asked in (None, hist_edges, None):
            mon.set_histogram(asked)
            rec, hist = mon.update()
            want, want_hist = ck.update(st, ref, lat, edges, now, asked)
            same_records(rec, want)
            if asked is None:
                assert hist is None
            else:
                assert hist.shape == (3, 17) and hist.sum() > 0
                assert_array_equal(hist, want_hist)
        mon.close()


def _plan_case(ora, w, h, n, m, seed):
    rng = np.random.default_rng(seed)
    images = np.stack([afa.scenarios.synthetic_depth_image(width=w, height=h, seed=seed + k, n_trunks=2 + k) for k in range(3)])
    ocfg = ora.planner_config(w, h, 10.0 / 256.0, w / 2.0, 0.116, 0.174, 0.5)
    ocfg.max_pyramids = 64
    ocfg.cost_type = 1
    ocfg.cost_vec[2] = 120.0
    image_index = rng.integers(0, 3, n).astype(np.int32)
    vel0 = np.stack([rng.normal(0, 0.4, n), rng.normal(0, 0.2, n), rng.uniform(0, 2.0, n)])
    acc0 = rng.normal(0, 0.3, (3, n))
    grav = np.tile(np.array([[0.0], [9.81], [0.0]]), (1, n))
    samples = ora.planner_samples(3, w, h, m)
    refs = [ora.planner_run(ocfg, images[image_index[i]], vel0[:, i], acc0[:, i], grav[:, i], samples) for i in range(n)]
    assert 0 < sum(r[0].found for r in refs) and sum(r[0].n_pyramids for r in refs) > 0
    return (_cfg(ocfg), images, vel0, acc0, grav, samples), image_index, refs


def test_planner_scratch_grows_from_nothing_and_is_kept(ora):
    little = _plan_case(ora, 72, 40, 8, 64, seed=700)
    much = _plan_case(ora, 200, 150, 24, 256, seed=710)
    afa.planner_release_scratch()
    answers = []
    for args, image_index, refs in (little, much, little):
        out, flags, _ = afa.rappids_plan(*args, image_index=image_index, want_flags=True)
        _compare(out, flags, refs)
        answers.append((afa.plans_as_array(out).copy(), flags.copy()))
    assert_array_equal(answers[0][0].view(np.uint8), answers[2][0].view(np.uint8))     # bit for bit
    assert_array_equal(answers[0][1], answers[2][1])
