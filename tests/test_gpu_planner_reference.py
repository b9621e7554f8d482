"""The batched planner (afe_planner.hip) and the image ground truth (afe_truth.hip) against what the REFERENCE's own code
decided: tests/golden/planner_reference.npz, recorded by oracle/_ref/planner_probe from DepthImagePlanner.cpp compiled in
place (tests/golden/make_planner_reference.py; tests/test_planner_reference.py holds the CPU checkers to the same file bit
for bit).  224 plans: clutter, orchard views, image sizes off the fast path, hanging rectangles, a ceiling, a wall, pyramid limits 1 and 2, states that fail
the thrust, rate and velocity tests.  Reads the fixture and the committed image generators only.  Needs an MI355X."""
import importlib.util
import os

import numpy as np
import pytest

from tests.scenarios import MEASUREMENTS, afa

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *parts))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ref(ora):
    """the generator module, the fixture, every scene's image (each held to its recorded SHA-256) and, per image size, the
    scenes of that size: {(w, h): [scene numbers]}"""
    mod = _load("make_planner_reference", "tests", "golden", "make_planner_reference.py")
    fx = mod.load_fixture()
    images = mod.checked_images(fx)
    sizes = {}
    for s, wh in enumerate(fx["scene_size"]):
        sizes.setdefault((int(wh[0]), int(wh[1])), []).append(s)
    return mod, fx, images, sizes


def _device_cfg(fx, w, h, limit, cost_type=0):
    c = afa.planner_default_config(w, h, float(fx["depth_scale"]), w / 2.0, float(fx["true_radius"]), float(fx["planning_radius"]),
                                   float(fx["min_checking_dist"]))
    c.max_pyramids = int(limit)
    c.cost_type = int(cost_type)
    return c


def _tables(ora, fx, w, h):
    return np.stack([ora.planner_samples(seed, w, h, int(fx["n_candidates"])) for seed in range(4)])


@pytest.mark.parametrize("path", ["recorded limit", "in lanes"])
def test_device_plans_what_the_reference_planned(ora, ref, path):
    """afa.rappids_plan on the fixture's plans, one call per image size, pyramid limit and cost type (both live in the
    configuration).  Every candidate's flags, found, the winner and the five counters must equal THE REFERENCE'S recorded
    values; the winner's coefficients to rtol 1e-12.

    "recorded limit" runs every plan at the limit the reference had: 100 for the ordinary scenes, which puts the device's
    pyramid list in memory, and 1 and 2.  "in lanes" runs the ordinary scenes at 64, where the wave keeps the list in its
    lanes; no such plan holds more than 29 pyramids, so no limit binds and the answers are the recorded ones.

    A plan that differs is accepted only under the rule of test_wide_campaign_every_mismatch_is_an_ulp_of_libm: the
    checker -- which tests/test_planner_reference.py shows equal to the reference on that very plan -- must land on the
    device's answer when ONE of its acos / cos / pow results is moved by at most 2 ulps.  Unexplained differences: 0.
    Explained ones: at most 1 % of the plans (the project measures at most 0.2 % over 8 000 plans, i.e. fewer than one
    expected here).  Plans that differ in the pyramid count alone: at most 3 %, the project's existing cap."""
    mod, fx, images, sizes = ref
    campaign = _load("planner_campaign", "tests", "campaigns", "planner_campaign.py")
    n_plans = explained = unexplained = pyramid_only = 0
    for (w, h), scene_list in sizes.items():
        tables = _tables(ora, fx, w, h)
        stack = np.stack([images[s] for s in scene_list])
        of_size = np.isin(fx["plan_scene"], scene_list)
        limits = sorted(set(fx["max_pyramids"][of_size].tolist()))
        for limit in limits:
            if path == "in lanes" and limit != mod.FREE_LIMIT:
                continue
            for cost_type in (0, 1):
                plans = np.flatnonzero(of_size & (fx["max_pyramids"] == limit) & (fx["cost_type"] == cost_type))
                if not len(plans):
                    continue
                device_limit = 64 if path == "in lanes" else limit
                idx = np.array([scene_list.index(s) for s in fx["plan_scene"][plans]], np.int32)
                out, flags, _ = afa.rappids_plan(_device_cfg(fx, w, h, device_limit, cost_type), stack, fx["vel0"][plans].T, fx["acc0"][plans].T,
                                                 fx["grav"][plans].T, tables, image_index=idx, cost_vec=fx["cost_vec"][plans].T,
                                                 sample_table=fx["seed"][plans].astype(np.int32), want_flags=True)
                for i, p in enumerate(plans):
                    o = out[i]

                    def hard(found, best, fl, counters):
                        return (o.found, o.best_index) == (found, best) and np.array_equal(flags[i], fl) and \
                            [o.n_generated, o.n_cost_checks, o.n_collision_checks, o.n_velocity_checks, o.n_collision_free] == list(counters)
                    n_plans += 1
                    if hard(fx["found"][p], fx["last_free"][p], fx["flags"][p], fx["counters"][p, :5]):
                        pyramid_only += int(o.n_pyramids != fx["counters"][p, 5])
                        if o.found:
                            got = np.array([[o.coeffs[q][a] for a in range(3)] for q in range(6)])
                            assert o.tf == fx["tf"][p], p
                            np.testing.assert_allclose(got, fx["coeffs"][p], rtol=1e-12, atol=1e-14, err_msg="plan %d" % p)
                        continue
                    ocfg = mod.oracle_config(ora, fx, int(fx["plan_scene"][p]), p)
                    ocfg.max_pyramids = device_limit
                    args = (ocfg, images[fx["plan_scene"][p]], fx["vel0"][p], fx["acc0"][p], fx["grav"][p], tables[fx["seed"][p]])
                    why, calls = campaign.explained_by_nudge(args, lambda res, rfl: hard(res.found, res.best_index, rfl, [
                        res.n_generated, res.n_cost_checks, res.n_collision_checks, res.n_velocity_checks, res.n_collision_free]))
                    print("plan %d (%s): differs from the reference; %d transcendental calls, reproduced by nudging call %s by %s ulp"
                          % (p, fx["scene_name"][fx["plan_scene"][p]], calls, *(why if why else ("NONE", "-"))))
                    explained += why is not None
                    unexplained += why is None
    print("planner against the reference, %s: %d plans, %d explained by one libm ulp, %d unexplained, %d differ in the pyramid count alone"
          % (path, n_plans, explained, unexplained, pyramid_only))
    MEASUREMENTS["planner_reference " + path] = dict(plans=int(n_plans), explained=int(explained), unexplained=int(unexplained), pyramid_count_only=int(pyramid_only))
    assert n_plans == (len(fx["found"]) if path == "recorded limit" else int((fx["max_pyramids"] == mod.FREE_LIMIT).sum()))
    assert unexplained == 0
    assert explained <= 0.01 * n_plans
    assert pyramid_only <= 0.03 * n_plans


def _paths_of_size(ora, mod, fx, scene_list, w, h):
    """every recorded ground-truth path on the scenes of one size: coefficients [n, 6, 3], t_range [2, n], the image of each
    (an index into scene_list), the reference's booleans"""
    tables = _tables(ora, fx, w, h)
    cfg = mod.oracle_config(ora, fx, scene_list[0])
    co, tf, idx, free = [], [], [], []
    for p in np.flatnonzero(np.isin(fx["plan_scene"], scene_list)):
        for j in range(fx["truth_offset"][p], fx["truth_offset"][p + 1]):
            sample = tables[fx["seed"][p], fx["truth_index"][j]]
            co.append(mod.candidate_coeffs(ora, cfg, fx["vel0"][p], fx["acc0"][p], sample))
            tf.append(sample[3])
            idx.append(scene_list.index(fx["plan_scene"][p]))
            free.append(bool(fx["truth_free"][j]))
    return np.stack(co), np.stack([np.zeros(len(tf)), np.array(tf)]), np.array(idx, np.int32), np.array(free)


def test_image_truth_calls_free_what_the_reference_calls_free(ora, ref):
    """afa.image_truth_paths on EVERY recorded ground-truth path (about 1 500; the polynomials from the parts of the checker
    that are pinned bit for bit), images on the host and in HBM: verdict 0 exactly where the reference's
    IsCollisionFreeGroundTruth returned true.  No exception: the arithmetic is + - * / sqrt.  (Which refused path left the
    view and which was occluded is this project's split; the reference returns a bool.)"""
    mod, fx, images, sizes = ref
    total = n_free = 0
    for (w, h), scene_list in sizes.items():
        co, tr, idx, free = _paths_of_size(ora, mod, fx, scene_list, w, h)
        cfg = _device_cfg(fx, w, h, mod.FREE_LIMIT)
        stack = np.stack([images[s] for s in scene_list])
        got, count, _ = afa.image_truth_paths(cfg, stack, co, tr, image_index=idx)
        wrong = np.flatnonzero((got["verdict"] == 0) != free)
        assert not len(wrong), ((w, h), wrong[:10], got["verdict"][wrong[:10]])
        assert count == int(free.sum())
        buf = afa.DeviceBuffer(stack.nbytes)
        buf.upload(stack)
        on_dev, count_dev, _ = afa.image_truth_paths(cfg, buf, co, tr, image_index=idx)
        buf.close()
        assert on_dev.tobytes() == got.tobytes() and count_dev == count
        total += len(free)
        n_free += count
    print("image ground truth against the reference: %d paths, %d free, all as recorded" % (total, n_free))
    assert total == len(fx["truth_free"]) and n_free == int(fx["truth_free"].sum())


def test_conservativeness_tally_is_the_reference_comparison(ora, ref):
    """afa.image_truth_candidates on the plans whose collision-checked candidates were all recorded, fed the REFERENCE's
    flags: each plan's tally equals the one the generator formed from the reference's flags and the reference's booleans
    (n_free_but_out_of_view + n_free_but_occluded against the reference's single count of refused free paths)."""
    mod, fx, images, sizes = ref
    total = np.zeros(5, np.int64)
    for (w, h), scene_list in sizes.items():
        plans = np.flatnonzero(np.isin(fx["plan_scene"], scene_list) & fx["truth_full"])
        if not len(plans):
            continue
        stack = np.stack([images[s] for s in scene_list])
        idx = np.array([scene_list.index(s) for s in fx["plan_scene"][plans]], np.int32)
        _, _, tally, per, _ = afa.image_truth_candidates(_device_cfg(fx, w, h, mod.FREE_LIMIT), stack, fx["vel0"][plans].T, fx["acc0"][plans].T,
                                                         _tables(ora, fx, w, h), fx["flags"][plans], image_index=idx,
                                                         sample_table=fx["seed"][plans].astype(np.int32), want_per_planner=True)
        got = np.stack([per["n_checked"], per["n_planner_free"], per["n_correct_in_collision"], per["n_incorrect_in_collision"],
                        per["n_free_but_out_of_view"] + per["n_free_but_occluded"]], 1)
        np.testing.assert_array_equal(got, fx["tally"][plans], err_msg="%dx%d" % (w, h))
        assert [int(tally[k]) for k in ("n_checked", "n_planner_free", "n_correct_in_collision", "n_incorrect_in_collision")] == \
            list(fx["tally"][plans, :4].sum(0))
        total += got.sum(0)
    print("conservativeness on %d fully recorded plans: checked %d, planner-free %d, correctly refused %d, needlessly refused %d, "
          "free but refused by the ground truth %d" % (int(fx["truth_full"].sum()), *total))
    MEASUREMENTS["planner_reference tally"] = dict(zip(("n_checked", "n_planner_free", "n_correct_in_collision", "n_incorrect_in_collision",
                                                        "n_free_but_not_free"), (int(v) for v in total)))
    assert np.array_equal(total, fx["tally"][fx["truth_full"]].sum(0)) and total[0] > 100
