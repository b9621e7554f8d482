"""The batched RAPPIDS planner where its other tests never take it, and under a judge that is not the oracle.

tests/test_gpu_planner.py compares kernel and oracle on tame states: no candidate there is ever rejected for thrust, body
rate or speed, so input_section's SEC_HIGH / SEC_LOW / SEC_INDETERMINABLE returns, input_feasible's stack, the peak terms
and every `return false` of velocity_feasible have no consequence in it.  Here the aggressive distribution of
tests/plan_checker.py makes each of the flag values 1 / 3 / 7 / 15 at least 5 % of the candidates (asserted on the oracle's
flags), candidates are planned alone so that cost pruning hides none of the four tests, and every flag the device returns --
equal to the oracle's or not -- is held against plan_checker's conditions: dense thrust and body rate inside the limits,
exact per-axis speed extrema, distance to the occupied volume of the depth image, closed-form coefficients and cost, and a
replay of the sequential search.  Needs an MI355X.

Against the oracle: LowCost, DynamicsFeasible and VelocityAdmissible of every candidate are equal, no allowance.
CollisionFree (and, in whole plans, what follows from it) may differ only where the oracle itself lands on the device's
answer with one acos / cos / pow result moved by an ulp or two (tests/campaigns/planner_campaign.py), for at most 0.2 %."""
import importlib.util
import os
import time

import numpy as np
import pytest

from tests import plan_checker as pc
from tests.scenarios import MEASUREMENTS, afa

pytestmark = pytest.mark.gpu

SCALE, RADIUS, PLANNING_RADIUS, MIN_DIST = 10.0 / 256.0, 0.116, 0.174, 0.5
TIGHT_LIMITS = dict(min_thrust=8.0, max_thrust=20.0, max_ang_vel=5.0, max_velocity=3.0)
M = 200


def _campaign():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "campaigns", "planner_campaign.py")
    spec = importlib.util.spec_from_file_location("planner_campaign", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _configs(ora, w, h, focal, **kw):
    """the same configuration for the oracle and for the engine"""
    ocfg = ora.planner_config(w, h, SCALE, focal, RADIUS, PLANNING_RADIUS, MIN_DIST)
    cfg = afa.planner_default_config(w, h, SCALE, focal, RADIUS, PLANNING_RADIUS, MIN_DIST)
    for c in (ocfg, cfg):
        c.max_pyramids = 64
        for key, value in kw.items():
            setattr(c, key, value)
    return ocfg, cfg


@pytest.fixture(scope="module")
def images():
    """6 synthetic depth images and 6 views rendered from inside the orchard, 320 x 240"""
    rng = np.random.default_rng(77)
    scene = afa.Scene(afa.scenarios.orchard_mesh(rows=8, cols=10, seed=11))
    pos = np.stack([rng.uniform(-5, 25, 6), rng.uniform(-2, 30, 6), rng.uniform(0.6, 2.5, 6)])
    att = afa.scenarios.random_attitudes(rng, 6, max_tilt_deg=20.0)
    rendered, _ = scene.render(afa.camera_default(320, 240), pos, att, afa.camera_default_mount())
    scene.close()
    synthetic = np.stack([afa.scenarios.synthetic_depth_image(seed=200 + k, n_trunks=4 + k) for k in range(6)])
    return np.concatenate([synthetic, np.asarray(rendered).reshape(6, 240, 320)])


def _record(name, **values):
    MEASUREMENTS.setdefault("planner_judged", {})[name] = values
    print(name, values)


def _shares(flags, what):
    shares = pc.flag_shares(flags)
    assert min(shares.values()) >= 0.05, (what, shares)
    return {str(v): round(100 * s, 1) for v, s in shares.items()}


def _singles(ora, ocfg, cfg, imgs, image_of, vel0, acc0, grav, samples, judged=None, max_winners=300):
    """every (state, sample) pair as a one-candidate planner: on the device in one call, by the oracle one by one.  Asserts
    the comparison and the judge's conditions; returns (oracle flags, device flags [states, samples], judged, measurements)."""
    n_states, m = vel0.shape[1], len(samples)
    state_of = np.repeat(np.arange(n_states), m)
    out, flags, ms = afa.rappids_plan(cfg, imgs, vel0[:, state_of], acc0[:, state_of], grav[:, state_of], samples[:, None, :],
                                      image_index=image_of[state_of].astype(np.int32), sample_table=np.tile(np.arange(m), n_states).astype(np.int32),
                                      want_flags=True)
    assert flags.shape == (n_states * m, 1)
    dev = flags[:, 0]
    ref = np.empty_like(dev)
    for p in range(n_states * m):
        i, k = divmod(p, m)
        ref[p] = ora.planner_run(ocfg, imgs[image_of[i]], vel0[:, i], acc0[:, i], grav[:, i], samples[k:k + 1])[1][0]
    assert np.all(np.isin(ref, (1, 3, 7, 15)))
    # LowCost, DynamicsFeasible, VelocityAdmissible: a one-ulp root moves none of them (only within 1e-15 of a limit)
    assert np.array_equal(dev & 7, ref & 7), np.flatnonzero((dev & 7) != (ref & 7))[:10]
    differ = np.flatnonzero(dev != ref)
    assert len(differ) <= 0.002 * len(dev), differ
    campaign = _campaign() if len(differ) else None
    for p in differ:
        i, k = divmod(p, m)
        explained, _ = campaign.explained_by_nudge((ocfg, imgs[image_of[i]], vel0[:, i], acc0[:, i], grav[:, i], samples[k:k + 1]),
                                                   lambda res, rflags: rflags[0] == dev[p] and res.found == out[p].found)
        assert explained is not None, "candidate %d of state %d: device %d, oracle %d, and no ulp of libm explains it" % (k, i, dev[p], ref[p])
    if judged is None:
        judged = pc.Judged(cfg, vel0[:, state_of].T, acc0[:, state_of].T, grav[:, state_of].T, np.tile(samples, (n_states, 1)))
    bad_ref, _ = pc.violations(cfg, judged, ref)
    bad, seen = pc.violations(cfg, judged, dev)
    assert bad_ref == [] and bad == []
    found = np.flatnonzero(dev == 15)
    assert np.array_equal(found, np.flatnonzero([o.found for o in out])) and all(out[p].best_index == 0 for p in found)
    picked = found[::max(1, -(-len(found) // max_winners))]
    cost = pc.costs(cfg, judged.pf, judged.T)
    seen["clearance_min"], seen["winners_checked"] = pc.CLEARANCE_CAP, len(picked)
    for p in picked:
        b, clear = pc.winner_violations(cfg, imgs[image_of[p // m]], judged, p, afa.plans_as_array(out)["coeffs"][p], out[p].best_cost, cost[p])
        bad += b
        seen["clearance_min"] = min(seen["clearance_min"], clear)
    assert bad == []
    seen.update(differ_in_collision_bit=int(len(differ)), kernel_ms=round(ms, 2))
    return ref.reshape(n_states, m), dev.reshape(n_states, m), judged, seen


def test_single_candidates_under_the_aggressive_distribution(ora, images):
    t0 = time.perf_counter()
    ocfg, cfg = _configs(ora, 320, 240, 160.0)
    vel0, acc0, grav = pc.aggressive_states(45, 36, upright_every=2)
    samples = pc.aggressive_samples(ora.planner_samples(0, 320, 240, M), 0)
    image_of = np.arange(36) // 3
    ref, dev, _, seen = _singles(ora, ocfg, cfg, images, image_of, vel0, acc0, grav, samples)
    _record("single_candidates", oracle_shares=_shares(ref, "single candidates"), seconds=round(time.perf_counter() - t0, 2), **seen)
    assert seen["dynamics_rejected"] > 0 and seen["rejected_speed_min"] is not None


def test_whole_plans_under_the_aggressive_distribution(ora, images):
    """96 searches over 200-candidate tables, tilted gravity, both cost types, a cost vector per vehicle"""
    t0 = time.perf_counter()
    n = 96
    rng = np.random.default_rng(46)
    vel0, acc0, grav = pc.aggressive_states(46, n)
    tables = np.stack([pc.aggressive_samples(ora.planner_samples(s, 320, 240, M), s) for s in range(4)])
    table = rng.integers(0, 4, n).astype(np.int32)
    image_of = rng.integers(0, len(images), n).astype(np.int32)
    cost_vec = rng.normal(0, 1, (3, n))
    cost_vec[2] = np.abs(cost_vec[2]) + 1.0
    campaign = None
    hard, found, clearance_min, seen_all, examined = 0, 0, pc.CLEARANCE_CAP, {}, []
    for cost_type in (0, 1):
        who = np.flatnonzero(np.arange(n) % 2 == cost_type)
        vec = cost_vec[:, who] * (1.0 if cost_type == 0 else 40.0)        # a direction / a goal some 40 m away
        ocfg, cfg = _configs(ora, 320, 240, 160.0, cost_type=cost_type)
        out, flags, _ = afa.rappids_plan(cfg, images, vel0[:, who], acc0[:, who], grav[:, who], tables, image_index=image_of[who],
                                         cost_vec=vec, sample_table=table[who], want_flags=True)
        coeffs = afa.plans_as_array(out)["coeffs"]
        for j, i in enumerate(who):
            for a in range(3):
                ocfg.cost_vec[a] = vec[a, j]
            args = (ocfg, images[image_of[i]], vel0[:, i], acc0[:, i], grav[:, i], tables[table[i]])
            o = out[j]

            def same(res, rflags, o=o, j=j):
                return (o.found, o.best_index) == (res.found, res.best_index) and np.array_equal(flags[j], rflags) and \
                    (o.n_cost_checks, o.n_collision_checks, o.n_velocity_checks, o.n_collision_free) == \
                    (res.n_cost_checks, res.n_collision_checks, res.n_velocity_checks, res.n_collision_free)
            res, rflags = ora.planner_run(*args)
            for f in (rflags, flags[j]):                                   # (a candidate neither examined has no bit to compare)
                assert np.array_equal(f & 1, (f != 0).astype(np.uint8))
            both = (rflags != 0) & (flags[j] != 0)
            assert np.array_equal(flags[j][both] & 7, rflags[both] & 7), i
            if not same(res, rflags):
                hard += 1
                campaign = campaign or _campaign()
                assert campaign.explained_by_nudge(args, same)[0] is not None, "plan %d: no ulp of libm explains the device's answer" % i
            # the judge, on the device's answer: the candidates it examined, the search, the winner
            k = np.flatnonzero(flags[j])
            examined.append(rflags[k])
            judged = pc.Judged(cfg, np.tile(vel0[:, i], (len(k), 1)), np.tile(acc0[:, i], (len(k), 1)), np.tile(grav[:, i], (len(k), 1)), tables[table[i]][k])
            bad, seen = pc.violations(cfg, judged, flags[j][k])
            seen_all = pc.merge_seen(seen_all, seen)
            cost = pc.costs(cfg, pc.end_points(cfg, tables[table[i]]), tables[table[i]][:, 3], np.tile(vec[:, j], (M, 1)))
            low, best, n_checks = pc.replay(cost, flags[j])
            assert np.array_equal(low, flags[j] != 0) and best == o.best_index and n_checks == o.n_cost_checks, i
            assert o.found == (best >= 0) and o.n_generated == M
            if o.found:
                found += 1
                b, clear = pc.winner_violations(cfg, images[image_of[i]], judged, int(np.searchsorted(k, best)), coeffs[j], o.best_cost, cost[best])
                bad += b
                clearance_min = min(clearance_min, clear)
                assert o.tf == tables[table[i]][best, 3]
            assert bad == [], i
    assert hard <= 0.002 * n
    assert found >= n // 2
    seen_all.update(clearance_min=clearance_min, plans_found=found, plans_differing=hard)
    kinds = np.concatenate(examined)
    _record("whole_plans", oracle_flags_of_examined={str(v): int((kinds == v).sum()) for v in (1, 3, 7, 15)},
            seconds=round(time.perf_counter() - t0, 2), **seen_all)
    assert all((kinds == v).sum() > 0 for v in (1, 3, 7, 15))


@pytest.fixture(scope="module")
def twelve_states(ora):
    """test 1's planners on its synthetic images, two states per image"""
    vel0, acc0, grav = pc.aggressive_states(45, 36, upright_every=2)
    keep = np.flatnonzero((np.arange(36) < 18) & (np.arange(36) % 3 != 2))
    samples = pc.aggressive_samples(ora.planner_samples(0, 320, 240, M), 0)
    return dict(vel0=vel0[:, keep], acc0=acc0[:, keep], grav=grav[:, keep], samples=samples, image_of=keep // 3, judged=None)


@pytest.mark.parametrize("name,settings", [("section_time_0.5", dict(min_section_time=0.5)), ("section_time_1e-3", dict(min_section_time=1e-3)),
                                           ("section_time_1e-6", dict(min_section_time=1e-6)), ("tight_limits", TIGHT_LIMITS)])
def test_other_section_times_and_limits(ora, images, twelve_states, name, settings):
    """min_section_time 0.5 leaves sections undecided after three halvings, 1e-6 takes input_feasible's stack to 22 pending
    halves (of 24; afe_rappids_plan refuses what could pass 23); the tight limits move every threshold of both tests"""
    t0 = time.perf_counter()
    s = twelve_states
    ocfg, cfg = _configs(ora, 320, 240, 160.0, **settings)
    ref, dev, s["judged"], seen = _singles(ora, ocfg, cfg, images, s["image_of"], s["vel0"], s["acc0"], s["grav"], s["samples"], judged=s["judged"],
                                           max_winners=100)
    _record(name, oracle_shares=_shares(ref, name), seconds=round(time.perf_counter() - t0, 2), **seen)


def test_single_candidates_on_a_ragged_width(ora):
    """200 x 150 (rows that are no whole 64-pixel words), f = 100: the aggressive trajectories leave the field of view, start
    backwards (behind the camera) or come back below min_checking_dist, which no collision test of the tame ones does"""
    t0 = time.perf_counter()
    w, h, focal = 200, 150, 100.0
    imgs = np.stack([afa.scenarios.synthetic_depth_image(width=w, height=h, seed=500 + k, n_trunks=3 + k) for k in range(3)])
    ocfg, cfg = _configs(ora, w, h, focal)
    vel0, acc0, grav = pc.aggressive_states(45, 12, upright_every=2)
    vel0[2, ::4] *= -0.15          # (the distribution never moves backwards: three states that do, at up to 0.8 m/s)
    samples = pc.aggressive_samples(ora.planner_samples(3, w, h, 100), 3)
    ref, dev, judged, seen = _singles(ora, ocfg, cfg, imgs, np.arange(12) // 4, vel0, acc0, grav, samples)
    # what the tame tests never see: accepted trajectories that leave the image or pass behind min_checking_dist
    t = judged.T[:, None] * np.linspace(0, 1, 201)[None, :]
    P = pc._evaluate(judged.coeffs, t)
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = focal * P[:, :, 0] / P[:, :, 2] + w / 2.0, focal * P[:, :, 1] / P[:, :, 2] + h / 2.0
    outside = ((P[:, :, 2] > 0) & ((u < 0) | (u >= w) | (v < 0) | (v >= h))).any(axis=1)
    above = P[:, :, 2] >= MIN_DIST
    behind = (above[:, :-1] & ~above[:, 1:]).any(axis=1) | (P[:, :, 2] < 0).any(axis=1)      # back below min_checking_dist, or behind the camera
    checked = (ref.ravel() & 4) != 0
    assert (checked & outside).sum() >= 10 and (checked & behind).sum() >= 10
    _record("ragged_width", oracle_shares=_shares(ref, "200 x 150"), collision_checked_leaving_the_view=int((checked & outside).sum()),
            collision_checked_behind_min_dist=int((checked & behind).sum()), seconds=round(time.perf_counter() - t0, 2), **seen)
