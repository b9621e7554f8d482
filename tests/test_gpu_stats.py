"""Ensemble statistics on the device (afe_stats_*, agri-fly_amd/csrc/afe_stats.hip) against the numpy statement of the
definition (tests/stats_checker.py): every field of every group record, the per-vehicle latches and the histogram are EQUAL
(numpy.testing.assert_array_equal: the two zeros count as equal, nothing else does)."""
import ctypes as C
import importlib
import time

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from tests import scenarios as tscen
from tests import stats_checker as ck
from tests.scenarios import random_ensemble

afa = importlib.import_module("agri-fly_amd")
pytestmark = pytest.mark.gpu

AFE_F32, AFE_F64 = afa.AFE_F32, afa.AFE_F64
INVALID_ARG, OUT_OF_RANGE = 1, 4
NEVER = ck.NEVER

# the awkward shapes: 37 vehicles before the first edge, 1185 after the last; the last group has 258 chunks (257 full ones
# and one of a single vehicle): two tiles in the group kernel, the second with two partials
GROUP_SIZES = [1, 0, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 65793]
LEAD, N = 37, 70000
EDGES = LEAD + np.concatenate([[0], np.cumsum(GROUP_SIZES)])
assert EDGES[-1] < N


def same_records(got, want, groups=None):
    for k in ck.DTYPE.names:
        g, w = (got[k], want[k]) if groups is None else (got[k][groups], want[k][groups])
        assert_array_equal(g, w, err_msg=k)


def same_latches(mon, lat, first=0, count=None):
    got, want = mon.latches(first, count), lat.as_dict(first, count)
    for k in want:
        assert_array_equal(got[k], want[k], err_msg=k)


@pytest.fixture(scope="module")
def awkward():
    """one ensemble of 70 000: positions over +-50 m, velocities and rates over five decades, attitudes tilted up to 60 deg;
    reference points at distances over six decades, so h2 spans twelve"""
    ens = random_ensemble(N, seed=11)
    d = ens.data
    rng = np.random.default_rng(12)
    d.pos[0] = rng.uniform(-50, 50, N)
    d.pos[1] = rng.uniform(-50, 50, N)
    d.vel *= 10.0 ** rng.uniform(-3, 2, N)
    d.ang_vel *= 10.0 ** rng.uniform(-3, 2, N)
    # what an fp32 engine can hold exactly, so that both precisions start from the same numbers
    for k in ("pos", "vel", "att", "ang_vel", "motor_speed"):
        setattr(d, k, getattr(d, k).astype(np.float32).astype(np.float64))
    ref = d.pos + rng.standard_normal((3, N)) * 10.0 ** rng.uniform(-4, 2, N)
    return ens, ref


@pytest.mark.parametrize("precision", [AFE_F32, AFE_F64])
def test_parity_at_the_awkward_shapes(awkward, precision):
    ens, ref = awkward
    assert afa.stats_check_layout(EDGES, N) == (sum(-(-s // 256) for s in GROUP_SIZES), 17)
    with ens.to_engine(precision) as e:
        mon = afa.StatsMonitor(e, EDGES)
        assert mon.info() == {"n_groups": len(GROUP_SIZES), "n_vehicles": N, "n_hist_edges": 0, "n_updates": 0}
        mon.set_reference(ref)
        lat = ck.Latches(N)
        for k_update in range(2):
            st, now = e.get_state(), e.time_us
            rec, hist = mon.update()
            want, _ = ck.update(st, ref, lat, EDGES, now)
            assert hist is None
            same_records(rec, want)
            same_latches(mon, lat)
            if k_update == 0:
                # the input is not tame: a left-to-right sum gives other bits than the tree for at least one group
                h2 = ck.quantities(st, ref)["h2"]
                differs = 0
                for a, b in zip(EDGES[:-1], EDGES[1:]):
                    loop = 0.0
                    for x in h2[a:b]:
                        loop = loop + x
                    differs += loop != ck.tree_sum(h2[a:b])
                assert differs >= 1
                assert (want["n_invalid"] == 0).all() and want["count"].tolist() == GROUP_SIZES
                e.step(1000, 3)
        assert mon.info()["n_updates"] == 2
        # vehicles before the first edge and after the last were never touched
        for first, count in ((0, LEAD), (int(EDGES[-1]), N - int(EDGES[-1]))):
            out = mon.latches(first, count)
            assert (out["peak_h2"] == 0).all() and np.isinf(out["min_up"]).all() and (out["acc_h2"] == 0).all()
            assert (out["n_valid"] == 0).all() and (out["first_grounded_us"] == NEVER).all() and (out["first_invalid_us"] == NEVER).all()
        inside = mon.latches(LEAD, int(EDGES[-1]) - LEAD)
        assert (inside["n_valid"] == 2).all()
        mon.close()


@pytest.mark.parametrize("precision", [AFE_F32, AFE_F64])
def test_invalid_and_grounded_vehicles(awkward, precision):
    ens, ref = awkward
    d = ens.data
    big = int(EDGES[11])                   # first vehicle of the 65 793 group
    plant = {"pos": [big + 3 * 256, int(EDGES[10]) + 5], "vel": [big + 3 * 256 + 63], "att": [big + 7 * 256 + 64], "ang_vel": [big + 7 * 256 + 127]}
    whole_chunk = np.arange(big + 5 * 256, big + 6 * 256)
    whole_group = np.arange(EDGES[2], EDGES[3])            # the group of 63: all invalid
    low = np.array([int(EDGES[10]) + 100, int(EDGES[10]) + 101, big + 1000])

    def engine(planted):
        e = ens.to_engine(precision)
        if planted:
            pos, vel, att, w = d.pos.copy(), d.vel.copy(), d.att.copy(), d.ang_vel.copy()
            pos[0, plant["pos"][0]] = np.nan
            pos[2, plant["pos"][1]] = np.inf
            vel[1, plant["vel"]] = -np.inf
            att[3, plant["att"]] = np.nan
            w[2, plant["ang_vel"]] = np.inf
            vel[0, whole_chunk] = np.nan
            att[0, whole_group] = np.nan
            # on or below the ground, sinking, nothing that could lift them: they stay grounded while stepped
            pos[2, low] = [0.0, -0.5, -1e-3]
            vel[2, low] = -1.0
            speed, cmd, force = d.motor_speed.copy(), d.motor_cmd.copy(), d.ext_force.copy()
            speed[:, low], cmd[:, low], force[:, low] = 0.0, 0.0, 0.0
            e.set_state(pos, vel, att, w, speed)
            e.set_motor_cmds(cmd)
            e.set_external_force(force)
        return e

    results = {}
    for planted in (False, True):
        with engine(planted) as e:
            mon = afa.StatsMonitor(e, EDGES)
            mon.set_reference(ref)
            lat = ck.Latches(N)
            e.step(1000, 2)
            st, now = e.get_state(), e.time_us
            assert now == 2000
            rec, _ = mon.update()
            want, _ = ck.update(st, ref, lat, EDGES, now)
            same_records(rec, want)
            same_latches(mon, lat)
            results[planted] = rec
            if planted:
                bad = np.concatenate([sum(plant.values(), []), whole_chunk, whole_group])
                assert (lat.first_invalid_us[bad] == 2000).all() and (lat.n_valid[bad] == 0).all()
                assert rec["n_invalid"][11] == 4 + 256 and rec["n_invalid"][10] == 1 and rec["n_invalid"][2] == 63
                assert rec["argmax_h2"][2] == -1 and rec["max_h2"][2] == -np.inf and rec["min_up"][2] == np.inf and rec["sum_h2"][2] == 0
                assert rec["argmax_peak_h2"][2] == EDGES[2] and rec["max_peak_h2"][2] == 0       # the latches are still initial
                assert rec["n_grounded"][10] >= 2 and (lat.first_grounded_us[low] == 2000).all()
                # the vehicles recover: "now" counts drop, the "ever" counts and the time latches stay
                e.set_state(d.pos, d.vel, d.att, d.ang_vel, d.motor_speed)
                e.step(1000, 1)
                st, now = e.get_state(), e.time_us
                rec2, _ = mon.update()
                want2, _ = ck.update(st, ref, lat, EDGES, now)
                same_records(rec2, want2)
                same_latches(mon, lat)
                assert rec2["n_invalid"][2] == 0 and rec2["n_ever_invalid"][2] == 63 and (lat.first_invalid_us[bad] == 2000).all()
            mon.close()
    clean_groups = [0, 1, 3, 4, 5, 6, 7, 8, 9]
    same_records(results[True], results[False], clean_groups)
    assert results[True]["sum_h2"][11] != results[False]["sum_h2"][11]


def test_reference_handling():
    n = 2000
    edges = [0, 700, 2000]
    ens = random_ensemble(n, seed=3, type_ids=(5,))
    rng = np.random.default_rng(4)
    with ens.to_engine(AFE_F32) as e:
        mon = afa.StatsMonitor(e, edges)
        lat = ck.Latches(n)
        ref = e.get_state()["pos"].copy()              # creation marks where the vehicles are
        for k in range(4):
            e.step(1000, 5)
            if k == 1:                                 # explicit points for a sub-range
                pts = rng.uniform(-3, 3, (3, 300))
                mon.set_reference(pts, first=650)
                ref[:, 650:950] = pts
            if k == 2:                                 # mark on the device for another, latches of a third back to initial
                mon.mark(first=100, count=257)
                ref[:, 100:357] = e.get_state()["pos"][:, 100:357]
                mon.reset(first=690, count=20)
                lat.reset(690, 20)
            st, now = e.get_state(), e.time_us
            rec, _ = mon.update()
            want, _ = ck.update(st, ref, lat, edges, now)
            same_records(rec, want)
            same_latches(mon, lat)
        assert (lat.n_valid[690:710] == 2).all() and (lat.n_valid[:690] == 4).all()
        mon.close()


def test_fp32_engine_far_from_the_origin():
    """4 km out an fp32 x has an ulp of 0.24 mm; the slab holds the offset from the set point and the anchor is added in
    double, so a 1 mm move shows"""
    n = 300
    p = afa.params_from_type(5)
    d = afa.scenarios.hover_ensemble(n, p)
    d.pos[0] = 4000.0 + 4.0 * np.arange(n)
    d.pos[1] = -4000.0
    d.vel[0] = 0.1
    e = afa.Ensemble(n, precision=AFE_F32)
    e.set_type_table([p])
    e.set_state(d.pos, d.vel, d.att, d.ang_vel, d.motor_speed)
    e.set_motor_cmds(d.motor_cmd)
    mon = afa.StatsMonitor(e, [0, n])
    ref = e.get_state()["pos"].copy()
    e.step(1000, 10)
    st, now = e.get_state(), e.time_us
    rec, _ = mon.update()
    want, _ = ck.update(st, ref, ck.Latches(n), [0, n], now)
    same_records(rec, want)
    lat = mon.latches()
    assert (lat["peak_h2"] > 0).all()
    assert 0 < rec["sum_h2"][0] / n <= 1.01e-6 and rec["max_h2"][0] <= 1.01e-6      # (1 mm)^2; drag can only shorten the move
    mon.close(); e.close()


def test_histogram():
    n = 3000
    edges = [10, 1000, 1000, 2990]
    ens = random_ensemble(n, seed=6, type_ids=(5,))
    d = ens.data
    rng = np.random.default_rng(7)
    ref = np.round(d.pos * 4) / 4
    k = rng.integers(0, 8, n).astype(np.float64)
    d.pos[0], d.pos[1], d.pos[2] = ref[0] + 3 * k, ref[1] + 4 * k, ref[2] + 1.0        # h2 = (5 k)^2 exactly, in fp32 too
    d.vel[0, [20, 1500, 1501]] = np.nan
    hist_edges = [2.5, 5.0, 10.0, 15.0, 17.0, 35.0, 50.0]
    with ens.to_engine(AFE_F32) as e:
        mon = afa.StatsMonitor(e, edges)
        mon.set_reference(ref)
        mon.set_histogram(hist_edges)
        assert mon.info()["n_hist_edges"] == 7
        lat = ck.Latches(n)
        st, now = e.get_state(), e.time_us
        rec, hist = mon.update()
        want, want_hist = ck.update(st, ref, lat, edges, now, hist_edges)
        same_records(rec, want)
        assert_array_equal(hist, want_hist)
        assert hist.shape == (3, 8) and hist.dtype == np.int64
        assert_array_equal(hist.sum(1), rec["count"] - rec["n_invalid"])
        ok = ck.quantities(st, ref)["valid"][10:1000]
        h2 = ck.quantities(st, ref)["h2"][10:1000][ok]
        assert set(np.unique(h2)) <= {(5.0 * j) ** 2 for j in range(8)}
        # a vehicle exactly on an edge belongs to the bin above it
        assert hist[0][2] == (h2 == 25.0).sum() > 0 and hist[0][3] == (h2 == 100.0).sum() > 0 and hist[0][4] == (h2 == 225.0).sum() > 0
        assert hist[0][0] == (h2 == 0).sum() and hist[0][5] == ((h2 == 400.0) | (h2 == 625.0) | (h2 == 900.0)).sum() and hist[0][7] == 0
        # 63 edges: every bin the kernel has
        many = 0.5 + 0.6 * np.arange(63)
        mon.set_histogram(many)
        rec, hist = mon.update()
        want, want_hist = ck.update(st, ref, lat, edges, now, many)
        same_records(rec, want)
        assert_array_equal(hist, want_hist)
        assert hist.shape == (3, 64)
        # and off again
        mon.set_histogram(None)
        assert mon.info()["n_hist_edges"] == 0
        rec, hist = mon.update()
        want, _ = ck.update(st, ref, lat, edges, now)
        assert hist is None
        same_records(rec, want)
        mon.close()


def test_latches_over_time():
    """64 vehicles drop from 5 cm with their motors off, the others hover; twenty updates ten steps apart"""
    n, n_drop = 364, 64
    edges = [0, n_drop, n]
    p = afa.params_from_type(5)
    d = afa.scenarios.hover_ensemble(n, p)
    d.pos[0] = np.arange(n) * 0.5
    d.pos[2, :n_drop] = 0.05
    d.motor_speed[:, :n_drop] = 0.0
    d.motor_cmd[:, :n_drop] = 0.0
    d.vel[0, n_drop:] = 0.3                    # the hovering ones drift: h2 grows
    e = afa.Ensemble(n, precision=AFE_F32)
    e.set_type_table([p])
    e.set_state(d.pos, d.vel, d.att, d.ang_vel, d.motor_speed)
    e.set_motor_cmds(d.motor_cmd)
    mon = afa.StatsMonitor(e, edges)
    ref = e.get_state()["pos"].copy()
    lat = ck.Latches(n)
    ever = []
    for k in range(20):
        e.step(1000, 10)
        st, now = e.get_state(), e.time_us
        assert now == 10000 * (k + 1)
        rec, _ = mon.update()
        want, _ = ck.update(st, ref, lat, edges, now)
        same_records(rec, want)
        same_latches(mon, lat)
        ever.append(int(rec["n_ever_grounded"][0]))
    assert ever[0] == 0 and ever[-1] == n_drop and rec["n_ever_grounded"][1] == 0 and rec["n_grounded"][0] == n_drop
    got = mon.latches()
    t = got["first_grounded_us"][:n_drop]
    assert (t == t[0]).all() and 90000 <= t[0] <= 120000            # sqrt(2 * 0.05 / 9.81) = 0.101 s
    assert (got["first_grounded_us"][n_drop:] == NEVER).all() and (got["n_valid"] == 20).all()
    assert (got["acc_h2"][n_drop:] > got["peak_h2"][n_drop:]).all() and (got["peak_h2"][n_drop:] > 0.03 ** 2).all()
    mon.close(); e.close()


def _make(n, mode):
    ens = random_ensemble(n, seed=5, type_ids=(5,))
    d = ens.data
    e = afa.Ensemble(n, precision=AFE_F32)
    e.set_type_table([afa.params_from_type(5)])
    e.set_logic_period(1 / 500)
    e.set_imu_noise(True, 0.1, 0.2, afa.AFE_SEED_DECORRELATED)
    e.set_state(d.pos, d.vel, d.att, d.ang_vel, d.motor_speed)
    e.set_motor_cmds(d.motor_cmd)
    e.set_external_force(d.ext_force)
    e.set_split_stepping(1)
    e.set_step_mode(mode)
    return e


def _everything(e):
    gyro, acc = e.get_imu()
    return dict(e.get_state(), gyro=gyro, acc=acc, rng=e.get_rng_state(), time=np.array([e.time_us, e.logic_ticks, e.steps_completed]))


@pytest.mark.parametrize("mode", [afa.AFE_STEP_LAUNCH, afa.AFE_STEP_PERSISTENT])
def test_the_engine_is_not_disturbed(mode):
    n = 5000
    edges = [0, 1234, 5000]
    plain, watched, probe = _make(n, mode), _make(n, mode), _make(n, afa.AFE_STEP_LAUNCH)
    mon = afa.StatsMonitor(watched, edges)
    ref = probe.get_state()["pos"].copy()
    plain.step(1000, 20)
    watched.step(1000, 10)
    rec, _ = mon.update()                      # in persistent mode this ends the resident grid ...
    watched.step(1000, 10)                     # ... and stepping resumes
    probe.step(1000, 10)
    want, _ = ck.update(probe.get_state(), ref, ck.Latches(n), edges, probe.time_us)
    same_records(rec, want)
    a, b = _everything(plain), _everything(watched)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert b["time"][2] == 20
    mon.close()
    for e in (plain, watched, probe):
        e.close()


def test_boundary_with_live_handles():
    n = 1000
    edges = np.array([0, 400, 1000], np.int64)
    ens = random_ensemble(n, seed=8, type_ids=(5,))
    L = afa.library()
    big = 2 ** 63 - 1
    with ens.to_engine(AFE_F32) as e, ens.to_engine(AFE_F32) as other:
        mon = afa.StatsMonitor(e, edges)
        lat = ck.Latches(n)
        ref = e.get_state()["pos"].copy()
        e.step(1000, 4)
        rec0, _ = mon.update()
        want, _ = ck.update(e.get_state(), ref, lat, edges, e.time_us)
        same_records(rec0, want)
        h = mon._h
        rec = np.zeros(2, afa.GROUP_STATS_DTYPE)
        hist = np.zeros((2, 64), np.int64)
        buf = np.zeros(3 * n)
        # NULL outputs, a histogram that was never asked for
        assert L.afe_stats_update(h, None, None) == INVALID_ARG
        assert L.afe_stats_update(h, rec.ctypes.data, hist.ctypes.data) == INVALID_ARG
        assert L.afe_stats_update(None, rec.ctypes.data, None) == INVALID_ARG
        # ranges: negative, beyond the end, wrapping
        for first, count, code in ((-1, 1, INVALID_ARG), (0, -1, INVALID_ARG), (n + 1, 0, OUT_OF_RANGE), (0, n + 1, OUT_OF_RANGE),
                                   (n, 1, OUT_OF_RANGE), (big, big, OUT_OF_RANGE), (1, big, OUT_OF_RANGE), (-big, big, INVALID_ARG)):
            assert L.afe_stats_get(h, first, count, buf.ctypes.data, None, None, None, None, None) == code, (first, count)
            assert L.afe_stats_reset(h, first, count) == code, (first, count)
            assert L.afe_stats_set_reference(h, first, count, buf.ctypes.data) == code, (first, count)
            assert L.afe_stats_set_reference(h, first, count, None) == code, (first, count)
        # count == 0 with a valid range
        for first in (0, 17, n):
            assert L.afe_stats_get(h, first, 0, None, None, None, None, None, None) == 0
            assert L.afe_stats_reset(h, first, 0) == 0
            assert L.afe_stats_set_reference(h, first, 0, None) == 0
        # a reference that is not finite
        bad = np.zeros((3, 10))
        bad[2, 9] = np.nan
        assert L.afe_stats_set_reference(h, 5, 10, bad.ctypes.data) == INVALID_ARG
        bad[2, 9] = np.inf
        assert L.afe_stats_set_reference(h, 5, 10, bad.ctypes.data) == INVALID_ARG
        # histogram edges: unordered, repeated, not finite, not positive, too many, NULL with a count
        for ed in ([1.0, 0.5], [1.0, 1.0], [1.0, np.nan], [1.0, np.inf], [0.0, 1.0], [-1.0, 1.0], list(np.arange(1.0, 65.0))):
            a = np.array(ed)
            assert L.afe_stats_set_histogram(h, a.ctypes.data, a.size) == INVALID_ARG, ed
        assert L.afe_stats_set_histogram(h, None, 3) == INVALID_ARG
        assert L.afe_stats_set_histogram(h, buf.ctypes.data, -1) == INVALID_ARG
        # edges made for an ensemble of another size, and the other refusals of creation
        out = C.c_void_p()
        wrong = np.array([0, 400, 1001], np.int64)
        assert L.afe_stats_create(other.handle, wrong.ctypes.data, 2, C.byref(out)) == OUT_OF_RANGE and not out.value
        assert L.afe_stats_create(other.handle, edges.ctypes.data, 2, None) == INVALID_ARG
        assert L.afe_stats_create(other.handle, None, 2, C.byref(out)) == INVALID_ARG
        assert L.afe_stats_create(None, edges.ctypes.data, 2, C.byref(out)) == INVALID_ARG
        assert L.afe_stats_create(other.handle, edges.ctypes.data, 0, C.byref(out)) == INVALID_ARG
        assert L.afe_stats_create(other.handle, edges[::-1].copy().ctypes.data, 2, C.byref(out)) == INVALID_ARG and not out.value
        assert L.afe_stats_destroy(None) == INVALID_ARG and L.afe_stats_info(None, None, None, None, None) == INVALID_ARG
        # no trace: info, latches and the next update are what they would have been
        assert mon.info() == {"n_groups": 2, "n_vehicles": n, "n_hist_edges": 0, "n_updates": 1}
        same_latches(mon, lat)
        e.step(1000, 4)
        rec1, hist1 = mon.update()
        want, _ = ck.update(e.get_state(), ref, lat, edges, e.time_us)
        assert hist1 is None
        same_records(rec1, want)
        same_latches(mon, lat)
        mon.close()


def test_at_size_once():
    """2^20 vehicles, fp32, 8 equal groups, after 100 steps under the gust process on the rates logic: BASELINE config 4's
    sweep, whose per-bin mean square deviation is a numpy mean over the downloaded state"""
    n = 1 << 20
    p = afa.params_from_type(5)
    d = afa.scenarios.hover_ensemble(n, p)
    idx = np.arange(n)
    d.pos[0], d.pos[1] = (idx % 1024) * 4.0, (idx // 1024) * 4.0
    e = afa.Ensemble(n, precision=AFE_F32)
    e.set_type_table([p])
    e.set_logic_period(1 / 500)
    e.set_imu_noise(True, 0.1, 0.2, afa.AFE_SEED_COUNTER)
    e.set_noise_seed(5)
    e.set_state(d.pos, d.vel, d.att, d.ang_vel, d.motor_speed)
    e.set_motor_cmds(d.motor_cmd)
    e.set_gust_process(True, seed=4, sigma_max=0.5, period_us=100000, n_global=n)
    e.set_rates_logic([afa.rates_logic_params_from_type(5)])
    e.set_rates_commands(np.full(n, 9.81, np.float32), np.zeros((3, n), np.float32))
    e.set_step_mode(afa.AFE_STEP_AUTO)
    edges = np.linspace(0, n, 9).astype(int)
    mon = afa.StatsMonitor(e, edges)
    p0 = e.get_state()["pos"]
    e.step(1000, 100)
    e.sync()
    mon.update()                               # (warm: the first launch loads the code object)
    mon.reset()
    t0 = time.perf_counter()
    rec, _ = mon.update()
    ms = (time.perf_counter() - t0) * 1e3
    tscen.MEASUREMENTS["stats_update_1048576_ms"] = ms
    print("afe_stats_update at 2^20 vehicles, 8 groups: %.3f ms" % ms)
    st = e.get_state()
    want, _ = ck.update(st, p0, ck.Latches(n), edges, e.time_us)
    same_records(rec, want)
    dev2 = (st["pos"][0] - p0[0]) ** 2 + (st["pos"][1] - p0[1]) ** 2
    assert (rec["n_invalid"] == 0).all() and (rec["sum_h2"] > 0).all()
    for g, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        mean = rec["sum_h2"][g] / (rec["count"][g] - rec["n_invalid"][g])
        assert abs(mean - dev2[a:b].mean()) <= 1e-12 * dev2[a:b].mean(), g
    mon.close(); e.close()
