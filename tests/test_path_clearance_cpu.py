"""Path clearance without a GPU: the pure-host sampler against the numpy statement of the definition
(tests/path_checker.py) bit for bit, the checker against values derived by hand, the record's layout and the new
kernels' register / scratch metadata."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from tests import path_checker as pc
from tests.test_kernel_resources import LIB, READELF, kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("K", [2, 3, 64, 65, 4096])
@pytest.mark.parametrize("placed", ["bare", "origin", "origin+rot"])
def test_sampler_equals_the_checker(afa, K, placed):
    rng = np.random.default_rng(100 + K)
    for _ in range(4):
        c = rng.normal(0, 1, (6, 3)) * np.array([0.01, 0.05, 0.3, 1.0, 3.0, 20.0])[:, None]
        tb, te = rng.uniform(-2, 2), rng.uniform(0.5, 3)
        o = rng.uniform(-4000, 4000, 3) if placed != "bare" else None
        R = rng.normal(0, 1, 9) if placed == "origin+rot" else None
        t, w = afa.path_sample_points(c, tb, te, o, R, K)
        want_t, want_w = pc.sample_points(c, tb, te, o, R, K)
        assert t.shape == (K,) and w.shape == (3, K)
        assert_array_equal(t, want_t)
        assert_array_equal(w, want_w)


@pytest.mark.parametrize("tb,te", [(0.25, 2.75), (3.0, -1.0), (1.5, 1.5), (0.0, 0.1), (-0.1, 1e9)])
def test_end_times_are_exact(afa, tb, te):
    c = np.zeros((6, 3))
    c[4] = 1.0
    for K in (2, 3, 7, 64, 100):
        t, w = afa.path_sample_points(c, tb, te, n_samples=K)
        assert t[0] == tb and t[-1] == te
        assert_array_equal(t, pc.sample_times(tb, te, K))
        if tb == te:
            assert (t == tb).all()
        assert_array_equal(w, np.stack([t, t, t]))      # p = ((((0*t + 0)*t + 0)*t + 0)*t + 1)*t + 0


def test_negative_zero_survives_without_an_origin(afa):
    c = np.zeros((6, 3))
    c[5] = -0.0
    c[4] = [1.0, 0.0, -1.0]
    for K in (2, 65):
        t, w = afa.path_sample_points(c, 0.0, 1.0, n_samples=K)
        _, want = pc.sample_points(c, 0.0, 1.0, n_samples=K)
        assert_array_equal(np.signbit(w), np.signbit(want))
        assert np.signbit(w[2, 0]) and w[2, 0] == 0        # -1*0 + -0 = -0: no zero was added
        assert not np.signbit(w[0, 0])                     # (1*0 + -0 = +0 is the arithmetic's own)
        # with an origin of +0 the sum is +0: the origin is added only where one is given
        _, w0 = afa.path_sample_points(c, 0.0, 1.0, origin=np.zeros(3), n_samples=K)
        assert not np.signbit(w0[2, 0])


def test_argument_errors_of_the_host_call(afa):
    L = afa.library()
    f = L.afe_path_sample_points
    c = np.zeros(18)
    o, R = np.zeros(3), np.zeros(9)
    t, w = np.empty(4096), np.empty(3 * 4096)
    ok = (c.ctypes.data, 0.0, 1.0, o.ctypes.data, R.ctypes.data, 8, t.ctypes.data, w.ctypes.data)

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return f(*a)
    assert call() == 0
    assert call(a0=None) == 1 and call(a6=None) == 1 and call(a7=None) == 1
    assert call(a3=None) == 1                   # rot without origin
    assert call(a3=None, a4=None) == 0 and call(a4=None) == 0
    for K in (1, 0, -1, 4097, 2 ** 31 - 1):
        assert call(a5=K) == 4
    assert call(a5=2) == 0 and call(a5=4096) == 0
    assert call(a1=float("nan")) == 0           # a NaN is data


# ---- the checker against values derived by hand ---------------------------------------------------------------

PLANE = np.array([[-8, -8, 0, 8, -8, 0, 0, 8, 0]], np.float32)      # one triangle in z = 0, the z axis well inside it


def test_checker_straight_descent():
    """z(t) = 1 - t over [0, 2] above one triangle in z = 0, K = 201: z_k = 1 - k/100 and d2_k = z_k^2 up to rounding.  The
    closest approach is the crossing, k = 100; inside radius 0.255 are exactly k = 75 .. 125 (|z_74| = 0.26, |z_75| = 0.25)."""
    c = np.zeros((1, 6, 3))
    c[0, 4, 2], c[0, 5, 2] = -1.0, 1.0
    rec, n_col = pc.audit(PLANE, c, np.array([[0.0], [2.0]]), n_samples=201, radius=0.255)
    r = rec[0]
    assert r["k_min"] == 100 and r["t_min"] == 1.0 and r["tri_min"] == 0
    assert 0.0 <= r["min_dist2"] <= 1e-24                    # (the foot point's barycentrics are rounded)
    assert np.abs(r["closest"]).max() <= 1e-12
    assert r["k_first_hit"] == 75 and r["n_hit"] == 51 and r["t_first_hit"] == 2.0 * (75.0 / 200.0)
    assert r["tri_first_hit"] == 0 and r["n_nonfinite"] == 0 and n_col == 1
    # the same descent seen with max_dist = radius: the hit fields and the minimum are what they were
    again, _ = pc.audit(PLANE, c, np.array([[0.0], [2.0]]), n_samples=201, radius=0.255, max_dist=0.255)
    pc.assert_records_equal(again, rec)
    # a path that stays 1 m above, search radius 0.5: nothing
    c[0, 4, 2], c[0, 5, 2] = 0.0, 1.0
    rec, n_col = pc.audit(PLANE, c, np.array([[0.0], [2.0]]), n_samples=9, radius=0.25, max_dist=0.5)
    pc.assert_records_equal(rec, pc.empty_records(1))
    assert n_col == 0


@pytest.mark.parametrize("radius,hits", [(0.4, 0), (0.6, 1)])
def test_checker_constant_path(radius, hits):
    """a point 0.5 m above the triangle for the whole range: every d2 has the same bits, so the first sample wins"""
    c = np.zeros((1, 6, 3))
    c[0, 5] = [0.25, -0.5, 0.5]
    K = 130
    ans = pc.sample_answers(PLANE, c, np.array([[0.0], [3.0]]), n_samples=K)
    assert (ans["d2"] == ans["d2"][0, 0]).all() and abs(ans["d2"][0, 0] - 0.25) <= 1e-15
    rec, n_col = pc.reduce_records(ans, radius)
    r = rec[0]
    assert r["min_dist2"] == ans["d2"][0, 0] and r["k_min"] == 0 and r["t_min"] == 0.0 and r["tri_min"] == 0
    assert np.abs(r["closest"] - [0.25, -0.5, 0.0]).max() <= 1e-12
    assert r["n_hit"] == hits * K and n_col == hits
    assert r["k_first_hit"] == (0 if hits else -1) and r["tri_first_hit"] == (0 if hits else -1)
    assert (r["t_first_hit"] == 0.0) if hits else np.isnan(r["t_first_hit"])


def test_checker_nan_coefficient():
    c = np.zeros((2, 6, 3))
    c[:, 5, 2] = 0.5
    c[1, 2, 1] = np.nan
    K = 70
    rec, n_col = pc.audit(PLANE, c, np.array([[0.0, 0.0], [1.0, 1.0]]), n_samples=K, radius=1.0)
    assert rec[0]["n_nonfinite"] == 0 and rec[0]["n_hit"] == K and n_col == 1
    want = pc.empty_records(1)
    want["n_nonfinite"] = K
    pc.assert_records_equal(rec[1:], want)


# ---- layout and resources ---------------------------------------------------------------------------------------

def test_record_layout_matches_the_header(afa, tmp_path):
    fields = [name for name, _ in afa.PathClearance._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "agrifly_engine.h"\n'
                   'int main(void){printf("%zu", sizeof(afe_path_clearance));\n' +
                   "".join('printf(" %%zu", offsetof(afe_path_clearance, %s));\n' % f for f in fields) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = list(map(int, subprocess.check_output([str(exe)]).split()))
    assert got[0] == 96 == C.sizeof(afa.PathClearance) == afa.PATH_CLEARANCE_DTYPE.itemsize == pc.RECORD_DTYPE.itemsize
    assert got[1:] == [getattr(afa.PathClearance, f).offset for f in fields]
    assert got[1:] == [afa.PATH_CLEARANCE_DTYPE.fields[f][1] for f in fields] == [pc.RECORD_DTYPE.fields[f][1] for f in fields]


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(READELF), reason="needs the built library and llvm-readelf")
def test_path_kernels_use_no_scratch(tmp_path):
    kernels = {n: m for n, m in kernel_metadata(tmp_path).items() if "afe_path_clearance_kernel" in n}
    assert len(kernels) == 3, sorted(kernels)           # explicit paths, their counting build, engine plans
    for name, m in kernels.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0, (name, m)
