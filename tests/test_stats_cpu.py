"""Ensemble statistics without a GPU: the layout check of the C ABI, the ABI record's layout, and the properties of the
summation tree that the GPU parity test (tests/test_gpu_stats.py) relies on."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from tests import stats_checker as ck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, OUT_OF_RANGE = 1, 4
SIZES = [0, 1, 255, 256, 257, 65793]


def wide_range_leaves(n, seed=0):
    """squares of normals scaled over eight decades: a summation order shows in the last bits"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 4, n)) ** 2


def test_check_layout_counts_and_levels(afa):
    edges = np.concatenate([[7], 7 + np.cumsum(SIZES)])
    n = int(edges[-1]) + 5
    assert afa.stats_check_layout(edges, n) == (0 + 1 + 1 + 1 + 2 + 258, 17)
    for size, chunks, levels in [(0, 0, 0), (1, 1, 0), (2, 1, 1), (255, 1, 8), (256, 1, 8), (257, 2, 9), (65793, 258, 17), (1 << 20, 4096, 20)]:
        assert afa.stats_check_layout([3, 3 + size], 3 + size) == (chunks, levels), size
    # the outputs are optional
    ed = np.array([0, 10], np.int64)
    assert afa.library().afe_stats_check_layout(ed.ctypes.data, 1, 10, None, None) == 0


def test_check_layout_refusals(afa):
    L = afa.library()

    def rc(edges, n_vehicles, n_groups=None):
        ed = np.ascontiguousarray(edges, np.int64)
        return L.afe_stats_check_layout(ed.ctypes.data, ed.size - 1 if n_groups is None else n_groups, n_vehicles, None, None)

    assert rc([0, 10, 20], 20) == 0
    assert rc([0, 10, 10, 20], 20) == 0                 # an empty group
    assert rc([0, 10, 9], 20) == INVALID_ARG            # decreasing
    assert rc([0, 10, 21], 20) == OUT_OF_RANGE          # beyond n_vehicles
    assert rc([-1, 10], 20) == INVALID_ARG              # negative
    assert rc([0, 10], 20, n_groups=0) == INVALID_ARG
    assert rc(np.zeros(65538), 20) == INVALID_ARG       # 65537 groups
    assert rc(np.zeros(65537), 20) == 0                 # 65536 groups
    assert rc([0, 0], -1) == INVALID_ARG
    assert L.afe_stats_check_layout(None, 1, 20, None, None) == INVALID_ARG
    with pytest.raises(afa.AfeError):
        afa.stats_check_layout([5, 4], 10)


def test_group_stats_layout_matches_header(afa, tmp_path):
    src = tmp_path / "gs.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "agrifly_engine.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu\\n", sizeof(afe_group_stats), offsetof(afe_group_stats, argmax_peak_h2),'
                   ' offsetof(afe_group_stats, sum_h2), offsetof(afe_group_stats, min_min_up)); return 0;}\n')
    exe = tmp_path / "gs"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, o_arg, o_sum, o_last = map(int, subprocess.check_output([str(exe)]).split())
    assert size == C.sizeof(afa.GroupStats) == afa.GROUP_STATS_DTYPE.itemsize == ck.DTYPE.itemsize == 23 * 8
    assert o_arg == afa.GroupStats.argmax_peak_h2.offset == afa.GROUP_STATS_DTYPE.fields["argmax_peak_h2"][1]
    assert o_sum == afa.GroupStats.sum_h2.offset == afa.GROUP_STATS_DTYPE.fields["sum_h2"][1]
    assert o_last == afa.GroupStats.min_min_up.offset == afa.GROUP_STATS_DTYPE.fields["min_min_up"][1]
    assert afa.GROUP_STATS_DTYPE == ck.DTYPE


def test_tree_equals_chunked_form():
    """256-leaf subtrees aligned to the start, then the tree over the partials: the same bits at every size"""
    a = wide_range_leaves(65793, seed=1)
    for n in list(range(1, 1026)) + [65793]:
        assert ck.tree_sum(a[:n]) == ck.chunked_tree_sum(a[:n]), n
    for n in (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 65793):      # and with 64-leaf subtrees (the wave butterfly)
        assert ck.tree_sum(a[:n]) == ck.chunked_tree_sum(a[:n], width=64), n
    assert ck.tree_sum([]) == 0.0 and not np.signbit(ck.tree_sum([]))
    assert ck.tree_sum([3.5]) == 3.5
    # exactly representable: the tree is a sum
    assert ck.tree_sum(np.arange(1000.0)) == 999 * 1000 / 2


def test_tree_is_not_a_left_to_right_sum():
    """on wide-range inputs the tree's bits differ from a loop's, so bit parity with the checker tells them apart"""
    sizes = (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 65793)
    a = wide_range_leaves(65793, seed=0)
    differs = 0
    for n in sizes:
        loop = 0.0
        for x in a[:n]:
            loop = loop + x
        tree = ck.tree_sum(a[:n])
        assert abs(tree - loop) <= 1e-12 * loop          # the same sum ...
        differs += tree != loop                          # ... in another order
    assert differs >= 4


def test_invalid_leaf_changes_only_its_own_contribution():
    """an invalid vehicle's leaf is +0.0: the tree's shape (who is paired with whom) does not move"""
    a = np.floor(wide_range_leaves(1000, seed=2) * 1e3) + 1.0      # integers < 2^53 / 1000: every partial sum is exact
    a = np.minimum(a, 2.0 ** 40)
    full = ck.tree_sum(a)
    for k in (0, 1, 63, 64, 255, 256, 999):
        b = a.copy()
        b[k] = 0.0
        assert ck.tree_sum(b) == full - a[k], k
    # and in floating point: zeroing leaf k equals the tree with leaf k's subtree partner passed through unchanged
    w = wide_range_leaves(8, seed=3)
    z = w.copy()
    z[5] = 0.0
    want = ((w[0] + w[1]) + (w[2] + w[3])) + ((w[4] + 0.0) + (w[6] + w[7]))
    assert ck.tree_sum(z) == want
    # the per-vehicle quantities: a non-finite value anywhere makes the vehicle invalid and nothing else
    n = 16
    st = dict(pos=np.ones((3, n)), vel=np.ones((3, n)), att=np.tile([[1.0], [0], [0], [0]], (1, n)), ang_vel=np.zeros((3, n)))
    st["vel"][1, 3] = np.nan
    st["att"][2, 7] = np.inf
    st["pos"][2, 9] = -1.0
    ref = np.zeros((3, n))
    ref[0, 11] = np.nan
    q = ck.quantities(st, ref)
    assert_array_equal(np.flatnonzero(~q["valid"]), [3, 7, 11])
    assert_array_equal(np.flatnonzero(q["grounded"]), [9])
    lat = ck.Latches(n)
    rec, hist = ck.update(st, ref, lat, [0, 8, 8, 16], 1234, hist_edges=[1.0, 2.0])
    assert_array_equal(rec["count"], [8, 0, 8])
    assert_array_equal(rec["n_invalid"], [2, 0, 1])
    assert_array_equal(rec["sum_h2"], [12.0, 0.0, 14.0])
    assert rec["max_h2"][1] == -np.inf and rec["min_up"][1] == np.inf and rec["argmax_h2"][1] == -1
    assert_array_equal(hist.sum(1), rec["count"] - rec["n_invalid"])
    assert_array_equal(lat.first_invalid_us[[3, 7, 11]], [1234] * 3)
    assert lat.first_grounded_us[9] == 1234 and (lat.n_valid == q["valid"]).all()
