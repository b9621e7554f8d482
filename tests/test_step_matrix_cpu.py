"""Completeness of tests/step_matrix.py, without a GPU: the step kernels in the gfx950 code object of the built library
and step_matrix.cells() are the same set.  A template flag or a dispatch branch added later without a cell fails here, and
so does a cell whose variant is no longer compiled.  Kernel NAMES only are read (the code object's notes, as
tests/test_kernel_resources.py does)."""
import collections
import os

import pytest

from tests import step_matrix as sm
from tests.test_kernel_resources import LIB, READELF, kernel_metadata

needs_library = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(READELF), reason="needs the built library and llvm-readelf")


def test_cells_are_distinct_and_well_formed():
    cells = sm.cells()
    assert len(set(cells)) == len(cells)
    assert len({sm.key(c) for c in cells}) == len(cells)
    assert set(sm.UNREACHABLE) <= set(cells) and all(isinstance(r, str) and r for r in sm.UNREACHABLE.values())
    for c in cells:
        assert c.family in sm.FAMILIES and c.precision in sm.PRECISIONS and c.noise in (0, 1, 2)
        assert (c.cp is not None) == (c.family == "args_single") and (c.resident is not None) == (c.family == "grid")
        if c.cp:
            assert c.buf and not c.text
        if c.family == "grid":
            assert c.buf and not c.text
        assert sum(sum(p) for p in sm.script_of(c)) == sm.STEPS


def test_cell_of_reads_the_template_arguments():
    assert sm.cell_of("_ZN3afe15afe_step_kernelIfLb1ELb0ELi2ELb0ELb1ELb1ELi3EEEvNS_8StepViewIT_EENS_9DevParamsIS2_EENS_8DevLogicE") == \
        sm.Cell("args_single", "f32", True, False, 2, False, True, 3, None)
    assert sm.cell_of("_Z15afe_step_kernelIdLb0ELb1ELi1ELb1ELb0ELb0ELi0EEv8StepViewIT_E9DevParamsIS1_E8DevLogic") == \
        sm.Cell("args_fused", "f64", False, True, 1, True, False, None, None)
    assert sm.cell_of("_ZN3afe26afe_step_kernel_wave_typesIdLb1ELb1ELi0ELb0ELb1EEEvNS_8StepViewIT_EE").family == "wave_types"
    assert sm.cell_of("_Z21afe_step_kernel_tableIfLb1ELb1ELi2ELb1ELb0EEv8StepViewIT_E") == \
        sm.Cell("table", "f32", True, True, 2, True, False, None, None)
    assert sm.cell_of("_ZN3afe26afe_step_persistent_kernelIfLb1ELi2ELb0ELb0EEEvNS_8StepViewIT_EENS_9DevParamsIS2_EENS_8DevLogicENS_11PersistArgsE") == \
        sm.Cell("grid", "f32", True, False, 2, False, True, None, False)
    for unknown in ("_Z21afe_step_kernel_tableIfLb1ELb1ELi2ELb1ELb0ELb1EEv8StepViewIT_E",      # one flag more
                    "_Z26afe_step_persistent_kernelIfLb1ELi2ELb0EEv8StepViewIT_E",             # one flag fewer
                    "_Z15afe_step_kernelIfLb1ELb0ELi2ELb0ELb0ELb1ELi3EEv8StepViewIT_E",        # a fused launch with a cache policy
                    "_ZN3afe20afe_step_kernel_fastIfLb1EEEvNS_8StepViewIT_EE", "_ZN3afe15afe_gust_kernelIfEEvPT_"):
        with pytest.raises(ValueError):
            sm.cell_of(unknown)
    assert sm.is_step_kernel("_ZN3afe20afe_step_kernel_fastIfLb1EEEvNS_8StepViewIT_EE") and not sm.is_step_kernel("_ZN3afe15afe_gust_kernelIfEEvPT_")


@needs_library
def test_cells_are_the_step_kernels_of_the_code_object(tmp_path):
    symbols = [n for n in kernel_metadata(tmp_path) if sm.is_step_kernel(n)]
    of = {n: sm.cell_of(n) for n in symbols}                       # (raises on a template or a flag the matrix does not know)
    per_cell = collections.Counter(of.values())
    assert not [c for c, k in per_cell.items() if k > 1], "two symbols map to one cell"
    compiled, stated = set(of.values()), set(sm.cells())
    assert compiled == stated, ("compiled without a cell: %s; cells that are not compiled: %s"
                                % (sorted(sm.key(c) for c in compiled - stated), sorted(sm.key(c) for c in stated - compiled)))
    per_family = collections.Counter(c.family for c in stated)
    print("step kernels in the code object: %d -- %s" % (len(symbols), ", ".join("%s %d" % (f, per_family[f]) for f in sm.FAMILIES)))
    assert all(per_family[f] for f in sm.FAMILIES)
