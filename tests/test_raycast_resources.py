"""The ray kernels' resources are a property of the BUILD: the walk's stack lives in LDS so that nothing goes to scratch
(a runtime-indexed private array would), and nothing may spill.  Read from the code object inside the built library: no
GPU needed."""
import os
import re
import subprocess

import pytest

from tests.test_kernel_resources import LIB, READELF, gfx950_code_objects

STACK_BYTES = 32 * 256 * 4          # [level][lane] of uint32: afe_raycast.hip, THE WALK
KEYS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")


def raycast_kernels(tmp_path):
    kernels = {}
    for k, blob in enumerate(gfx950_code_objects(LIB)):
        f = tmp_path / ("ray%d.elf" % k)
        f.write_bytes(blob)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and "afe_raycast_kernel" in name.group(1):
                kernels[name.group(1)] = {key: int(val) for key, val in re.findall(r"\.(%s):\s+(\d+)" % "|".join(KEYS), block)}
    return kernels


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(READELF), reason="needs the built library and llvm-readelf")
def test_raycast_kernels_use_no_scratch_and_exactly_the_stack(tmp_path):
    kernels = raycast_kernels(tmp_path)
    # explicit rays (first hit), the same counting, line of sight (any hit), the engine's sensor
    assert len(kernels) == 4, sorted(kernels)
    for tag in ("ILi0ELb0ELb0E", "ILi0ELb0ELb1E", "ILi1ELb1ELb0E", "ILi2ELb0ELb0E"):
        assert sum(tag in n for n in kernels) == 1, (tag, sorted(kernels))
    for name, m in kernels.items():
        print(name, m)
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == STACK_BYTES, (name, m)
