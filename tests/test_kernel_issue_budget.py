"""The headline instantiation of the resident step grid -- afe_step_persistent_kernel<float, FEXT, libstdc++ noise, no
logic, one step> -- is bound by vector-instruction issue while its working set lives in the L2s (131 072 - 262 144 vehicles;
at 2^20 the bytes set the step), and a scalar value the compiler cannot keep in a scalar register
comes back through a v_readlane, a vector instruction.  The one-step grid therefore re-reads its constants from the
kernel-argument segment in its loops (afe_kernels.hip, RELOADS in afe_step_persistent_kernel) instead of keeping them alive across the poll
loop.  What that buys is visible in the code object's notes: .sgpr_spill_count was 165 before the change and is 90 in this
build (no lane operation left inside the chunk loop).  Held here: below 165, not above 96 (this build's 90 rounded up to a
multiple of 8), and still at most 80 vector registers, no scratch and the held inputs' 5 376 B of LDS.  Metadata only; read
from the built library like tests/test_kernel_resources.py, no GPU needed."""
import os
import re
import subprocess

import pytest

from tests.test_kernel_resources import LIB, READELF, gfx950_code_objects

HEADLINE = "afe_step_persistent_kernelIfLb1ELi1ELb0ELb0E"
KEYS = "sgpr_spill_count|vgpr_count|private_segment_fixed_size|group_segment_fixed_size"


def headline_notes(tmp_path):
    found = []
    for k, blob in enumerate(gfx950_code_objects(LIB)):
        f = tmp_path / ("budget%d.elf" % k)
        f.write_bytes(blob)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and HEADLINE in name.group(1):
                found.append({key: int(val) for key, val in re.findall(r"\.(%s):\s+(\d+)" % KEYS, block)})
    return found


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(READELF), reason="needs the built library and llvm-readelf")
def test_headline_kernel_keeps_its_scalars_out_of_vector_lanes(tmp_path):
    found = headline_notes(tmp_path)
    assert len(found) == 1, found
    m = found[0]
    assert m["sgpr_spill_count"] < 165, m           # the parent's
    assert m["sgpr_spill_count"] <= 96, m           # this build's 90, rounded up to a multiple of 8
    assert m["vgpr_count"] <= 80, m                 # six waves per SIMD
    assert m["private_segment_fixed_size"] == 0, m  # nothing in scratch
    assert m["group_segment_fixed_size"] == 5376, m # 3 chunks x 64 lanes x 28 B of held inputs
