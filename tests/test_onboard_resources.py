"""The onboard flight computer's kernels are streaming kernels that keep a vehicle's state in registers with compile-time
indices only: no scratch memory, no spilled register.  Read from the code object inside the built library, as
tests/test_kernel_resources.py reads the step kernels': no GPU needed.  The register counts are recorded in DESIGN.md
section 4m, not bounded here."""
import os

import pytest

from tests.test_kernel_resources import LIB, READELF, kernel_metadata

KERNELS = ("afe_onboard_init_kernel", "afe_onboard_tick_kernel", "afe_onboard_telemetry_kernel", "afe_onboard_stamp_kernel",
           "afe_onboard_math_kernel")


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(READELF), reason="needs the built library and llvm-readelf")
def test_onboard_kernels_use_no_scratch(tmp_path):
    kernels = kernel_metadata(tmp_path)
    onboard = sorted(n for n in kernels if "afe_onboard_" in n)
    assert len(onboard) == len(KERNELS), onboard             # every afe_onboard_* kernel is one of the five
    for tag in KERNELS:
        mine = {n: m for n, m in kernels.items() if tag in n}
        assert len(mine) == 1, (tag, sorted(mine))
        (name, m), = mine.items()
        print(name, m)
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m.get("vgpr_spill_count", 0) == 0, (name, m)
        assert m.get("sgpr_spill_count", 0) == 0, (name, m)
