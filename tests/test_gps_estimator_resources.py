"""The GPS + IMU estimator's kernels keep a vehicle's 9x9 covariance rows in registers with compile-time indices only; an
array the compiler could not take apart would be spilled to scratch memory.  Read from the code object inside the built
library, as tests/test_kernel_resources.py reads the step kernels': no GPU needed.  The register counts are recorded in
DESIGN.md section 4k, not bounded here."""
import os

import pytest

from tests.test_kernel_resources import LIB, READELF, kernel_metadata

KERNELS = ("afe_gps_estimator_imu_kernel", "afe_gps_estimator_measure_kernelIf", "afe_gps_estimator_measure_kernelId",
           "afe_gps_estimator_reset_kernel", "afe_gps_estimator_mark_kernel", "afe_gps_estimator_math_kernel")


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(READELF), reason="needs the built library and llvm-readelf")
def test_gps_estimator_kernels_use_no_scratch(tmp_path):
    kernels = kernel_metadata(tmp_path)
    for tag in KERNELS:
        mine = {n: m for n, m in kernels.items() if tag in n}
        assert len(mine) == 1, (tag, sorted(mine))
        (name, m), = mine.items()
        print(name, m)
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m.get("vgpr_spill_count", 0) == 0, (name, m)
        assert "afe_step" not in name
