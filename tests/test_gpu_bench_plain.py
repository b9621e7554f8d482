"""bench.py without --full: one line with the headline, exactly the steps it was given, and --dump-outputs -- the same
outputs from two runs with the same arguments, equal to what the ensemble bench.py builds holds after those steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pos", "vel", "att", "ang_vel", "motor_speed", "gyro", "acc")


def _plain_run(args, cwd):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, cwd=str(cwd),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_dumps_the_same_outputs_twice_and_they_are_the_steps_it_was_given(tmp_path, afa):
    import bench
    n, k, w = 1 << 20, 20, 5
    runs = []
    for i in range(2):
        out = tmp_path / ("run%d" % i)
        line = _plain_run(["--steps", str(k), "--warmup", str(w), "--vehicles", str(n), "--dump-outputs", str(out)], tmp_path)
        assert line["steps"] == k and line["warmup"] == w and line["n_gpus"] == 1 and line["dtype"] == "f32" and line["higher_is_better"] is True
        assert line["value"] == pytest.approx(n / (line["ms_per_step"] * 1e-3), rel=1e-4)
        assert "roofline" not in line and "detail" not in line and "cpu_baseline" not in line
        files = sorted(os.listdir(out))
        assert files == sorted(name + ".npy" for name in NAMES)
        assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
        arrays = {name: np.load(out / (name + ".npy")) for name in NAMES}
        assert all(a.dtype == np.float32 and a.shape[1] == bench.DUMP_VEHICLES for a in arrays.values())
        runs.append(arrays)
    for name in NAMES:
        assert np.array_equal(runs[0][name], runs[1][name], equal_nan=True), name
    # the same ensemble, stepped here through the warm-up, the settle and the timed steps, one afe_step call each, and read
    # through the engine's own getters; the sample drawn here as documented: 2^19 vehicles, numpy's default_rng(20), sorted
    assert bench.DUMP_VEHICLES == 1 << 19 and bench.DUMP_SEED == 20
    pick = np.sort(np.random.default_rng(20).choice(n, 1 << 19, replace=False))
    e = bench.build_shard(afa, n, 0, n, 0)
    for _ in range(w + bench.settle_steps(n) + k):
        e.step(bench.DT_US, 1)
    st = e.get_state(dtype=np.float32)
    gyro, acc = e.get_imu()
    e.close()
    want = dict(st, gyro=gyro, acc=acc)
    want = {name: want[name][:, pick] for name in NAMES}
    assert np.isfinite(want["pos"]).all()
    for name in NAMES:
        assert np.array_equal(runs[0][name], want[name], equal_nan=True), name
