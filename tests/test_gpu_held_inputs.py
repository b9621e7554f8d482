"""The resident grid's held inputs (afe_kernels.hip persist_holds, AFE_PERSIST_HOLD): the fp32 one-step grid with an external
force reads the motor commands and the force once per grid into LDS instead of once per step.  What that must not change:
  * a grid that runs across gust epochs gives the launched bits (the grid's own waves write the new force to the slab AND
    to their LDS copy), also where a worker has more chunks than it holds;
  * new commands written between two blocks of steps act from the next step on (every setter ends the grid);
  * with an exported device view the grid reads from memory: a foreign write of the commands after afe_sync is seen;
  * afe_algorithmic_bytes_per_step reports what the grid that will step the engine moves: 28 B less per vehicle-step
    for the holding grid, the old count for every other path."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_persistent import assert_same, make

afa = importlib.import_module("agri-fly_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_ARENA = bool(os.environ.get("AFE_FORCE_HOST_ARENA"))      # (the suite's host-visible run: nothing is held there)


def gusty(n, persistent, period_us=3000, precision=None):
    e, d = make(n, afa.AFE_F32 if precision is None else precision, persistent, wrench=False)
    e.set_gust_process(True, seed=4, sigma_max=0.5, period_us=period_us, n_global=n)
    return e, d


def test_grid_across_gust_epochs_is_the_launched_bits():
    n = 70001                                  # 1 094 chunks, the last one ragged
    a, _ = gusty(n, False)
    b, _ = gusty(n, True)
    with a, b:
        for k in (1, 1, 2, 5, 1, 7, 3, 11, 1, 1):      # blocks that start and end inside and on the 3 ms epochs
            a.step(1000, k); b.step(1000, k)
        assert_same(a, b, "across gust epochs")
        np.testing.assert_array_equal(a.get_external_force(), b.get_external_force())
        b.step(1000, 40); a.step(1000, 40)
        assert_same(a, b, "40 steps in one block")
        np.testing.assert_array_equal(a.get_external_force(), b.get_external_force())


def test_more_chunks_than_a_worker_holds():
    """AFE_PERSIST_WAVES_PER_CU=1 leaves 255 worker waves: 65 613 vehicles are 1 026 chunks, four or five per wave -- three
    held, the rest read from memory, across gust epochs.  In a child process (the variable is read when the grid is sized)."""
    code = r'''
import importlib, sys, numpy as np
sys.path.insert(0, %r)
from tests.test_gpu_persistent import assert_same
from tests.test_gpu_held_inputs import gusty
a, _ = gusty(65536 + 77, False)
b, _ = gusty(65536 + 77, True)
for k in (1, 2, 30, 1, 9):
    a.step(1000, k); b.step(1000, k)
assert_same(a, b)
np.testing.assert_array_equal(a.get_external_force(), b.get_external_force())
print("ok")
''' % ROOT
    from tests.scenarios import dev_hooks_env
    env = dev_hooks_env()         # AFE_PERSIST_WAVES_PER_CU is a lab variable: the child runs on the -DAFE_DEV_HOOKS build
    if env is None:
        pytest.skip("no library with -DAFE_DEV_HOOKS (agri-fly_amd/lib/dev/, built by __graft_entry__.build())")
    env = dict(env, AFE_PERSIST_WAVES_PER_CU="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


def test_new_commands_between_blocks_act_at_the_next_step():
    n = 20000
    a, _ = gusty(n, False)
    b, _ = gusty(n, True)
    rng = np.random.default_rng(21)
    p = afa.params_from_type(5)
    with a, b:
        for block in range(4):
            for _ in range(3):
                a.step(1000, 1); b.step(1000, 1)
            b.sync()
            cmd = rng.uniform(0.3, 0.9, (4, n)).astype(np.float32) * np.float32(p.motor_max_speed)
            a.set_motor_cmds(cmd); b.set_motor_cmds(cmd)
            a.step(1000, 1); b.step(1000, 1)
            assert_same(a, b, "block %d" % block)
            np.testing.assert_array_equal(b.get_motor_cmds(), cmd)


def test_exported_view_sees_a_foreign_write_of_the_commands():
    import torch
    n = 20000
    a, _ = gusty(n, False)
    b, _ = gusty(n, True)
    p = afa.params_from_type(5)
    with a, b:
        a.step(1000, 4); b.step(1000, 4)
        v = b.device_view()                     # from here on somebody else may write the slabs

        class _Wrap:
            def __init__(self, ptr, shape):
                self.__cuda_array_interface__ = dict(shape=shape, typestr="<f4", data=(ptr, False), version=2, strides=None)
        cmd_dev = torch.as_tensor(_Wrap(v.motor_cmd, (4, v.stride)), device="cuda")[:, :n]
        rng = np.random.default_rng(8)
        for block in range(3):
            b.step(1000, 3); a.step(1000, 3)
            b.sync()
            cmd = rng.uniform(0.3, 0.9, (4, n)).astype(np.float32) * np.float32(p.motor_max_speed)
            cmd_dev.copy_(torch.from_numpy(cmd))          # the foreign writer, between afe_sync and the next afe_step
            torch.cuda.synchronize()
            a.set_motor_cmds(cmd)
            b.step(1000, 2); a.step(1000, 2)
            assert_same(a, b, "foreign write %d" % block)


def test_byte_accounting_follows_the_grid_that_steps():
    n = 4096
    es = 4
    launched_off = 13 * es * 2 + 16 + 3 * es + (4 * es if HOST_ARENA else 0)     # state r/w, commands, force (rotor speeds: host arena only)
    launched_on = launched_off + 24 + 8                                           # IMU sample, engine word r/w
    held = 0 if HOST_ARENA else 16 + 3 * es
    e, _ = gusty(n, True)
    with e:
        assert e.algorithmic_bytes_per_step(False) == launched_off - held
        assert e.algorithmic_bytes_per_step(True) == launched_on - held
        e.step(1000, 5)
        assert e.algorithmic_bytes_per_step(False) == launched_off - held           # (the grid that ran: every chunk held)
        e.set_step_mode(afa.AFE_STEP_LAUNCH)
        assert (e.algorithmic_bytes_per_step(False), e.algorithmic_bytes_per_step(True)) == (launched_off, launched_on)
        e.set_step_mode(afa.AFE_STEP_RESIDENT)                                      # the resident-state grid: as it was
        assert (e.algorithmic_bytes_per_step(False), e.algorithmic_bytes_per_step(True)) == (launched_off, launched_on)
        e.set_step_mode(afa.AFE_STEP_PERSISTENT)
        assert e.algorithmic_bytes_per_step(False) == launched_off - held
        e.device_view()                                                             # exported: read from memory again
        assert (e.algorithmic_bytes_per_step(False), e.algorithmic_bytes_per_step(True)) == (launched_off, launched_on)
    f, _ = make(n, afa.AFE_F32, True, wrench=False)                                 # no force stream: nothing held
    with f:
        assert f.algorithmic_bytes_per_step(False) == 13 * es * 2 + 16 + (4 * es if HOST_ARENA else 0)
    g, _ = gusty(n, True, precision=afa.AFE_F64)                                    # fp64: nothing held
    with g:
        assert g.algorithmic_bytes_per_step(False) == 13 * 8 * 2 + 16 + 3 * 8 + (4 * 8 if HOST_ARENA else 0)
