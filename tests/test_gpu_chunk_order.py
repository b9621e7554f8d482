"""The one-step resident grid walks a worker's chunks forward in even steps and backward in odd ones (afe_kernels.hip, the chunk
loop of afe_step_persistent_kernel, TURNS), so that the last chunk of a step is the first of the next and stays in the L2.  What
that must not change is any bit: per-vehicle work does not depend on the order, PROVIDED every chunk is still paired with its
own held-input slot (its place with the worker) in both directions -- a wrong pairing hands vehicles another chunk's commands
and gust force.  So: per-vehicle random commands (tests.test_gpu_persistent.make), the 3 ms gust process
(tests.test_gpu_held_inputs.gusty), and everything compared bitwise with an AFE_STEP_LAUNCH engine, at the smallest shapes at
which each case of the loop occurs.  (The order is compiled into the fp32 reference-streams holding instantiation; the same
source loop serves the others in the fixed order, and they are held to the same script whichever order they are given.)

  255 workers (AFE_PERSIST_WAVES_PER_CU=1, dev-hooks library, child process)
    20 165 vehicles   316 chunks, 1 or 2 per worker: the shortest turn
    39 057 vehicles   611 chunks, 2 or 3 per worker: the headline's mix, all held, ragged last chunk
    67 209 vehicles 1 051 chunks, 4 or 5 per worker: both directions cross the held / unheld boundary (three slots)
  at 39 057 also fp32 counter noise (holding), fp64 and the on-device logic (not holding): the other arms of the same loop
  release library, in process: 524 365 vehicles, 8 194 chunks on the full grid, 1 or 2 per worker, ragged last chunk

Blocks of 1, 1, 1, 2, 3, 1, 8, 1 steps of 1 ms: polls that bring odd and even numbers of steps, so the direction has to follow
the absolute step and not the position in a poll; afe_sync after some blocks and not after others; new per-vehicle commands
once in the middle (the setter ends the grid after five steps: the next grid starts on an odd step, backward)."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_held_inputs import gusty
from tests.test_gpu_persistent import assert_same, make

afa = importlib.import_module("agri-fly_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BLOCKS = (1, 1, 1, 2, 3, 1, 8, 1)
SYNC_AFTER = (1, 4, 6)          # indices into BLOCKS
COMMANDS_AFTER = 3


def pair(n, variant):
    """(launched engine, resident-grid engine) of one variant, both on the 3 ms gust process"""
    out = []
    for persistent in (False, True):
        if variant == "logic":
            e, _ = make(n, afa.AFE_F32, persistent, logic=True, wrench=False)
            e.set_gust_process(True, seed=4, sigma_max=0.5, period_us=3000, n_global=n)
        else:
            e, _ = gusty(n, persistent, period_us=3000, precision=afa.AFE_F64 if variant == "fp64" else afa.AFE_F32)
            if variant == "counter":
                e.set_imu_noise(True, 0.1, 0.2, afa.AFE_SEED_COUNTER)
        out.append(e)
    return out


def same(a, b, what):
    assert_same(a, b, what)
    np.testing.assert_array_equal(a.get_external_force(), b.get_external_force(), err_msg=str(what))


def run_script(n, variant):
    a, b = pair(n, variant)
    rng = np.random.default_rng(33)
    p = afa.params_from_type(5)
    with a, b:
        for k, steps in enumerate(BLOCKS):
            a.step(1000, steps); b.step(1000, steps)
            if k in SYNC_AFTER:
                b.sync()
            if k == COMMANDS_AFTER:
                same(a, b, (n, variant, "before the new commands"))
                cmd = rng.uniform(0.3, 0.9, (4, n)).astype(np.float32) * np.float32(p.motor_max_speed)
                thrust = rng.uniform(9.0, 10.5, n).astype(np.float32)
                rates = (0.2 * rng.standard_normal((3, n))).astype(np.float32)
                for e in (a, b):
                    e.set_motor_cmds(cmd)
                    if variant == "logic":          # (the logic writes the motor commands at its ticks: its own inputs change too)
                        e.set_rates_commands(thrust, rates)
        same(a, b, (n, variant, "end"))
        assert a.steps_completed == b.steps_completed == sum(BLOCKS)


CHILD = r'''
import sys
sys.path.insert(0, %r)
from tests.test_gpu_chunk_order import run_script
run_script(%d, %r)
print("ok")
'''


def in_child_with_255_workers(n, variant):
    from tests.scenarios import dev_hooks_env
    env = dev_hooks_env()         # AFE_PERSIST_WAVES_PER_CU is a lab variable: the child runs on the -DAFE_DEV_HOOKS build
    if env is None:
        pytest.skip("no library with -DAFE_DEV_HOOKS (agri-fly_amd/lib/dev/, built by __graft_entry__.build())")
    env = dict(env, AFE_PERSIST_WAVES_PER_CU="1")
    out = subprocess.run([sys.executable, "-c", CHILD % (ROOT, n, variant)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


@pytest.mark.parametrize("n", [20165, 39057, 67209])
def test_both_directions_give_the_launched_bits(n):
    in_child_with_255_workers(n, "reference")


@pytest.mark.parametrize("variant", ["counter", "fp64", "logic"])
def test_every_one_step_grid_gets_the_order(variant):
    in_child_with_255_workers(39057, variant)


def test_full_grid_one_or_two_chunks_per_worker():
    n = 524365                     # 8 194 chunks, the last one ragged
    a, b = pair(n, "reference")
    with a, b:
        for _ in range(12):
            a.step(1000, 1); b.step(1000, 1)
        a.step(1000, 7); b.step(1000, 7)
        same(a, b, "524 365 vehicles")
