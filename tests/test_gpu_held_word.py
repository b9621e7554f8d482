"""The resident grid's held engine word (afe_kernels.hip HeldWords, WORD in afe_step_persistent_kernel): the headline's grid -- fp32,
one step, external force, reference noise streams -- keeps the `rng` word of each held chunk in a vector register for its
lifetime.  A tick neither loads nor stores it; the worker writes its words back to the slab where it leaves the kernel (park
entry, give-up).  What that must not change, judged bitwise against launched steps (state, IMU samples, engine words,
commands, clock):
  * blocks of every length, ticks opening and closing blocks in both step parities: every getter parks the grid, so every
    comparison reads words that the write-back put there;
  * a worker with more chunks than it holds: held and memory-served words side by side;
  * every way a grid ends: the idle park, retirement between two calls, a setter, new words from the host, a checkpoint;
  * one grid serving several calls with nothing in between that parks it;
  * an exported device view: the word is read from memory, a foreign write is seen at the next tick."""
import importlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests.test_gpu_held_inputs import gusty
from tests.test_gpu_persistent import assert_same

afa = importlib.import_module("agri-fly_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SMALL = 4160                                  # 65 chunks: the ways a grid ends, each in the seconds range


def test_mixed_block_lengths_in_both_tick_parities():
    n = 70001                                   # 1 094 chunks, the last one ragged
    a, _ = gusty(n, False)
    b, _ = gusty(n, True)
    with a, b:
        for period in (1 / 500, 0.003):         # a tick every 2nd step, then every 3rd: ticks meet even and odd steps
            a.set_logic_period(period); b.set_logic_period(period)
            for k in (1, 1, 2, 5, 1, 7, 3, 11):
                a.step(1000, k); b.step(1000, k)
                assert_same(a, b, (period, k))
        assert a.logic_ticks == b.logic_ticks > 0


def test_held_and_memory_served_words_in_one_worker():
    """AFE_PERSIST_WAVES_PER_CU=1 leaves 255 worker waves: 65 613 vehicles are 1 026 chunks, four or five per wave -- three
    words in registers, the rest loaded and stored at every tick.  In a child process (the variable is read when the grid is sized)."""
    code = r'''
import importlib, sys, numpy as np
sys.path.insert(0, %r)
from tests.test_gpu_persistent import assert_same
from tests.test_gpu_held_inputs import gusty
a, _ = gusty(65536 + 77, False)
b, _ = gusty(65536 + 77, True)
for k in (1, 2, 30, 1, 9, 4):
    a.step(1000, k); b.step(1000, k)
    assert_same(a, b, k)
print("ok")
''' % ROOT
    from tests.scenarios import dev_hooks_env
    env = dev_hooks_env()         # AFE_PERSIST_WAVES_PER_CU is a lab variable: the child runs on the -DAFE_DEV_HOOKS build
    if env is None:
        pytest.skip("no library with -DAFE_DEV_HOOKS (agri-fly_amd/lib/dev/, built by __graft_entry__.build())")
    env = dict(env, AFE_PERSIST_WAVES_PER_CU="1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


def _pair():
    a, d = gusty(N_SMALL, False)
    b, _ = gusty(N_SMALL, True)
    return a, b, d


def test_idle_park_between_blocks():
    a, b, _ = _pair()
    with a, b:
        for k in (3, 1, 4, 2):
            b.step(1000, k); a.step(1000, k)
            time.sleep(0.01)                    # 50 x the grid's patience: it has parked itself, words written back
            assert_same(a, b, ("idle park", k))


def test_retirement_between_two_calls():
    """A grid is retired on entry to afe_step once it has served 512 steps (65 workers: no issue priority, retirement on).
    The second call finds a live grid of 520 steps, parks it and starts the next, which takes the written-back words over;
    no getter in between, and 600 steps against the launched run's one uninterrupted block."""
    a, b, _ = _pair()
    with a, b:
        b.step(1000, 520)                       # (returns once the steps are authorised: about a millisecond of work for the grid)
        b.step(1000, 80)                        # the first grid is alive and 520 steps old here: retired, the next one launched
        a.step(1000, 600)
        assert_same(a, b, "retired")


def test_one_grid_across_several_calls():
    """Blocks arriving back to back, nothing in between that parks: one holding grid serves them all from its registers."""
    a, b, _ = _pair()
    with a, b:
        for k in (1, 2, 1, 5, 3, 1, 1, 8):      # (microseconds apart; the grid parks itself only after 200 us of quiet)
            b.step(1000, k)
        a.step(1000, 22)
        assert_same(a, b, "several calls")


def test_new_commands_between_blocks():
    a, b, d = _pair()
    with a, b:
        for block in range(3):
            a.step(1000, 3); b.step(1000, 3)
            cmd = np.clip(d.motor_cmd * (1.0 + 0.03 * block), 0, None)
            a.set_motor_cmds(cmd); b.set_motor_cmds(cmd)
            a.step(1000, 2); b.step(1000, 2)
            assert_same(a, b, ("commands", block))


def test_new_noise_seed_between_blocks():
    a, b, _ = _pair()
    with a, b:
        for block in range(3):
            a.step(1000, 3); b.step(1000, 3)
            a.set_noise_seed(77 + block); b.set_noise_seed(77 + block)
            a.step(1000, 2); b.step(1000, 2)    # what the setter left in the slab acts from the next tick
            assert_same(a, b, ("noise seed", block))


def test_new_words_from_the_host_act_from_the_next_tick():
    a, b, _ = _pair()
    rng = np.random.default_rng(12)
    with a, b:
        for block in range(3):
            a.step(1000, 3); b.step(1000, 3)
            words = rng.integers(1, 2147483646, N_SMALL, dtype=np.uint32)
            a.set_rng_state(words); b.set_rng_state(words)
            np.testing.assert_array_equal(b.get_rng_state(), words)
            a.step(1000, 2); b.step(1000, 2)
            assert_same(a, b, ("words", block))
            assert not np.array_equal(b.get_rng_state(), words)      # (a tick has advanced them)


def test_checkpoint_in_mid_run_resumes_bitwise():
    a, b, _ = _pair()
    with a, b:
        a.step(1000, 25); b.step(1000, 25)
        blob = b.save_checkpoint()              # parks the grid: the blob carries the words the registers held
        b.step(1000, 7)
        c, _ = gusty(N_SMALL, True)
        with c:
            c.load_checkpoint(blob)
            c.step(1000, 30)
            a.step(1000, 30)                    # the launched run, never interrupted
            assert_same(a, c, "restored")
        b.step(1000, 23)
        assert_same(a, b, "the engine that saved")


@pytest.mark.parametrize("persistent", [False, True])
def test_exported_view_sees_a_foreign_write_of_the_words(persistent):
    import torch
    n = N_SMALL
    a, _ = gusty(n, False)                      # launched, the host's setter
    b, _ = gusty(n, persistent)                 # launched / grid, the foreign writer through the view
    with a, b:
        a.step(1000, 4); b.step(1000, 4)
        v = b.device_view()                     # from here on somebody else may write the slabs: nothing is held

        class _Wrap:
            def __init__(self, ptr, shape):
                self.__cuda_array_interface__ = dict(shape=shape, typestr="<i4", data=(ptr, False), version=2, strides=None)
        rng_dev = torch.as_tensor(_Wrap(v.rng, (n,)), device="cuda")
        rng = np.random.default_rng(9)
        for block in range(3):
            b.step(1000, 3); a.step(1000, 3)
            b.sync()
            words = rng.integers(1, 2147483646, n, dtype=np.uint32)
            rng_dev.copy_(torch.from_numpy(words.astype(np.int32)))      # between afe_sync and the next afe_step
            torch.cuda.synchronize()
            a.set_rng_state(words)
            b.step(1000, 2); a.step(1000, 2)
            assert_same(a, b, ("foreign write", block))
