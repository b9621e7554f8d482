"""The planner on every image-shape path (tests/planner_shapes.py), judged against the oracle with
tests/test_gpu_planner.py's own comparison: chosen candidate, every candidate's flags and every counter identical,
coefficients to 1e-12.  Needs an MI355X.  Every item records its seconds in the measurement ledger."""
import contextlib
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

from tests import planner_shapes as ps
from tests.scenarios import MEASUREMENTS, afa, dev_hooks_env
from tests.test_gpu_planner import _compare

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@contextlib.contextmanager
def _timed(item):
    t0 = time.perf_counter()
    yield
    MEASUREMENTS.setdefault("planner_shapes_seconds", {})[item] = round(time.perf_counter() - t0, 3)


def _plan(cls, inp, images=None, max_pyramids=64):
    return afa.rappids_plan(ps.engine_config(cls, max_pyramids), inp["images"] if images is None else images, inp["vel0"], inp["acc0"],
                            inp["grav"], inp["samples"], image_index=inp["image_index"], want_flags=True)


def _bytes(out, flags):
    return np.concatenate([np.frombuffer(bytes(out), np.uint8), flags.ravel()])


@pytest.mark.parametrize("cls", ps.CLASSES, ids=repr)
def test_host_images_of_every_class_plan_like_the_oracle(ora, cls):
    with _timed("host[%s]" % cls.name):
        refs = ps.oracle_refs(ora, cls.name)
        out, flags, _ = _plan(cls, ps.inputs(cls.name))
        _compare(out, flags, refs)


@pytest.mark.parametrize("name", ps.DEVICE_RESIDENT)
def test_device_resident_images_plan_like_the_oracle(ora, name):
    """The chain of the config-3 test at this camera size: three views of the 2 x 3 orchard, image == the checker's render,
    plan (from the images in HBM) == the oracle on that image.  201 x 151 images start on 2-byte boundaries and go pixel by
    pixel; 202 x 150 ones take the dword path with rows that start off every 16-byte boundary."""
    with _timed("device[%s]" % name):
        cls = ps.BY_NAME[name]
        tris = afa.scenarios.orchard_mesh(rows=2, cols=3, seed=7)
        mount = afa.camera_default_mount()
        pos = np.array([[-3.0, -2.0, -2.5], [2.0, 5.5, 3.5], [1.2, 1.5, 1.0]])
        yaw = np.array([0.0, 0.0, 0.35])
        att = np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)])
        cam = afa.camera_default(cls.w, cls.h)
        assert cam.focal_length == cls.focal
        scene = afa.Scene(tris)
        images, _ = scene.render(cam, pos, att, mount)
        scene.close()
        ocam = ora.render_camera(cls.w, cls.h)
        for i in range(3):
            np.testing.assert_array_equal(images[i], ora.render_depth(ocam, tris, pos[:, i], att[:, i], mount), err_msg="view %d" % i)
        inp = dict(ps.inputs(name), images=images)
        refs = ps.run_oracle(ora, ps.oracle_config(ora, cls), **inp)
        assert sum(r.n_pyramids for r, _ in refs) >= 3 * ps.N_PLANS and any(r.found for r, _ in refs)      # orchard views: cluttered
        buf = afa.DeviceBuffer(images.nbytes)
        try:
            buf.upload(images)
            out, flags, _ = _plan(cls, inp, images=buf)
            _compare(out, flags, refs)
            host_out, host_flags, _ = _plan(cls, inp)
            assert np.array_equal(_bytes(out, flags), _bytes(host_out, host_flags))
        finally:
            buf.close()


def test_pyramid_list_in_lanes_and_in_memory_agree_on_odd_images():
    """max_pyramids 64 keeps the sorted pyramid list in the wave's lanes, 65 in memory; no plan comes near either limit
    (tests/test_planner_shapes_cpu.py), so both must give the same bytes -- here on the pixel-by-pixel image path"""
    with _timed("lanes_vs_memory[201x151]"):
        cls, inp = ps.BY_NAME["201x151"], ps.inputs("201x151")
        res = [_plan(cls, inp, max_pyramids=limit) for limit in (64, 65)]
        assert max(o.n_pyramids for o in res[0][0]) >= 2
        assert np.array_equal(_bytes(*res[0][:2]), _bytes(*res[1][:2]))


_NO_SUMS_CHILD = r"""
import importlib, sys, numpy as np
sys.path.insert(0, %r)
from tests import planner_shapes as ps
afa = ps.afa
assert afa.library().afe_has_dev_hooks()
parts = []
for name in ps.NO_SUMS_CLASSES:
    inp = ps.inputs(name)
    out, flags, _ = afa.rappids_plan(ps.engine_config(ps.BY_NAME[name]), inp["images"], inp["vel0"], inp["acc0"], inp["grav"], inp["samples"],
                                     image_index=inp["image_index"], want_flags=True)
    parts.append(np.concatenate([np.frombuffer(bytes(out), np.uint8), flags.ravel()]))
np.save(sys.argv[1], np.concatenate(parts))
"""


def test_summaries_and_plain_sweep_give_the_same_bytes(ora):
    """64 x 48, 128 x 64 and 320 x 240 build their bit images from the per-word summaries; with the lab variable
    AFE_PLANNER_NO_SUMS (a child process on the -DAFE_DEV_HOOKS build) the same shapes go through build_mask with rows of
    whole words.  The child's bytes must be the release library's, which in turn are judged against the oracle."""
    with _timed("summaries_vs_plain"):
        env = dev_hooks_env()
        assert env is not None, "no library with -DAFE_DEV_HOOKS (agri-fly_amd/lib/dev/, built by __graft_entry__.build())"
        want = []
        for name in ps.NO_SUMS_CLASSES:
            out, flags, _ = _plan(ps.BY_NAME[name], ps.inputs(name))
            _compare(out, flags, ps.oracle_refs(ora, name))
            want.append(_bytes(out, flags))
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "no_sums.npy")
            r = subprocess.run([sys.executable, "-c", _NO_SUMS_CHILD % ROOT, path], env=dict(env, AFE_PLANNER_NO_SUMS="1"),
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            got = np.load(path)
        assert np.array_equal(got, np.concatenate(want))


@pytest.mark.parametrize("name", [c.name for c in ps.SEAM_CLASSES])
def test_images_on_both_sides_of_the_launch_seam(ora, name):
    """65 537 images: the prepare kernel is launched for 65 535 of them and then for the last two.  All are a wall but six
    -- two at the start, two that end the first launch, the two of the second -- and the 32 plans look at those six; the
    oracle's answers on them differ from one another and from the wall's (tests/test_planner_shapes_cpu.py)."""
    with _timed("seam[%s]" % name):
        s = ps.seam_inputs(name)
        cls = s["cls"]
        refs = [ora.planner_run(ps.oracle_config(ora, cls), s["special"][s["which"][i]], s["vel0"][:, i], s["acc0"][:, i], s["grav"][:, i],
                                s["samples"]) for i in range(ps.SEAM_PLANS)]
        images = ps.seam_image_array(name)
        assert images.shape[0] == ps.SEAM_IMAGES > ps.GRID_Z + 1
        try:
            out, flags, _ = afa.rappids_plan(ps.engine_config(cls), images, s["vel0"], s["acc0"], s["grav"], s["samples"],
                                             image_index=s["image_index"], want_flags=True)
        finally:
            afa.planner_release_scratch()          # half a gigabyte of images and as much again transposed
        _compare(out, flags, refs)
