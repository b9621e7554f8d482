"""The planner's shape matrix is complete, its inputs make the planner work, and the scans' division is exact on every
image the API accepts -- all without the engine (tests/planner_shapes.py; flown on the device by tests/test_gpu_planner_shapes.py).

The oracle alone on each class's inputs (3 synthetic images, 24 plans, 96 candidates, at most 64 pyramids, cost type 1):

    class      focal  plans found  pyramids  collision checks  candidates free / in collision
    201x151    100.5      24          58          330               173 / 157
    202x151    101        24          58          321               184 / 137
    202x150    101        24          42          321               184 / 137
    64x48       32        24          40          314               182 / 132
    65x49       32.5      24          53          313               186 / 127
    40x30       20        24          45          316               165 / 151
    128x64      64        24          42          317               115 / 202
    129x65      64.5      24          77          384               128 / 256
    48x400      24        24          60          146                61 /  85
    832x628    416        24          72          316               183 / 133
    1024x512   512        23          42          429               143 / 286
    8192x64     80        19          24          341                56 /  47
    2048x256   128        24         109          264               120 /  26

(8192x64 with the default focal length, width / 2, is a slit in which no candidate fits: nothing to plan.  At 80 pixels
every plan grows exactly one pyramid, thousands of pixels wide.)"""
import ctypes as C

import numpy as np
import pytest

from tests import planner_shapes as ps

OUT_OF_RANGE, NO_DEVICE = 4, 2
# shape -> (a line length inner <= max(W, H), the first index i < W * H whose quotient by it is wrong, how many are): these
# pass ceil(W / 64) * H * 8 <= 65536 and W * H < 2^24, the only limits there were
COUNTEREXAMPLES = {(9000, 56): (8960, 501759, 1), (12000, 40): (11972, 371131, 10), (16000, 32): (15960, 351119, 11)}


def test_every_value_of_every_row_is_taken_and_declared_paths_are_the_dispatch():
    for cls in ps.CLASSES + ps.SEAM_CLASSES:
        assert ps.accepted(cls.w, cls.h), cls
        assert set(cls.paths) == set(ps.PATH_VALUES), cls
        assert cls.paths == ps.paths_of(cls.w, cls.h, cls.n_images), cls
    for row, values in ps.PATH_VALUES.items():
        taken = {cls.paths[row] for cls in ps.CLASSES + ps.SEAM_CLASSES}
        assert taken == set(values), (row, taken)
    # the plain sweep over whole 64-pixel rows is reached both ways: by shape, and by the lab variable on summaries shapes
    assert all(ps.paths_of(w, h)["bit_image"] == "summaries" for w, h in ps.NO_SUMS_SHAPES)
    assert {ps.paths_of(w, h)["mask_divide"] for w, h in ps.NO_SUMS_SHAPES} == {"inner_one", "multiply_high"}
    # the seam is flown with and without summaries
    assert {c.paths["bit_image"] for c in ps.SEAM_CLASSES} == {"summaries", "partial_word"}
    assert all(c.paths["prepare_launches"] == "two" and c.n_images - ps.GRID_Z == 2 for c in ps.SEAM_CLASSES)
    # device-resident images: odd rows from 2-byte-aligned starts, dwords at a width that is no multiple of 8, and the summaries
    dev = [ps.BY_NAME[n] for n in ps.DEVICE_RESIDENT]
    assert any(c.paths["prepare"] == "pixel" and (c.w * c.h * 2) % 4 == 2 for c in dev)
    assert any(c.paths["prepare"] == "dword" and c.paths["width_mod_8"] == "nonzero" for c in dev)
    assert any(c.paths["bit_image"] == "summaries" for c in dev)
    # the names of the issue's boundary cases
    assert ps.paths_of(1024, 512)["bit_image"] == "whole_words" and (1024 // 64) * 512 * 8 == ps.LDS_BYTES
    assert 8192 * 64 * 8192 == ps.DIV_DOMAIN and (8192 // 64) * 64 * 8 == ps.LDS_BYTES
    assert ps.paths_of(129, 65)["transpose"] == "padded" and (65 + 63) // 64 * 64 == 128


@pytest.mark.parametrize("cls", ps.CLASSES, ids=repr)
def test_the_oracle_alone_has_work_on_every_class(ora, cls):
    """conditions on the INPUTS (no engine): a class whose plans meet nothing would pass whatever the kernels do"""
    refs = ps.oracle_refs(ora, cls.name)
    assert len(refs) == ps.N_PLANS
    flags = np.stack([f for _, f in refs])
    assert sum(r.n_pyramids for r, _ in refs) >= ps.N_PLANS                  # one pyramid per plan on average
    assert sum(r.n_collision_checks for r, _ in refs) >= 100
    assert (flags == 15).any() and (flags == 7).any()                        # collision-free and in-collision candidates
    assert sum(r.found for r, _ in refs) >= ps.N_PLANS // 2
    assert max(r.n_pyramids for r, _ in refs) < 64                           # nowhere near the limit: 64 and 65 must agree


@pytest.mark.parametrize("name", [c.name for c in ps.SEAM_CLASSES])
def test_the_seam_images_cannot_be_mistaken_for_one_another(ora, name):
    """the oracle's answer for every one of the 32 plans differs between its own image, the wall and each of the other
    five special images: a plan that read the wrong image -- a neighbour's, or the wall -- does not pass"""
    s = ps.seam_inputs(name)
    cls = s["cls"]
    ocfg = ps.oracle_config(ora, cls)
    candidates = np.concatenate([s["special"], np.full((1, cls.h, cls.w), ps.SEAM_WALL, np.uint16)])
    assert set(s["which"].tolist()) == set(range(6))
    found = 0
    for i in range(ps.SEAM_PLANS):
        runs = [ora.planner_run(ocfg, candidates[k], s["vel0"][:, i], s["acc0"][:, i], s["grav"][:, i], s["samples"]) for k in range(7)]
        sigs = [ps.signature(*r) for r in runs]
        own = int(s["which"][i])
        assert all(sigs[k] != sigs[own] for k in range(7) if k != own), (i, own)
        assert runs[6][0].found == 0
        found += runs[own][0].found
    assert found > ps.SEAM_PLANS // 2
    assert np.array_equal(s["image_index"], np.asarray(ps.SEAM_SPECIAL)[s["which"]]) and s["image_index"].max() == ps.SEAM_IMAGES - 1


# ---- the division -------------------------------------------------------------------------------------------------------
def _worst_index(inner, n):
    """k * inner - 1 for the largest k with k * inner - 1 < n: the dividend below n whose quotient is the first to go wrong"""
    return (np.asarray(n, np.int64) // inner) * inner - 1


def _frontier():
    """(W, largest accepted H) for every width that has one: a lower image of the same width has fewer pixels and no longer line"""
    w = np.arange(1, 65537, dtype=np.int64)
    ww = (w + 63) // 64
    h = np.minimum(ps.LDS_BYTES // 8 // ww, ((1 << 24) - 1) // w)
    h_wide = ps.DIV_DOMAIN // (w * w)                            # H <= W: W * H * W <= 2^32
    h_tall = np.floor(np.sqrt(ps.DIV_DOMAIN / w)).astype(np.int64)   # H > W: W * H * H <= 2^32
    h_tall = np.where(w * (h_tall + 1) ** 2 <= ps.DIV_DOMAIN, h_tall + 1, h_tall)
    h_tall = np.where(w * h_tall ** 2 > ps.DIV_DOMAIN, h_tall - 1, h_tall)
    h = np.minimum(h, np.where(h_tall > w, h_tall, np.minimum(h_wide, w)))
    keep = h >= 1
    return w[keep], h[keep]


def test_the_frontier_is_the_acceptance_rule():
    w, h = _frontier()
    assert w[-1] == 65536 and h[-1] == 1                         # 65536 x 1 is the widest image there is
    for k in np.random.default_rng(1).integers(0, len(w), 4000):
        assert ps.accepted(int(w[k]), int(h[k])) and not ps.accepted(int(w[k]), int(h[k]) + 1), (w[k], h[k])
    assert not ps.accepted(65537, 1)


def test_div_small_is_exact_on_every_accepted_shape():
    """For one divisor the multiply-high's excess grows with the dividend, so the quotient goes wrong first at a dividend
    k * inner - 1, and a divisor that is right at the largest such dividend it can meet is right everywhere below.  The
    largest dividend a divisor meets: over all accepted shapes whose longer side is at least the divisor, the most pixels
    -- taken from the frontier (every width with its largest accepted height).  Then, with no such reasoning, every
    divisor at the worst dividend of the frontier's shapes themselves (one in 32, and all from 8000 pixels of width
    up to the bound's corner), and every dividend of the widest shapes for a spread of divisors."""
    w, h = _frontier()
    n, m = w * h, np.maximum(w, h)
    order = np.argsort(m)
    n_from = np.maximum.accumulate(n[order][::-1])[::-1]         # most pixels among the shapes whose longer side is >= m[order][k]
    inner = np.arange(1, 65537, dtype=np.int64)
    n_max = n_from[np.searchsorted(m[order], inner, side="left")]
    i = _worst_index(inner, n_max)
    ok = i >= 0
    assert np.array_equal(ps.div_small(i[ok], inner[ok]), i[ok] // inner[ok])
    assert int((i * inner).max()) < 1 << 32                      # the sufficient condition itself
    # shape by shape
    picks = np.unique(np.concatenate([np.arange(0, len(w), 32), np.nonzero((w >= 8000) & (w <= 8400))[0]]))
    for k in picks:
        inner = np.arange(1, int(m[k]) + 1, dtype=np.int64)
        i = _worst_index(inner, int(n[k]))
        ok = i >= 0
        assert np.array_equal(ps.div_small(i[ok], inner[ok]), i[ok] // inner[ok]), (w[k], h[k])
    for cls in ps.CLASSES + ps.SEAM_CLASSES:
        inner = np.arange(1, max(cls.w, cls.h) + 1, dtype=np.int64)
        i = _worst_index(inner, cls.w * cls.h)
        ok = i >= 0
        assert np.array_equal(ps.div_small(i[ok], inner[ok]), i[ok] // inner[ok]), cls
    # every dividend
    every = np.arange(8192 * 64, dtype=np.int64)
    for inner in [1, 2, 3, 63, 64, 65, 127, 128, 1000, 4095, 4096, 4097, 6553, 8000, 8189, 8190, 8191, 8192]:
        assert np.array_equal(ps.div_small(every, inner), every // inner), inner
    every = np.arange(65536, dtype=np.int64)
    for inner in [2, 255, 32767, 32768, 32769, 65521, 65535, 65536]:
        assert np.array_equal(ps.div_small(every, inner), every // inner), inner


@pytest.mark.parametrize("shape", sorted(COUNTEREXAMPLES), ids=lambda s: "%dx%d" % s)
def test_div_small_is_wrong_on_the_shapes_the_old_limits_let_through(shape):
    """why the refusal exists: one too large, i.e. the pixel one row further down and one column left of the scanned rectangle"""
    w, h = shape
    first_inner, first_i, count = COUNTEREXAMPLES[shape]
    assert (w + 63) // 64 * h * 8 <= ps.LDS_BYTES and w * h < 1 << 24 and not ps.accepted(w, h)
    inner = np.arange(1, max(w, h) + 1, dtype=np.int64)
    i = _worst_index(inner, w * h)
    wrong = ps.div_small(i, inner) != i // inner
    assert wrong[first_inner - 1] and int(wrong.sum()) >= 15        # (15, 431 and 2177 line lengths have such an index)
    every = np.arange(w * h, dtype=np.int64)
    got = ps.div_small(every, first_inner)
    bad = np.nonzero(got != every // first_inner)[0]
    assert len(bad) == count and bad[0] == first_i and np.array_equal(got[bad], bad // first_inner + 1)
    assert first_i * first_inner >= 1 << 32


# ---- the refusal ----------------------------------------------------------------------------------------------------------
def _plan_status(afa, w, h, on_device):
    """afe_rappids_plan / afe_rappids_plan_device on one wall image of w x h, one plan, four candidates -> status"""
    import torch
    cfg = afa.planner_default_config(w, h, ps.DEPTH_SCALE, w / 2.0, *ps.RADII)
    img = np.full((1, h, w), ps.SEAM_WALL, np.uint16)
    vel0, zeros, grav = np.array([[0.0], [0.0], [1.0]]), np.zeros((3, 1)), np.array([[0.0], [9.81], [0.0]])
    samples = afa.planner_samples(0, w, h, 4)
    out = (afa.PlanOutput * 1)()
    buf = None
    if not on_device:
        fn, ptr = afa.library().afe_rappids_plan, img.ctypes.data
    elif torch.cuda.is_available():
        buf = afa.DeviceBuffer(img.nbytes)
        fn, ptr = afa.library().afe_rappids_plan_device, buf.ptr
    else:
        fn, ptr = afa.library().afe_rappids_plan_device, C.c_void_p(img.ctypes.data & ~15)      # never dereferenced on the host
    rc = fn(-1, C.byref(cfg), 1, ptr, 1, None, vel0.ctypes.data, zeros.ctypes.data, grav.ctypes.data, None, samples.ctypes.data, 1,
            None, 4, out, None, None)
    if buf is not None:
        buf.close()
    return rc


@pytest.mark.parametrize("on_device", [False, True], ids=["afe_rappids_plan", "afe_rappids_plan_device"])
def test_shapes_past_the_division_bound_are_refused_on_the_host(afa, on_device):
    """Both entries share plan_impl's check.  Without a GPU the status also tells WHERE the refusal happens: an accepted
    shape gets as far as the device picker (AFE_ERR_NO_DEVICE), which comes before every allocation and launch; a refused
    one never does."""
    import torch
    past = sorted(COUNTEREXAMPLES) + [(8320, 63), (8257, 63), (65536, 2), (20000, 24)]
    for w, h in past:
        assert (w + 63) // 64 * h * 8 <= ps.LDS_BYTES and w * h < 1 << 24 and w * h * max(w, h) > ps.DIV_DOMAIN, (w, h)
        assert _plan_status(afa, w, h, on_device) == OUT_OF_RANGE, (w, h)
    if not torch.cuda.is_available():
        for w, h in [(8192, 64), (8256, 63), (65536, 1), (64, 8192), (2048, 256), (201, 151)]:
            assert ps.accepted(w, h) and _plan_status(afa, w, h, on_device) == NO_DEVICE, (w, h)
        for w, h in [(2048, 1536), (1024, 513), (64, 8193)]:                 # the older limits still hold
            assert not ps.accepted(w, h) and _plan_status(afa, w, h, on_device) == OUT_OF_RANGE, (w, h)
