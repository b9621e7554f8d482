"""The planner's image-shape matrix (test infrastructure, no GPU).

Which code runs in agri-fly_amd/csrc/afe_planner.hip and afe_planner_api.cpp is chosen by the image shape.  `paths_of`
restates those dispatch conditions (with the source lines they come from); CLASSES names the smallest shapes that reach
every value of every row, with the value each is expected to take; `inputs` / `oracle_refs` build one seeded set of
images, states and candidates per class (after tests/test_gpu_planner.py::test_image_sizes_off_the_fast_path) and the
oracle's answers on it, computed once per process and shared by the CPU and the GPU tests.

tests/test_planner_shapes_cpu.py proves the matrix complete and the inputs non-trivial without the engine;
tests/test_gpu_planner_shapes.py flies every class on the device."""
import functools

import numpy as np

from tests.scenarios import afa

DEPTH_SCALE = 10.0 / 256.0
RADII = (0.116, 0.174, 0.5)          # true radius, planning radius, minimum checking distance (the reference vehicle's)
N_PLANS, N_CANDIDATES, N_IMAGES = 24, 96, 3
IMAGE_SEED0, SAMPLES_SEED = 500, 3   # image k: synthetic_depth_image(seed=IMAGE_SEED0 + k, n_trunks=3 + k)
LDS_BYTES = 65536                    # dynamic LDS of the search kernel: the bit image (and the summaries' list behind it)
DIV_DOMAIN = 1 << 32                 # width * height * max(width, height) <= 2^32: the scans' division (div_small) is exact
GRID_Z = 65535                       # images per launch of afe_prepare_images_kernel (launch_rappids)

# row -> every value the row can take
PATH_VALUES = {
    "prepare": ("dword", "pixel"),
    "bit_image": ("summaries", "whole_words", "partial_word"),
    "max_depth": ("vector16", "generic"),
    "transpose": ("unpadded", "padded"),
    "mask_divide": ("inner_one", "multiply_high"),
    "width_mod_8": ("zero", "nonzero"),
    "height": ("even", "odd"),
    "prepare_launches": ("one", "two"),
}


def accepted(w, h):
    """the image-size checks of plan_impl (afe_planner_api.cpp:104-112)"""
    return (w + 63) // 64 * h * 8 <= LDS_BYTES and w * h < (1 << 24) and w * h * max(w, h) <= DIV_DOMAIN


def paths_of(w, h, n_images=N_IMAGES):
    """Which path an accepted w x h image takes, row by row (release library, no lab variable)."""
    ww = (w + 63) // 64
    return {
        # afe_prepare_images_kernel (afe_planner.hip:1460): `even = ((W | H) & 1) == 0` -- two pixels per dword, else one by one
        "prepare": "dword" if (w | h) & 1 == 0 else "pixel",
        # afe_planner_api.cpp:152 `whole_words`: rows of whole 64-pixel words and 512 B of LDS left behind the bit image ->
        # build_mask_sum (afe_planner.hip:458); else build_mask (:366), whose `x < W` test cuts a row's last word when W % 64 != 0
        "bit_image": ("summaries" if ((w * h) >> 6) * 8 + 512 <= LDS_BYTES else "whole_words") if w % 64 == 0 else "partial_word",
        # inflate_pyramid's maxDepth sweep (afe_planner.hip:920): `(W & 63) == 0` -> 16-byte vectors, else pixel by pixel (:969)
        "max_depth": "vector16" if w % 64 == 0 else "generic",
        # afe_planner_api.cpp:160 `height_t = (height + 63) / 64 * 64`: the transposed image's column length HT
        "transpose": "unpadded" if h % 64 == 0 else "padded",
        # div_small (afe_planner.hip:355) `inner == 1 ? i : umulhi`: build_mask / build_mask_sum divide by WW = ceil(W / 64)
        "mask_divide": "inner_one" if ww == 1 else "multiply_high",
        # a row of W % 8 != 0 pixels starts rows (and device-resident images) off every 16-byte boundary
        "width_mod_8": "zero" if w % 8 == 0 else "nonzero",
        # an odd H: the transposed image's columns have no whole number of dwords
        "height": "even" if h % 2 == 0 else "odd",
        # launch_rappids (afe_planner.hip:1520): grid.z <= 65535, one launch of the prepare kernel per run of that many images
        "prepare_launches": "one" if n_images <= GRID_Z else "two",
    }


class ShapeClass:
    def __init__(self, name, w, h, why, focal=None, n_images=N_IMAGES, **paths):
        self.name, self.w, self.h, self.why, self.n_images = name, w, h, why, n_images
        self.focal = w / 2.0 if focal is None else float(focal)        # main.cpp:360: focal = width / 2
        self.paths = paths

    def __repr__(self):
        return self.name


def _c(w, h, why, prepare, bit_image, max_depth, transpose, mask_divide, width_mod_8, height, focal=None, n_images=N_IMAGES, name=None):
    return ShapeClass(name or "%dx%d" % (w, h), w, h, why, focal=focal, n_images=n_images, prepare=prepare, bit_image=bit_image,
                      max_depth=max_depth, transpose=transpose, mask_divide=mask_divide, width_mod_8=width_mod_8, height=height,
                      prepare_launches="one" if n_images <= GRID_Z else "two")


# The image classes: every one is flown on host images against the oracle (tests/test_gpu_planner_shapes.py).
CLASSES = [
    _c(201, 151, "odd x odd", "pixel", "partial_word", "generic", "padded", "multiply_high", "nonzero", "odd"),
    _c(202, 151, "W even, H odd", "pixel", "partial_word", "generic", "padded", "multiply_high", "nonzero", "odd"),
    _c(202, 150, "even, W % 8 != 0", "dword", "partial_word", "generic", "padded", "multiply_high", "nonzero", "even"),
    _c(64, 48, "one word per row, summaries", "dword", "summaries", "vector16", "padded", "inner_one", "zero", "even"),
    _c(65, 49, "the second word of a row holds one pixel", "pixel", "partial_word", "generic", "padded", "multiply_high", "nonzero", "odd"),
    _c(40, 30, "one partial word per row", "dword", "partial_word", "generic", "padded", "inner_one", "zero", "even"),
    _c(128, 64, "H % 64 == 0: the transposed image is not padded", "dword", "summaries", "vector16", "unpadded", "multiply_high", "zero", "even"),
    _c(129, 65, "HT = 128", "pixel", "partial_word", "generic", "padded", "multiply_high", "nonzero", "odd"),
    _c(48, 400, "tall", "dword", "partial_word", "generic", "padded", "inner_one", "zero", "even"),
    _c(832, 628, "whole words, too large for the summaries' list", "dword", "whole_words", "vector16", "padded", "multiply_high", "zero", "even"),
    _c(1024, 512, "the LDS bit image is exactly 65 536 bytes", "dword", "whole_words", "vector16", "unpadded", "multiply_high", "zero", "even"),
    # the widest image the division bound admits: 8192 * 64 * 8192 = 2^32 exactly (and 128 words x 64 rows = 65 536 bytes
    # of LDS).  With focal = W / 2 a 64-row image is a slit 0.9 degrees high in which the vehicle never fits (the oracle
    # finds no plan from 128 pixels up); at 80 pixels every plan grows one pyramid thousands of pixels wide -- the
    # longest lines the scans ever divide by -- and 19 of the 24 find a trajectory.
    _c(8192, 64, "at the division bound: W * H * W = 2^32", "dword", "whole_words", "vector16", "unpadded", "multiply_high", "zero", "even", focal=80.0),
    # a quarter of the bound, the shape with several pyramids per plan (focal 128: 109 pyramids in 24 plans)
    _c(2048, 256, "wide, several pyramids per plan", "dword", "whole_words", "vector16", "unpadded", "multiply_high", "zero", "even", focal=128.0),
]
# the production shape, for the comparison of the summaries with the plain sweep
EXTRA_CLASSES = [_c(320, 240, "the flagship camera", "dword", "summaries", "vector16", "padded", "multiply_high", "zero", "even")]
BY_NAME = {c.name: c for c in CLASSES + EXTRA_CLASSES}

# The launch seam: 65 537 images, the last two of them in the second run of prepare launches.
SEAM_IMAGES = 65537
SEAM_SPECIAL = (0, 1, 65533, 65534, 65535, 65536)      # distinct synthetic images; every other image is the wall
SEAM_WALL = 30                                          # counts: 1.17 m, nothing passes
SEAM_PLANS = 32
SEAM_CLASSES = [
    _c(64, 64, "seam, summaries", "dword", "summaries", "vector16", "unpadded", "inner_one", "zero", "even", n_images=SEAM_IMAGES, name="seam64x64"),
    _c(40, 30, "seam, no summaries", "dword", "partial_word", "generic", "padded", "inner_one", "zero", "even", n_images=SEAM_IMAGES, name="seam40x30"),
]

# The shapes the summaries are judged on against the plain sweep (lab variable AFE_PLANNER_NO_SUMS on the -DAFE_DEV_HOOKS build)
NO_SUMS_SHAPES = [(64, 48), (128, 64), (320, 240)]
NO_SUMS_CLASSES = ["%dx%d" % s for s in NO_SUMS_SHAPES]
# ... and the classes whose plans are also made from device-resident images
DEVICE_RESIDENT = ["201x151", "202x150", "64x48"]


def oracle_config(ora, cls, max_pyramids=64):
    ocfg = ora.planner_config(cls.w, cls.h, DEPTH_SCALE, cls.focal, *RADII)
    ocfg.max_pyramids = max_pyramids
    ocfg.cost_type = 1
    ocfg.cost_vec[0], ocfg.cost_vec[1], ocfg.cost_vec[2] = 0.0, 0.0, 120.0
    return ocfg


def engine_config(cls, max_pyramids=64):
    c = afa.planner_default_config(cls.w, cls.h, DEPTH_SCALE, cls.focal, *RADII)
    c.max_pyramids = max_pyramids
    c.cost_type = 1
    c.cost_vec[0], c.cost_vec[1], c.cost_vec[2] = 0.0, 0.0, 120.0
    return c


def states(seed, n):
    """vel0, acc0, grav [3, n] in the camera frame (y down), as test_image_sizes_off_the_fast_path draws them"""
    rng = np.random.default_rng(seed)
    image_index = rng.integers(0, N_IMAGES, n).astype(np.int32)
    vel0 = np.stack([rng.normal(0, 0.4, n), rng.normal(0, 0.2, n), rng.uniform(0, 2.0, n)])
    acc0 = rng.normal(0, 0.3, (3, n))
    grav = np.tile(np.array([[0.0], [9.81], [0.0]]), (1, n))
    return image_index, vel0, acc0, grav


def synthetic_images(cls, seeds, trunks, **kw):
    return np.stack([afa.scenarios.synthetic_depth_image(width=cls.w, height=cls.h, seed=s, n_trunks=t, focal_length=cls.focal,
                                                         **{k: v[j] if isinstance(v, list) else v for k, v in kw.items()})
                     for j, (s, t) in enumerate(zip(seeds, trunks))])


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The class's images [3, H, W], image_index [24], states and candidates [96, 4]; the generator's seed is the width.
    Shared: do not modify."""
    cls = BY_NAME[name]
    images = synthetic_images(cls, [IMAGE_SEED0 + k for k in range(N_IMAGES)], [3 + k for k in range(N_IMAGES)])
    image_index, vel0, acc0, grav = states(cls.w, N_PLANS)
    samples = afa.planner_samples(SAMPLES_SEED, cls.w, cls.h, N_CANDIDATES)
    out = dict(images=images, image_index=image_index, vel0=vel0, acc0=acc0, grav=grav, samples=samples)
    for v in out.values():
        v.setflags(write=False)
    return out


def run_oracle(ora, ocfg, images, image_index, vel0, acc0, grav, samples):
    return [ora.planner_run(ocfg, images[image_index[i]], vel0[:, i], acc0[:, i], grav[:, i], samples) for i in range(vel0.shape[1])]


_refs = {}


def oracle_refs(ora, name):
    """[(result, flags)] * 24: the oracle on inputs(name), computed once"""
    if name not in _refs:
        _refs[name] = run_oracle(ora, oracle_config(ora, BY_NAME[name]), **inputs(name))
    return _refs[name]


@functools.lru_cache(maxsize=None)
def seam_inputs(name):
    """The six distinct images [6, H, W] that sit at SEAM_SPECIAL among 65 531 walls, and 32 plans on them
    (image_index holds the positions in the 65 537-image array).  Shared: do not modify."""
    cls = {c.name: c for c in SEAM_CLASSES}[name]
    # near trunks, ever more of them, over a ground that drops from image to image: no two of the six give any of the 32
    # plans the same answer (tests/test_planner_shapes_cpu.py), so an image taken from the wrong index cannot pass
    special = synthetic_images(cls, [700 + k for k in range(6)], [4 + 2 * k for k in range(6)], trunk_range_m=(1.2, 5.0),
                               ground_height_m=[0.6 + 0.25 * k for k in range(6)])
    rng = np.random.default_rng(cls.w + 1000)
    which = np.concatenate([np.arange(6), rng.integers(0, 6, SEAM_PLANS - 6)]).astype(np.int32)     # every special image is planned on
    _, vel0, acc0, grav = states(cls.w + 2000, SEAM_PLANS)
    samples = afa.planner_samples(SAMPLES_SEED, cls.w, cls.h, N_CANDIDATES)
    out = dict(cls=cls, special=special, which=which, image_index=np.asarray(SEAM_SPECIAL, np.int32)[which], vel0=vel0, acc0=acc0,
               grav=grav, samples=samples)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def seam_image_array(name):
    """[65537, H, W]: the wall everywhere but at SEAM_SPECIAL (about 0.5 GB for 64 x 64)"""
    s = seam_inputs(name)
    images = np.full((SEAM_IMAGES, s["cls"].h, s["cls"].w), SEAM_WALL, np.uint16)
    images[list(SEAM_SPECIAL)] = s["special"]
    return images


def signature(res, flags):
    """what _compare holds identical, as bytes"""
    return bytes(flags) + repr((res.found, res.best_index, res.n_cost_checks, res.n_collision_checks, res.n_velocity_checks,
                                res.n_collision_free, res.n_pyramids)).encode()


# ---- div_small (afe_planner.hip:349-357) restated ----------------------------------------------------------------------
def div_small(i, inner):
    """numpy restatement: inner == 1 ? i : umulhi(i, floor(2^32 / inner) + 1), on uint64"""
    i = np.asarray(i, np.uint64)
    inner = np.asarray(inner, np.uint64)
    magic = (np.uint64(1 << 32) // inner + np.uint64(1)) & np.uint64(0xffffffff)
    return np.where(inner == 1, i, (i * magic) >> np.uint64(32))
