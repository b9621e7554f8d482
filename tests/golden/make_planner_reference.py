"""tests/golden/planner_reference.npz: what the REFERENCE's own depth-image planner decided (oracle/_ref/planner_probe:
DepthImagePlanner.cpp, RapidTrajectoryGenerator.cpp and SingleAxisTrajectory.cpp compiled where they lie) on 224 plans --
every candidate's TrajectoryTestResult, the counters, the winner's polynomial, GetPyramids() and the value of
IsCollisionFreeGroundTruth for up to 8 collision-checked candidates per plan.  The fixture holds the requests' scalars and
the recorded answers, NOT the images: those come from the committed generators below (scene_image) and are guarded by a
SHA-256 each.

    python tests/golden/make_planner_reference.py        # needs oracle/_ref/planner_probe (built where the reference is)

Also the loader and the small helpers the two test files share (tests/test_planner_reference.py on the CPU,
tests/test_gpu_planner_reference.py on the device); the tests never run the probe except to check staleness."""
import hashlib
import importlib
import io
import os
import struct
import subprocess
import sys
import threading
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(HERE, "planner_reference.npz")
PROBE = os.path.join(ROOT, "oracle", "_ref", "planner_probe")

MAGIC = 0x31505041
# Rappids_Simulator geometry: MINIQUAD arm 0.058 -> radii 0.116 / 0.174, 0.5 m (main.cpp:166-169); 8-bit DepthVis counts
DEPTH_SCALE, TRUE_RADIUS, PLANNING_RADIUS, MIN_CHECKING_DIST = 10.0 / 256.0, 0.116, 0.174, 0.5
N_CANDIDATES, PLANS_PER_SCENE, MAX_TRUTH = 128, 8, 8
FREE_LIMIT = 100            # "no limit" for these scenes (no plan comes near it); above 64, so the device keeps the list in memory
MOUNT = (0.5, -0.5, 0.5, -0.5)   # depthCamAtt, Rotationd::FromEulerYPR(-90 deg, 0, -90 deg), main.cpp:123-125
GRAV = (0.0, 9.81, 0.0)     # camera y points down
ORCHARD = dict(rows=4, cols=5, seed=11)
# (x, y, z, yaw): between the rows looking along them, at canopy height inside a row, low among the trunks, and nose to a canopy
ORCHARD_POSES = [(-4.0, 2.0, 1.2, 0.0), (1.5, 6.2, 2.6, 0.35), (5.0, -3.0, 0.9, 1.45), (2.2, 4.1, 2.4, 0.0)]


def scenes():
    """the scene list: name, kind, image size, pyramid limit, and what scene_image needs"""
    out = []
    for k in range(12):
        out.append(dict(name="synthetic%02d" % k, kind="synthetic", size=(320, 240), limit=FREE_LIMIT,
                        args=dict(seed=900 + k, n_trunks=2 + k % 7, ground_height_m=round(1.0 + 0.6 * k / 11.0, 3))))
    for k, pose in enumerate(ORCHARD_POSES):
        out.append(dict(name="orchard%d" % k, kind="orchard", size=(320, 240), limit=FREE_LIMIT, args=dict(pose=pose)))
    for w, h in ((200, 150), (136, 100), (384, 200)):
        for k in range(2):
            out.append(dict(name="synthetic_%dx%d_%d" % (w, h, k), kind="synthetic", size=(w, h), limit=FREE_LIMIT,
                            args=dict(seed=500 + 10 * k + w, n_trunks=3 + 3 * k, ground_height_m=1.5 - 0.3 * k)))
    for k in range(2):
        out.append(dict(name="blocks%d" % k, kind="blocks", size=(320, 240), limit=FREE_LIMIT, args=dict(seed=40 + k, n_blocks=14 + 10 * k)))
    # (with the plans of scene 20 this one reaches the bottom-side scan's "shrink the right edge" line, which no other scene does)
    out.append(dict(name="ceiling", kind="ceiling", size=(320, 240), limit=FREE_LIMIT, requests=20,
                    args=dict(seed=910, n_trunks=8, ground_height_m=1.5)))
    out.append(dict(name="wall30", kind="wall", size=(320, 240), limit=FREE_LIMIT, args=dict(count=30)))
    for limit in (1, 2):
        out.append(dict(name="limit%d" % limit, kind="synthetic", size=(320, 240), limit=limit,
                        args=dict(seed=3, n_trunks=6, ground_height_m=1.5)))
    return out


_orchard_tris = []


def scene_image(scene):
    """the scene's depth image, uint16 [h, w], from the committed generators (CPU only)"""
    afa = importlib.import_module("agri-fly_amd")
    w, h = scene["size"]
    if scene["kind"] == "synthetic":
        return afa.scenarios.synthetic_depth_image(width=w, height=h, **scene["args"])
    if scene["kind"] == "ceiling":
        # a synthetic scene upside down: the plane is overhead, so what the top-side scans of InflatePyramid meet under a
        # ground plane the bottom-side scans meet here
        return np.ascontiguousarray(np.flipud(afa.scenarios.synthetic_depth_image(width=w, height=h, **scene["args"])))
    if scene["kind"] == "blocks":
        # rectangles at 2.3 to 8 m hanging anywhere in front of an empty background: obstacles beside, above and below a
        # pyramid on one side only, which trunks (full height) and a ground plane (full width) never give
        rng = np.random.Generator(np.random.PCG64(scene["args"]["seed"]))
        img = np.full((h, w), 255, np.uint16)
        for _ in range(scene["args"]["n_blocks"]):
            bw, bh = int(rng.integers(4, 50)), int(rng.integers(4, 50))
            x, y = int(rng.integers(0, w - bw)), int(rng.integers(0, h - bh))
            count = int(rng.integers(60, 205))
            img[y:y + bh, x:x + bw] = np.minimum(img[y:y + bh, x:x + bw], count)
        return img
    if scene["kind"] == "wall":
        return np.full((h, w), scene["args"]["count"], np.uint16)
    from oracle import oracle_py as ora
    if not _orchard_tris:
        _orchard_tris.append(afa.scenarios.orchard_mesh(**ORCHARD))
    x, y, z, yaw = scene["args"]["pose"]
    att = [np.cos(yaw / 2), 0.0, 0.0, np.sin(yaw / 2)]
    return ora.render_depth(ora.render_camera(w, h), _orchard_tris[0], [x, y, z], att, MOUNT)


def image_sha256(img):
    return hashlib.sha256(np.ascontiguousarray(img, dtype="<u2").tobytes()).hexdigest()


def plan_requests(scene_index):
    """the 8 plans of a scene: seed, cost type and vector, vel0, acc0 (camera frame).  vel0.z runs from -0.2 to 3; odd
    plans start with an acceleration; three per scene are hard on purpose -- a downward acceleration that leaves about the
    minimum thrust of 5 m/s^2 at t = 0 (candidates fail the thrust test), a forward acceleration at 4.8 to 4.94 m/s (candidates
    reach the 5 m/s of the velocity test), and a hard sideways one (thrust high / body rates)"""
    rng = np.random.Generator(np.random.PCG64(20261019 + scene_index))
    vz = np.linspace(-0.2, 3.0, PLANS_PER_SCENE)
    plans = []
    for k in range(PLANS_PER_SCENE):
        vel0 = [float(rng.normal(0, 0.5)), float(rng.normal(0, 0.3)), float(vz[(k + scene_index) % PLANS_PER_SCENE])]
        acc0 = [float(a) for a in rng.normal(0, 1.0, 3)] if k % 2 else [0.0, 0.0, 0.0]
        hard = (k - scene_index) % PLANS_PER_SCENE
        if hard == 0:
            acc0 = [0.0, 4.7 + 0.02 * (scene_index % 8), 0.0]
        elif hard == 3:
            vel0[2], acc0 = 4.8 + 0.02 * (scene_index % 8), [0.0, 0.0, 2.0]
        elif hard == 5:
            acc0 = [9.0, -2.0, 0.0]
        cost_type = (k + scene_index // 2) % 2
        if cost_type == 0:
            cost_vec = [float(rng.normal(0, 0.5)), float(rng.normal(0, 0.3)), 1.0]
        else:
            cost_vec = [float(rng.uniform(-20, 20)), float(rng.uniform(-3, 3)), 60.0 * (1 + k % 2)]
        plans.append(dict(seed=(k + scene_index) % 4, cost_type=cost_type, cost_vec=cost_vec, vel0=vel0, acc0=acc0, grav=list(GRAV)))
    return plans


# ---- the probe's request and answer -----------------------------------------------------------------------------------
def encode_request(img, limit, plans, truth_index):
    h, w = img.shape
    b = struct.pack("<4i7d", MAGIC, w, h, len(plans), DEPTH_SCALE, w / 2.0, w / 2.0, h / 2.0, TRUE_RADIUS, PLANNING_RADIUS, MIN_CHECKING_DIST)
    b += np.ascontiguousarray(img, dtype="<u2").tobytes()
    for p, ti in zip(plans, truth_index):
        b += struct.pack("<5i12d", limit, p["seed"], p["cost_type"], N_CANDIDATES, len(ti), *p["vel0"], *p["acc0"], *p["grav"], *p["cost_vec"])
        b += np.asarray(ti, "<i4").tobytes()
    return b


def decode_answer(b):
    off = [0]

    def take(fmt):
        v = struct.unpack_from("<" + fmt, b, off[0])
        off[0] += struct.calcsize("<" + fmt)
        return v

    magic, n = take("2i")
    assert magic == MAGIC
    out = []
    for _ in range(n):
        found, last_free, m = take("3i")
        flags = np.frombuffer(b, np.uint8, m, off[0]).copy()
        off[0] += m
        counters = take("6i")
        win = take("19d")
        pyr = np.zeros(counters[5], PYRAMID_DTYPE)
        for k in range(counters[5]):
            rec = take("d4i12d")
            pyr[k] = (rec[0], rec[1], rec[2], rec[3], rec[4], np.asarray(rec[5:]).reshape(4, 3))
        (nt,) = take("i")
        free = np.frombuffer(b, np.uint8, nt, off[0]).copy()
        off[0] += nt
        out.append(dict(found=found, last_free=last_free, flags=flags, counters=np.asarray(counters, np.int32),
                        coeffs=np.asarray(win[:18]).reshape(6, 3), tf=win[18], pyramids=pyr, truth_free=free))
    assert off[0] == len(b)
    return out


PYRAMID_DTYPE = np.dtype([("depth", "<f8"), ("right", "<i4"), ("top", "<i4"), ("left", "<i4"), ("bottom", "<i4"), ("normal", "<f8", (4, 3))])


def run_probe(probe, request):
    """the probe twice on the same request: the bytes must be identical"""
    runs = [subprocess.Popen([probe], stdin=subprocess.PIPE, stdout=subprocess.PIPE) for _ in range(2)]
    out = [None, None]

    def talk(i):
        out[i] = runs[i].communicate(request)[0]
    threads = [threading.Thread(target=talk, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(r.returncode == 0 for r in runs), [r.returncode for r in runs]
    assert out[0] == out[1], "the probe gave different bytes on the same request"
    return decode_answer(out[0])


def choose_truth(flags, last_free):
    """up to 8 of the candidates the planner collision-checked (bit 4), the winner always among them, then in index order"""
    checked = [int(i) for i in np.flatnonzero(flags & 4)]
    pick = ([last_free] if last_free >= 0 else []) + [i for i in checked if i != last_free]
    return sorted(pick[:MAX_TRUTH])


def reference_tally(flags, index, free):
    """MeasureConservativeness' comparison over a plan whose checked candidates were ALL recorded, from the reference's flags and
    the reference's booleans: n_checked, n_planner_free, n_correct_in_collision, n_incorrect_in_collision, n_free_but_not_free
    (the reference's bool does not say whether a path it refuses left the view or was occluded)"""
    fl = flags[index]
    pfree, tfree = (fl & 8) != 0, free != 0
    return [len(index), int(pfree.sum()), int((~pfree & ~tfree).sum()), int((~pfree & tfree).sum()), int((pfree & ~tfree).sum())]


def make_planner_reference(probe=PROBE, verbose=False):
    sc = scenes()
    cols = {k: [] for k in ("plan_scene", "max_pyramids", "seed", "cost_type", "cost_vec", "vel0", "acc0", "grav", "found", "last_free",
                            "flags", "counters", "coeffs", "tf", "truth_full", "tally")}
    pyr, pyr_count, truth_index, truth_free, truth_count, shas = [], [], [], [], [], []
    for si, s in enumerate(sc):
        img = scene_image(s)
        shas.append(image_sha256(img))
        plans = plan_requests(s.get("requests", si))
        first = run_probe(probe, encode_request(img, s["limit"], plans, [[] for _ in plans]))
        want = [choose_truth(a["flags"], a["last_free"]) for a in first]
        ans = run_probe(probe, encode_request(img, s["limit"], plans, want))
        for p, a, b, ti in zip(plans, ans, first, want):
            assert all(np.array_equal(a[k], b[k]) for k in ("flags", "counters", "coeffs", "pyramids")) and a["found"] == b["found"]
            cols["plan_scene"].append(si)
            cols["max_pyramids"].append(s["limit"])
            for k in ("seed", "cost_type", "cost_vec", "vel0", "acc0", "grav"):
                cols[k].append(p[k])
            for k in ("found", "last_free", "flags", "counters", "coeffs", "tf"):
                cols[k].append(a[k])
            pyr.append(a["pyramids"])
            pyr_count.append(len(a["pyramids"]))
            ti = np.asarray(ti, np.int32)
            truth_index.append(ti)
            truth_free.append(a["truth_free"])
            truth_count.append(len(ti))
            full = len(ti) == int(((a["flags"] & 4) != 0).sum())
            cols["truth_full"].append(full)
            cols["tally"].append(reference_tally(a["flags"], ti, a["truth_free"]) if full else [-1] * 5)
        if verbose:
            print("%-22s limit %3d: found %d/8, pyramids %s, truth %d paths (%d free)" % (
                s["name"], s["limit"], sum(a["found"] for a in ans), [len(a["pyramids"]) for a in ans],
                sum(len(t) for t in want), sum(int(a["truth_free"].sum()) for a in ans)), flush=True)
    pyr = np.concatenate(pyr)
    pyr_offset = np.concatenate([[0], np.cumsum(pyr_count)]).astype(np.int32)
    fx = dict(
        depth_scale=np.float64(DEPTH_SCALE), true_radius=np.float64(TRUE_RADIUS), planning_radius=np.float64(PLANNING_RADIUS),
        min_checking_dist=np.float64(MIN_CHECKING_DIST), n_candidates=np.int32(N_CANDIDATES),
        scene_name=np.array([s["name"] for s in sc]), scene_size=np.array([s["size"] for s in sc], np.int32), image_sha256=np.array(shas),
        plan_scene=np.array(cols["plan_scene"], np.int32), max_pyramids=np.array(cols["max_pyramids"], np.int32),
        seed=np.array(cols["seed"], np.int32), cost_type=np.array(cols["cost_type"], np.int32), cost_vec=np.array(cols["cost_vec"], np.float64),
        vel0=np.array(cols["vel0"], np.float64), acc0=np.array(cols["acc0"], np.float64), grav=np.array(cols["grav"], np.float64),
        found=np.array(cols["found"], np.int32), last_free=np.array(cols["last_free"], np.int32), flags=np.stack(cols["flags"]),
        counters=np.stack(cols["counters"]), coeffs=np.stack(cols["coeffs"]), tf=np.array(cols["tf"], np.float64),
        pyr_offset=pyr_offset, pyr_depth=pyr["depth"].copy(),
        pyr_bounds=np.stack([pyr["right"], pyr["top"], pyr["left"], pyr["bottom"]], 1).astype(np.int32),
        pyr_normals=pyr["normal"].copy(),
        truth_offset=np.concatenate([[0], np.cumsum(truth_count)]).astype(np.int32), truth_index=np.concatenate(truth_index),
        truth_free=np.concatenate(truth_free), truth_full=np.array(cols["truth_full"], bool), tally=np.array(cols["tally"], np.int32))
    check_coverage(fx)
    return fx


def check_coverage(fx):
    """what the fixture must hold before it is committed"""
    fl, npyr = fx["flags"], np.diff(fx["pyr_offset"])
    assert set(np.unique(fl)) == {0, 1, 3, 7, 15}, np.unique(fl)
    assert (npyr >= 3).sum() >= 30 and npyr.max() >= 20, (int((npyr >= 3).sum()), int(npyr.max()))
    assert npyr.max() < 64                                          # both of the device's pyramid-list paths can run every FREE_LIMIT plan
    assert np.any(npyr == fx["max_pyramids"])                       # a plan reaches its limit
    orchard = np.isin(fx["plan_scene"], [i for i, n in enumerate(fx["scene_name"]) if str(n).startswith("orchard")])
    assert np.any(orchard & (fx["found"] == 0)) and np.any(orchard & (npyr >= 20))
    wall = fx["plan_scene"] == list(fx["scene_name"]).index("wall30")
    assert not fx["found"][wall].any()
    assert len(fx["truth_free"]) >= 200 and fx["truth_free"].sum() >= 20
    assert {0, 1} == set(np.unique(fx["cost_type"])) and set(np.unique(fx["seed"])) == {0, 1, 2, 3}
    assert fx["truth_full"].sum() >= 20


def check_truth_kinds(fx):
    """the recorded ground-truth paths hold at least 20 free ones and at least 20 of each of the checker's two kinds of
    refusal (out of view, occluded); run by the generator before the fixture is written (a minute of numpy)"""
    from oracle import oracle_py as ora
    from tests import truth_checker as tc
    images = checked_images(fx)
    kinds = np.zeros(3, int)
    for s in range(len(images)):
        cfg = oracle_config(ora, fx, s)
        rays = tc.ImageRays(cfg, images[s])
        for p in np.flatnonzero(fx["plan_scene"] == s):
            samples = ora.planner_samples(int(fx["seed"][p]), cfg.width, cfg.height, int(fx["n_candidates"]))
            for j in range(fx["truth_offset"][p], fx["truth_offset"][p + 1]):
                k = fx["truth_index"][j]
                v = tc.judge(rays, candidate_coeffs(ora, cfg, fx["vel0"][p], fx["acc0"][p], samples[k]), 0.0, samples[k][3])["verdict"]
                assert (v == 0) == bool(fx["truth_free"][j]), (s, p, k, v)
                kinds[v] += 1
    print("ground-truth paths: %d free, %d out of view, %d occluded" % tuple(kinds))
    assert kinds.min() >= 20, kinds


def write_fixture(fx, path=FIXTURE):
    """an .npz whose bytes depend on its arrays alone (np.savez stamps the time of day into the archive)"""
    with zipfile.ZipFile(path, "w") as z:
        for name in sorted(fx):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(fx[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


# ---- shared by the tests ----------------------------------------------------------------------------------------------
def load_fixture(path=FIXTURE):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def checked_images(fx):
    """every scene's image from the generators, each held to its recorded SHA-256"""
    out = []
    for i, s in enumerate(scenes()):
        assert s["name"] == str(fx["scene_name"][i]) and tuple(s["size"]) == tuple(fx["scene_size"][i])
        img = scene_image(s)
        assert image_sha256(img) == str(fx["image_sha256"][i]), "the generator of scene %s no longer gives the recorded image" % s["name"]
        out.append(img)
    return out


def oracle_config(ora, fx, scene, plan=None):
    """the checker's configuration of a scene (and, with a plan index, that plan's limit and cost)"""
    w, h = (int(v) for v in fx["scene_size"][scene])
    c = ora.planner_config(w, h, float(fx["depth_scale"]), w / 2.0, float(fx["true_radius"]), float(fx["planning_radius"]),
                           float(fx["min_checking_dist"]))
    if plan is not None:
        c.max_pyramids = int(fx["max_pyramids"][plan])
        c.cost_type = int(fx["cost_type"][plan])
        for k in range(3):
            c.cost_vec[k] = fx["cost_vec"][plan, k]
    return c


def candidate_coeffs(ora, cfg, vel0, acc0, sample):
    """CommonMath::Trajectory of one candidate (RapidTrajectoryGenerator::GetTrajectory, RTG.hpp:232-241) from the parts of
    the checker that are pinned to the reference bit for bit (ora_axis_generate: planner_math_kat.json): [6, 3], t^5 .. t^0"""
    import ctypes as C
    x, y, depth, tf = (float(v) for v in sample)
    goal = [depth * ((x - cfg.cx) / cfg.focal_length), depth * ((y - cfg.cy) / cfg.focal_length), depth * 1]
    co = np.zeros((6, 3))
    for i in range(3):
        ax = ora.OraAxis()
        ax.p0, ax.v0, ax.a0, ax.pf, ax.vf, ax.af = 0.0, float(vel0[i]), float(acc0[i]), goal[i], 0.0, 0.0
        ora.planner_lib().ora_axis_generate(C.byref(ax), tf)
        co[:, i] = [ax.a / 120, ax.b / 24, ax.g / 6, ax.a0 / 2, ax.v0, ax.p0]
    return co


if __name__ == "__main__":
    if not os.path.exists(PROBE):
        sys.exit("oracle/_ref/planner_probe is not built (make -C oracle ref, where the reference sources are present)")
    fixture = make_planner_reference(verbose=True)
    check_truth_kinds(fixture)
    write_fixture(fixture)
    print("written", FIXTURE, os.path.getsize(FIXTURE), "bytes")
