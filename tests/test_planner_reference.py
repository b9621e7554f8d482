"""The planner checker (oracle/agrifly_oracle_planner.c) and the image ground-truth checker (tests/truth_checker.py) against
what the REFERENCE's own planner decided: tests/golden/planner_reference.npz is what oracle/_ref/planner_probe recorded --
DepthImagePlanner.cpp, RapidTrajectoryGenerator.cpp and SingleAxisTrajectory.cpp compiled where they lie, against the
declaration-only oracle/eigen_decl and the three-field cv::Mat of oracle/cv_decl -- on 224 plans: synthetic scenes,
rendered orchard views (up to 29 pyramids a plan, plans that find nothing), three image sizes off the fast path, a wall,
pyramid limits 1 and 2, both cost types, states that fail the thrust, rate and velocity tests.  Both sides are double,
-ffp-contract=off, the same libm: everything is compared bit for bit.  CPU only."""
import importlib.util
import os
import re

import numpy as np
import pytest

from tests import truth_checker as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUTH_STRIDE = 7        # every 7th recorded ground-truth path: more than 200 of them


def _generator():
    spec = importlib.util.spec_from_file_location("make_planner_reference", os.path.join(ROOT, "tests", "golden", "make_planner_reference.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ref(ora):
    """the generator module, the fixture and every scene's image (each held to its recorded SHA-256)"""
    mod = _generator()
    fx = mod.load_fixture()
    return mod, fx, mod.checked_images(fx)


@pytest.fixture(scope="module")
def verdicts(ora, ref):
    """truth_checker.judge on the recorded paths both tests below need, once: {path number: verdict}.  Every TRUTH_STRIDE-th
    path, and every path of the plans whose collision-checked candidates were all recorded."""
    mod, fx, images = ref
    off = fx["truth_offset"]
    out = {}
    for s in range(len(images)):
        cfg = mod.oracle_config(ora, fx, s)
        rays = None
        for p in np.flatnonzero(fx["plan_scene"] == s):
            samples = ora.planner_samples(int(fx["seed"][p]), cfg.width, cfg.height, int(fx["n_candidates"]))
            for j in range(off[p], off[p + 1]):
                if j % TRUTH_STRIDE == 0 or fx["truth_full"][p]:
                    rays = rays or tc.ImageRays(cfg, images[s])
                    k = fx["truth_index"][j]
                    co = mod.candidate_coeffs(ora, cfg, fx["vel0"][p], fx["acc0"][p], samples[k])
                    out[j] = tc.judge(rays, co, 0.0, samples[k][3])["verdict"]
    return out


def test_fixture_holds_the_cases(ref):
    mod, fx, _ = ref
    assert len(fx["found"]) == 224 and fx["flags"].shape == (224, 128)
    mod.check_coverage(fx)     # every flag value, >= 30 plans with 3+ pyramids, a view with 20+, limits reached, a wall, both costs
    assert set(map(tuple, fx["scene_size"])) == {(320, 240), (200, 150), (136, 100), (384, 200)}
    assert fx["vel0"][:, 2].min() == -0.2 and fx["vel0"][:, 2].max() > 3 and np.any(fx["acc0"] != 0)
    # the winner is among the recorded ground-truth candidates of every plan that found one
    for p in np.flatnonzero(fx["found"]):
        assert fx["last_free"][p] in fx["truth_index"][fx["truth_offset"][p]:fx["truth_offset"][p + 1]]
    assert os.path.getsize(mod.FIXTURE) <= 256 * 1024


def _same_bits(a, b):
    return np.ascontiguousarray(a, np.float64).tobytes() == np.ascontiguousarray(b, np.float64).tobytes()


def test_checker_plans_like_the_reference_bit_for_bit(ora, ref):
    """ora_planner_run on every plan: FindLowestCostTrajectory's return value, the winner, every candidate's
    TrajectoryTestResult, the five GetNum* counters and GetNumPyramids(), the winner's end time and its 18 coefficients."""
    mod, fx, images = ref
    for p in range(len(fx["found"])):
        s = int(fx["plan_scene"][p])
        cfg = mod.oracle_config(ora, fx, s, p)
        samples = ora.planner_samples(int(fx["seed"][p]), cfg.width, cfg.height, int(fx["n_candidates"]))
        res, flags = ora.planner_run(cfg, images[s], fx["vel0"][p], fx["acc0"][p], fx["grav"][p], samples)
        where = "plan %d (%s)" % (p, fx["scene_name"][s])
        assert (res.found, res.best_index) == (fx["found"][p], fx["last_free"][p]), where
        np.testing.assert_array_equal(flags, fx["flags"][p], err_msg=where)
        assert [res.n_generated, res.n_cost_checks, res.n_collision_checks, res.n_velocity_checks, res.n_collision_free,
                res.n_pyramids] == list(fx["counters"][p]), where
        got = np.array([[res.coeffs[q][a] for a in range(3)] for q in range(6)])
        assert res.tf == fx["tf"][p] and _same_bits(got, fx["coeffs"][p]), where


def test_checker_inflates_the_reference_pyramids(ora, ref):
    """GetPyramids() of every plan: depth and the four pixel bounds exactly, the four normals bit for bit, in the
    reference's order.  Depths are whole counts, so pyramids of EQUAL depth within a plan are common (199 groups in this
    fixture).  The reference does not std::sort its list: it inserts at std::lower_bound on the depth, i.e. in front of its
    equals, which is defined, and the checker does the same -- so the order is held exactly there too."""
    mod, fx, images = ref
    n_ties = total = 0
    for p in range(len(fx["found"])):
        s = int(fx["plan_scene"][p])
        cfg = mod.oracle_config(ora, fx, s, p)
        samples = ora.planner_samples(int(fx["seed"][p]), cfg.width, cfg.height, int(fx["n_candidates"]))
        _, _, pyr = ora.planner_run(cfg, images[s], fx["vel0"][p], fx["acc0"][p], fx["grav"][p], samples, want_pyramids=True)
        a, b = fx["pyr_offset"][p], fx["pyr_offset"][p + 1]
        where = "plan %d (%s)" % (p, fx["scene_name"][s])
        assert len(pyr) == b - a, where
        assert _same_bits(pyr["depth"], fx["pyr_depth"][a:b]), where

        def key(depth, bounds, normals):
            return (np.float64(depth).tobytes(), tuple(int(v) for v in bounds), np.ascontiguousarray(normals).tobytes())
        got = [key(q["depth"], (q["right"], q["top"], q["left"], q["bottom"]), q["normal"]) for q in pyr]
        want = [key(fx["pyr_depth"][j], fx["pyr_bounds"][j], fx["pyr_normals"][j]) for j in range(a, b)]
        assert got == want, (where, [i for i in range(len(got)) if got[i] != want[i]][:4])
        n_ties += len(set(fx["pyr_depth"][a:b].tolist())) < b - a
        total += b - a
    print("pyramids compared: %d, plans that hold pyramids of equal depth: %d" % (total, n_ties))
    assert total > 1000 and n_ties > 20


def test_truth_checker_calls_free_what_the_reference_calls_free(ref, verdicts):
    """tests/truth_checker.judge on every 7th recorded path: verdict 0 exactly where IsCollisionFreeGroundTruth returned
    true.  The reference returns a bool; which refused path left the view (1) and which was occluded (2) stays this
    project's own reading of the function's two loops and is not pinned."""
    _, fx, _ = ref
    picked = [j for j in verdicts if j % TRUTH_STRIDE == 0]
    assert len(picked) >= 200
    assert {verdicts[j] for j in picked} == {0, 1, 2}
    wrong = [j for j in verdicts if (verdicts[j] == 0) != bool(fx["truth_free"][j])]
    assert not wrong, wrong[:10]


def test_tally_is_the_reference_comparison(ref, verdicts):
    """MeasureConservativeness itself collision-checks dynamically infeasible candidates too, so its two counts are not
    tally()'s; what is pinned is the tally the generator formed from the reference's flags and the reference's booleans,
    for the plans whose collision-checked candidates were all recorded."""
    _, fx, _ = ref
    full = np.flatnonzero(fx["truth_full"])
    assert len(full) >= 20
    n_refused = 0
    for p in full:
        v = np.zeros(fx["flags"].shape[1], np.uint8)
        for j in range(fx["truth_offset"][p], fx["truth_offset"][p + 1]):
            v[fx["truth_index"][j]] = verdicts[j]
        t = tc.tally(fx["flags"][p], v)
        assert [t["n_checked"], t["n_planner_free"], t["n_correct_in_collision"], t["n_incorrect_in_collision"],
                t["n_free_but_out_of_view"] + t["n_free_but_occluded"]] == list(fx["tally"][p]), p
        n_refused += t["n_correct_in_collision"]
    assert fx["tally"][full, 4].sum() == 0          # nothing the reference's planner called free was refused by its ground truth
    assert n_refused > 0 and fx["tally"][full, 3].sum() > 0


def test_fixture_is_what_the_probe_writes_now(ref):
    """staleness: the generator run again (needs oracle/_ref/planner_probe, built where the reference is present).  The
    generator runs the probe twice on every request and requires identical bytes."""
    mod, fx, _ = ref
    if not os.path.exists(mod.PROBE):
        pytest.skip("oracle/_ref/planner_probe not built (the reference sources are not on this machine)")
    fresh = mod.make_planner_reference(mod.PROBE)
    assert sorted(fresh) == sorted(fx)
    for k in fx:
        a, b = np.asarray(fresh[k]), fx[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_probe_recipe_uses_the_declaration_only_headers():
    """the probe's include path names oracle/eigen_decl and oracle/cv_decl and never tests/shim, compiles the three
    reference sources where they lie, and the OpenCV stand-in declares three fields and nothing else"""
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        mk = f.read()
    inc = re.search(r"^PLANNER_INC\s*:=(.*)$", mk, re.M).group(1)
    src = re.search(r"^PLANNER_SRC\s*:=((?:.*\\\n)*.*)$", mk, re.M).group(1)
    recipe = re.search(r"^_ref/planner_probe:.*\n((?:\t.*\n)+)", mk, re.M).group(1)
    assert "$(PLANNER_INC)" in recipe and "$(PLANNER_SRC)" in recipe and {"-Ieigen_decl", "-Icv_decl"} <= set(inc.split())
    assert "shim" not in inc and "shim" not in recipe and "shim" not in src
    for flag in ("-ffp-contract=off", "-fno-fast-math", "-include algorithm", "-O2", "-std=c++11"):
        assert flag in recipe
    for name in ("DepthImagePlanner.cpp", "RapidTrajectoryGenerator.cpp", "SingleAxisTrajectory.cpp"):
        assert re.search(r"\$\(REF\)/\S*" + re.escape(name), src)
    assert "_ref/planner_probe" in mk.split("\nref:")[1].split("\n\n")[0]   # built by `make ref`, i.e. by build()
    decl = os.path.join(ROOT, "oracle", "cv_decl", "opencv2")
    code = []
    for path in (os.path.join(decl, "opencv.hpp"), os.path.join(decl, "imgproc", "imgproc.hpp")):
        with open(path) as f:
            code += [l for l in f if l.strip() and not l.lstrip().startswith(("//", "#pragma"))]
    assert code == ["namespace cv { struct Mat { int rows, cols; unsigned char *data; }; }\n", '#include "../opencv.hpp"\n']
