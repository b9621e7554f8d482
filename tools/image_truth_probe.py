"""What the planner's own self-evaluation (image ground truth and conservativeness tally, csrc/afe_truth.hip) costs on
the device, and what the pixel rectangle saves:

    python tools/image_truth_probe.py            -> profiles/image_truth_probe.json

The parent never opens the GPU: the measurement runs in one child under `timeout -k 10`.  Synthetic 320 x 240 depth
images (scenarios.synthetic_depth_image, 64 of them shared through image_index), the reference vehicle's radii, 256
candidates per planner, timestep 0.1; medians over repetitions after a warm-up:
  (1) afe_image_truth_plans on the winners of 65 536 planners: wall and kernel time
  (2) afe_image_truth_candidates for 4 096 planners x 256 candidates: wall and kernel time, and the tally
  (3) pixels tested / width * height * samples from the counting build, on the first 4 096 found plans
  (4) tests/truth_checker.py (numpy, every pixel) on the first 64 of those, for the ratio per path
No target is fixed for any of them.
"""
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PLANS, N_CAND_PLANNERS, M, N_IMAGES = 65536, 4096, 256, 64
N_COUNTED, N_HOST = 4096, 64
REPS = 15


def child():
    import torch  # noqa: F401  (first: see INTEGRATION.md section 5)
    sys.path.insert(0, ROOT)
    afa = importlib.import_module("agri-fly_amd")
    from tests import truth_checker as tc
    cfg = afa.planner_default_config(320, 240, 10.0 / 256.0, 160.0, 0.116, 0.174, 0.5)
    images = np.stack([afa.scenarios.synthetic_depth_image(seed=300 + k, n_trunks=3 + k % 6) for k in range(N_IMAGES)])
    buf = afa.DeviceBuffer(images.nbytes)
    buf.upload(images)
    rng = np.random.default_rng(0)
    n = N_PLANS
    index = rng.integers(0, N_IMAGES, n).astype(np.int32)
    vel0 = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.3, 0.3, n), rng.uniform(0.0, 2.0, n)])
    acc0 = np.zeros((3, n))
    grav = np.tile(np.array([[0.0], [9.81], [0.0]]), (1, n))
    samples = afa.planner_samples(0, 320, 240, M)
    out, flags, plan_ms = afa.rappids_plan(cfg, buf, vel0, acc0, grav, samples, image_index=index, want_flags=True)
    plans = afa.plans_as_array(out).copy()
    found = plans["found"] != 0
    med = lambda v: float(np.median(v))                                                                # noqa: E731

    wall, kern = [], []
    for rep in range(REPS + 2):
        t0 = time.perf_counter()
        rec, n_free, ms = afa.image_truth_plans(cfg, buf, plans, image_index=index)
        if rep >= 2:
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(ms)
    row = dict(n_plans=n, plans_found=int(found.sum()), plan_kernel_ms=plan_ms, truth_plans_ms=med(wall), truth_plans_kernel_ms=med(kern),
               winners_free=int(n_free), winners_out_of_view=int((rec["verdict"] == 1).sum()), winners_occluded=int((rec["verdict"] == 2).sum()),
               samples_per_plan=float(rec["n_samples"][found].mean()) if found.any() else None)

    nc = N_CAND_PLANNERS
    wall, kern = [], []
    for rep in range(5 + 1):
        t0 = time.perf_counter()
        verdict, _, tally, _, ms = afa.image_truth_candidates(cfg, buf, vel0[:, :nc], acc0[:, :nc], samples, flags[:nc], image_index=index[:nc])
        if rep >= 1:
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(ms)
    row.update(n_candidate_planners=nc, n_candidates=M, truth_candidates_ms=med(wall), truth_candidates_kernel_ms=med(kern),
               tally={k: int(tally[k]) for k in tally.dtype.names},
               candidate_verdicts=[int((verdict == v).sum()) for v in (0, 1, 2)])

    pick = np.nonzero(found)[0][:N_COUNTED]
    tr = np.stack([np.zeros(pick.size), plans["tf"][pick]])
    st, _ = afa.image_truth_paths(cfg, buf, plans["coeffs"][pick], tr, image_index=index[pick], want_stats=True)
    row.update(counted_paths=int(pick.size), counters=st,
               pixels_tested_over_brute_force=st["pixels_tested"] / max(st["pixels_brute_force"], 1))

    few = pick[:N_HOST]
    t0 = time.perf_counter()
    want = tc.judge_batch(cfg, images, plans["coeffs"][few], np.stack([np.zeros(few.size), plans["tf"][few]]), index[few])
    host_ms = (time.perf_counter() - t0) * 1e3
    row.update(host_checker_paths=int(few.size), host_checker_ms=host_ms, host_checker_agrees=not tc.records_equal(rec[few], want),
               host_checker_ms_per_path=host_ms / max(few.size, 1), device_kernel_ms_per_path=row["truth_plans_kernel_ms"] / n)
    buf.close()
    print("RESULT " + json.dumps(row))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child()
    sys.path.insert(0, ROOT)
    provenance = importlib.import_module("agri-fly_amd.provenance")
    run = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True)
    line = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
    if run.returncode != 0 or not line:
        print("image_truth_probe ended with status %d\n%s" % (run.returncode, run.stderr[-2000:]))
        return 1
    out = dict(kernel_sources=provenance.kernel_source_hashes(("afe_truth.hip", "afe_planner.h")), reps=REPS, result=json.loads(line[0][7:]))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "image_truth_probe.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out["result"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
