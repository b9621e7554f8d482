// oracle/ref_planner_probe.cpp -- TEST INFRASTRUCTURE.
// What the REFERENCE's own depth-image planner decides, its sources compiled from where they lie (the Makefile names
// them on the compiler's command line; nothing of them is copied here):
//   Components/Components/DepthImagePlanner/DepthImagePlanner.{hpp,cpp}, Pyramid.hpp, MonotonicTrajectory.hpp
//   Components/Components/TrajectoryGenerator/RapidTrajectoryGenerator.{hpp,cpp}, SingleAxisTrajectory.{hpp,cpp}
//   Common/Common/Math/{Vec3,Trajectory,RootFinder}.hpp
// against oracle/eigen_decl (Eigen::Matrix declared, never defined) and oracle/cv_decl (a three-field cv::Mat).
//
// This file's own text is the driver and the two things the reference leaves to its caller:
//   * a candidate generator that hands on DepthImagePlanner::RandomTrajectoryGenerator's candidates and returns -1 after
//     N of them (FindLowestCostTrajectory's contract for a finite generator, DepthImagePlanner.cpp:131-136): a candidate
//     COUNT in place of the wall-clock budget, which is set to 1000 s (int(t * 1e6) overflows past ~2000 s);
//   * the cost function: type 0 is -dir . p(T) / T, type 1 the goal cost -(|goal| - |goal - p(T)|) / T.
//
// usage: planner_probe [request-file] > answer      (request on stdin without an argument; everything little endian)
// request:  int32 magic 0x31505041, width, height, n_plans
//           double depth_scale, focal_length, cx, cy, true_vehicle_radius, planning_vehicle_radius, min_checking_dist
//           uint16 image[height * width]
//           per plan: int32 max_pyramids (SetMaxNumberOfPyramids), seed (SetRandomSeed), cost_type, n_candidates, n_truth
//                     double vel0[3], acc0[3], grav[3], cost_vec[3]
//                     int32 truth_index[n_truth]   candidates to run IsCollisionFreeGroundTruth on
// answer:   int32 magic, n_plans;  per plan:
//           int32 found (the return value), last_free (last candidate whose result has the CollisionFree bit, -1 if none),
//                 n_candidates;  uint8 result[n_candidates] (TrajectoryTestResult)
//           int32 GetNumTrajectoriesGenerated, GetNumCostChecks, GetNumCollisionChecks, GetNumVelocityChecks,
//                 GetNumCollisionFree, GetNumPyramids
//           double coeffs[6][3] (the returned trajectory's GetTrajectory(): t^5 .. t^0), end time   -- zeros if not found
//           per pyramid of GetPyramids(), in its order: double depth; int32 right, top, left, bottom; double normals[4][3]
//           int32 n_truth;  uint8 free[n_truth]   IsCollisionFreeGroundTruth of the requested candidates
// Doubles travel as their eight bytes.  Nothing here reads a clock or an address, so a request always gives the same bytes.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdint.h>
#include <vector>
#include "Components/DepthImagePlanner/DepthImagePlanner.hpp"

using RapidQuadrocopterTrajectoryGenerator::RapidTrajectoryGenerator;
using RectangularPyramidPlanner::DepthImagePlanner;
using RectangularPyramidPlanner::Pyramid;
using RectangularPyramidPlanner::TrajectoryTest;

static const int32_t MAGIC = 0x31505041;

// hands on the reference generator's candidates, N of them
struct CountedGenerator {
  DepthImagePlanner::RandomTrajectoryGenerator *gen;
  int left;
  static int Next(void *self, RapidTrajectoryGenerator &nextTraj) {
    CountedGenerator *g = (CountedGenerator *) self;
    if (g->left <= 0) return -1;
    g->left--;
    return g->gen->GetNextCandidateTrajectory(nextTraj);
  }
};

struct Cost {
  int type;
  double v[3];
  static double Get(void *self, RapidTrajectoryGenerator &traj) {
    const Cost *c = (const Cost *) self;
    const double dur = traj.GetFinalTime();
    const Vec3d e = traj.GetPosition(dur);
    const double ex = e.x, ey = e.y, ez = e.z;
    if (c->type == 0) return -(c->v[0] * ex + c->v[1] * ey + c->v[2] * ez) / dur;
    const double gx = c->v[0], gy = c->v[1], gz = c->v[2];
    const double SG = sqrt((gx - 0) * (gx - 0) + (gy - 0) * (gy - 0) + (gz - 0) * (gz - 0));
    const double PiG = sqrt((gx - ex) * (gx - ex) + (gy - ey) * (gy - ey) + (gz - ez) * (gz - ez));
    return -(SG - PiG) / dur;
  }
};

static bool rd(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }
static void wr(const void *p, size_t n) { if (fwrite(p, 1, n, stdout) != n) exit(3); }
static void wr_i32(int32_t v) { wr(&v, 4); }

int main(int argc, char **argv) {
  FILE *in = argc > 1 ? fopen(argv[1], "rb") : stdin;
  if (!in) { fprintf(stderr, "planner_probe: cannot open %s\n", argv[1]); return 2; }
  int32_t head[4];
  double cam[7];
  if (!rd(in, head, sizeof(head)) || head[0] != MAGIC || !rd(in, cam, sizeof(cam))) return 2;
  const int W = head[1], H = head[2], nPlans = head[3];
  if (W <= 0 || H <= 0 || W > 4096 || H > 4096 || nPlans < 0) return 2;
  std::vector<uint16_t> image((size_t) W * H);
  if (!rd(in, image.data(), image.size() * 2)) return 2;
  cv::Mat mat;
  mat.rows = H; mat.cols = W; mat.data = (unsigned char *) image.data();

  wr_i32(MAGIC);
  wr_i32(nPlans);
  for (int p = 0; p < nPlans; p++) {
    int32_t ih[5];
    double st[12];
    if (!rd(in, ih, sizeof(ih)) || !rd(in, st, sizeof(st))) return 2;
    const int nCand = ih[3], nTruth = ih[4];
    if (nCand < 0 || nTruth < 0 || nTruth > nCand) return 2;
    std::vector<int32_t> truthIndex(nTruth);
    if (nTruth && !rd(in, truthIndex.data(), (size_t) nTruth * 4)) return 2;

    DepthImagePlanner planner(mat, cam[0], cam[1], cam[2], cam[3], cam[4], cam[5], cam[6]);
    planner.SetMaxNumberOfPyramids(ih[0]);
    planner.SetRandomSeed(ih[1]);
    Cost cost = {ih[2], {st[9], st[10], st[11]}};
    DepthImagePlanner::RandomTrajectoryGenerator gen(&planner);
    CountedGenerator counted = {&gen, nCand};
    RapidTrajectoryGenerator traj(Vec3d(0, 0, 0), Vec3d(st[0], st[1], st[2]), Vec3d(st[3], st[4], st[5]),
                                  Vec3d(st[6], st[7], st[8]));
    std::vector<TrajectoryTest> tests;
    const bool found = planner.FindLowestCostTrajectory(traj, tests, 1000.0, &cost, &Cost::Get, &counted,
                                                        &CountedGenerator::Next);
    if ((int) tests.size() != nCand) { fprintf(stderr, "planner_probe: %d of %d candidates\n", (int) tests.size(), nCand); return 4; }
    int lastFree = -1;
    std::vector<uint8_t> bits(nCand);
    for (int k = 0; k < nCand; k++) {
      bits[k] = (uint8_t) (int) tests[k].result;
      if (tests[k].result & RectangularPyramidPlanner::CollisionFree) lastFree = k;
    }
    wr_i32(found ? 1 : 0);
    wr_i32(lastFree);
    wr_i32(nCand);
    wr(bits.data(), bits.size());
    wr_i32(planner.GetNumTrajectoriesGenerated());
    wr_i32(planner.GetNumCostChecks());
    wr_i32(planner.GetNumCollisionChecks());
    wr_i32(planner.GetNumVelocityChecks());
    wr_i32(planner.GetNumCollisionFree());
    wr_i32(planner.GetNumPyramids());
    double win[19];
    memset(win, 0, sizeof(win));
    if (found) {
      CommonMath::Trajectory t = traj.GetTrajectory();
      for (int q = 0; q < 6; q++) { const Vec3d c = t[q]; win[3 * q] = c.x; win[3 * q + 1] = c.y; win[3 * q + 2] = c.z; }
      win[18] = t.GetEndTime();
    }
    wr(win, sizeof(win));
    const std::vector<Pyramid> pyramids = planner.GetPyramids();
    if ((int) pyramids.size() != planner.GetNumPyramids()) return 4;
    for (size_t k = 0; k < pyramids.size(); k++) {
      const Pyramid &py = pyramids[k];
      wr(&py.depth, 8);
      wr_i32(py.rightPixBound); wr_i32(py.topPixBound); wr_i32(py.leftPixBound); wr_i32(py.bottomPixBound);
      for (int f = 0; f < 4; f++) { const double n[3] = {py.planeNormals[f].x, py.planeNormals[f].y, py.planeNormals[f].z}; wr(n, sizeof(n)); }
    }
    wr_i32(nTruth);
    for (int k = 0; k < nTruth; k++) {
      if (truthIndex[k] < 0 || truthIndex[k] >= nCand) return 2;
      const uint8_t isFree = planner.IsCollisionFreeGroundTruth(tests[truthIndex[k]].traj.GetTrajectory()) ? 1 : 0;
      wr(&isFree, 1);
    }
  }
  fflush(stdout);
  return 0;
}
