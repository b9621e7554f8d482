// oracle/ref_offboard_probe.cpp -- TEST INFRASTRUCTURE.
// Three pieces of the REFERENCE's offboard stack, compiled from where they lie:
//   Components/Components/Offboard/QuadcopterController.cpp   (named on the compiler's command line, oracle/Makefile; with
//                                                              Logic/QuadcopterPositionController.hpp and
//                                                              Logic/QuadcopterAttitudeController.hpp behind its header)
//   Components/Components/Offboard/SafetyNet.hpp              (#included below)
//   Components/Components/Offboard/PredictionPipe.hpp         (#included below; SafetyNet.hpp pulls it in as well)
// driven by Common/Common/Time/ManualTimer.hpp.  -I oracle/eigen_store: SafetyNet.hpp includes MocapStateEstimator.hpp, whose
// two Eigen::Matrix<double, 2, 2> members need storage; no .cpp of an estimator is compiled and no Eigen arithmetic is on
// this path (it would not compile).  -include cassert -include sstream: SafetyNet.hpp uses assert and std::stringstream
// without including them.
//
// This file's own text is the driver: it reads numbers, calls the reference's functions with them and writes what they
// returned.  Nothing of the three pieces is restated here.  PredictionPipe keeps its deque private and has no size():
// private members are read, nothing is changed (as in ref_rigid_body_probe.cpp).
//
// usage: offboard_probe < request > answer     (binary, little endian; tests/golden/make_offboard_reference.py)
//   request: int32 magic "ROF1", int32 mode, int32 n, then
//   mode 0, Run:          double nat_freq, damping, tc_xy, tc_z (SetParameters' arguments), then n records of 20 doubles:
//                         pos[3], vel[3], att[4], des_pos[3], des_vel[3], des_acc[3], yaw
//                         -> per record double thrust, ang_vel[3]
//   mode 1, RunTracking:  the same four, then n records of 24 doubles: pos[3], vel[3], att[4], ref_pos[3], ref_vel[3],
//                         ref_acc[3], yaw, ref_thrust, ref_ang_vel[3]
//                         -> per record double thrust, ang_vel[3], float cmd_att[4]
//   mode 2, SafetyNet:    double min_corner[3], max_corner[3], min_normal_height (SetSafeCorners' arguments), then n records
//                         of 8 doubles pos[3], att[4], since and 2 int32: fresh (a new SafetyNet with these corners before
//                         the record), set_unsafe (SetUnsafe() after UpdateWithEstimator)
//                         -> per record 5 uint8: vehicleNotSeen, unsafePosition, upsideDownAndLow, userUnsafe, GetIsSafe()
//   mode 3, PredictionPipe: double delay, then n records of int32 op, int32 id, int32 ballistic, int32 pad, int64 advance_us,
//                         double t.  op 0 AddMessage({id, ballistic}); 1 AdvanceMicroSeconds(advance_us) on the ManualTimer
//                         the pipe was made with; 2 GetActiveMessage(t); 3 ClearExpiredMessages(t)
//                         -> per record int32 found (op 2: 0 or 1; otherwise -1), id, ballistic (of the message handed out;
//                         -1 where none), size (messages held after the op), double timeRemaining (NaN where none)
//   answer: int32 magic, mode, n, then the records above
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <stdint.h>
#include <cassert>
#include <deque>
#include <limits>
#include <mutex>
#include <sstream>
#include <string>
#include <vector>
#include <Eigen/Dense>

#define private public
#include "Components/Offboard/PredictionPipe.hpp"
#undef private
#include "Components/Offboard/SafetyNet.hpp"
#include "Components/Offboard/QuadcopterController.hpp"
#include "Common/Time/ManualTimer.hpp"

static const int32_t MAGIC = 0x31464f52;   // "ROF1"

template <typename T>
static bool rd(T *v, size_t n) { return fread(v, sizeof(T), n, stdin) == n; }
template <typename T>
static void wr(const T *v, size_t n) { fwrite(v, sizeof(T), n, stdout); }

static int run_controller(int32_t n, bool tracking) {
  double p[4];
  if (!rd(p, 4)) return 2;
  Offboard::QuadcopterController ctrl;
  ctrl.SetParameters(p[0], p[1], p[2], p[3]);
  const size_t words = tracking ? 24 : 20;
  for (int32_t i = 0; i < n; i++) {
    double r[24];
    if (!rd(r, words)) return 2;
    const Vec3d pos(r[0], r[1], r[2]), vel(r[3], r[4], r[5]);
    const Rotationd att(r[6], r[7], r[8], r[9]);
    const Vec3d a(r[10], r[11], r[12]), b(r[13], r[14], r[15]), c(r[16], r[17], r[18]);
    Vec3d w;
    double thrust;
    if (tracking) {
      Rotationf cmd_att;
      ctrl.RunTracking(pos, vel, att, a, b, c, r[19], r[20], Vec3d(r[21], r[22], r[23]), w, thrust, cmd_att);
      const double out[4] = {thrust, w.x, w.y, w.z};
      const float q[4] = {cmd_att[0], cmd_att[1], cmd_att[2], cmd_att[3]};
      wr(out, 4);
      wr(q, 4);
    } else {
      ctrl.Run(pos, vel, att, a, b, c, r[19], w, thrust);
      const double out[4] = {thrust, w.x, w.y, w.z};
      wr(out, 4);
    }
  }
  return 0;
}

static int run_safety_net(int32_t n) {
  double c[7];
  if (!rd(c, 7)) return 2;
  Offboard::SafetyNet *net = new Offboard::SafetyNet();
  net->SetSafeCorners(Vec3d(c[0], c[1], c[2]), Vec3d(c[3], c[4], c[5]), c[6]);
  for (int32_t i = 0; i < n; i++) {
    double r[8];
    int32_t f[2];
    if (!rd(r, 8) || !rd(f, 2)) return 2;
    if (f[0]) {
      delete net;
      net = new Offboard::SafetyNet();
      net->SetSafeCorners(Vec3d(c[0], c[1], c[2]), Vec3d(c[3], c[4], c[5]), c[6]);
    }
    Offboard::EstimatedState est;
    est.pos = Vec3d(r[0], r[1], r[2]);
    est.vel = Vec3d(0, 0, 0);
    est.angVel = Vec3d(0, 0, 0);
    est.att = Rotationd(r[3], r[4], r[5], r[6]);
    net->UpdateWithEstimator(est, r[7]);
    if (f[1]) net->SetUnsafe();
    const Offboard::SafetyNet::SafetyState s = net->GetSafetyState();
    const uint8_t out[5] = {(uint8_t) s.vehicleNotSeen, (uint8_t) s.unsafePosition, (uint8_t) s.upsideDownAndLow,
                            (uint8_t) s.userUnsafe, (uint8_t) net->GetIsSafe()};
    wr(out, 5);
  }
  delete net;
  return 0;
}

struct PipeMessage {
  int32_t id, ballistic;
};

static int run_pipe(int32_t n) {
  double delay;
  if (!rd(&delay, 1)) return 2;
  ManualTimer clock;
  Offboard::PredictionPipe<PipeMessage> pipe(&clock, delay);
  for (int32_t i = 0; i < n; i++) {
    int32_t h[4];
    int64_t advance;
    double t;
    if (!rd(h, 4) || !rd(&advance, 1) || !rd(&t, 1)) return 2;
    int32_t out[4] = {-1, -1, -1, 0};
    double remaining = std::numeric_limits<double>::quiet_NaN();
    if (h[0] == 0) {
      PipeMessage m = {h[1], h[2]};
      pipe.AddMessage(m);
    } else if (h[0] == 1) {
      if (advance < 0) return 2;
      clock.AdvanceMicroSeconds((uint64_t) advance);
    } else if (h[0] == 2) {
      PipeMessage m = {-1, -1};
      double rem = std::numeric_limits<double>::quiet_NaN();
      const bool found = pipe.GetActiveMessage(t, m, rem);
      out[0] = found ? 1 : 0;
      if (found) {
        out[1] = m.id;
        out[2] = m.ballistic;
        remaining = rem;
      }
    } else if (h[0] == 3) {
      pipe.ClearExpiredMessages(t);
    } else {
      return 2;
    }
    out[3] = (int32_t) pipe._messages.size();
    wr(out, 4);
    wr(&remaining, 1);
  }
  return 0;
}

int main() {
  int32_t head[3];
  if (!rd(head, 3) || head[0] != MAGIC || head[2] < 0) return 2;
  wr(head, 3);
  int rc = 2;
  if (head[1] == 0 || head[1] == 1) rc = run_controller(head[2], head[1] == 1);
  if (head[1] == 2) rc = run_safety_net(head[2]);
  if (head[1] == 3) rc = run_pipe(head[2]);
  if (rc) return rc;
  return fflush(stdout) == 0 ? 0 : 1;
}
