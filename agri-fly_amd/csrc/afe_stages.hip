// afe_stages.hip -- the flight stage machine and its safety net: the top of the field node's offboard loop on the device.
// ExampleVehicleStateMachine::Run of the GPS node (AIFS_ROS/hiperlab_rostools/src/QuadGPSRatesControl/
// ExampleVehicleStateMachine.cpp:106-379), Offboard::SafetyNet (Components/Components/Offboard/SafetyNet.hpp:73-98, :25-43) and
// QuadcopterController::Run (Components/Components/Offboard/QuadcopterController.cpp:11-74), one lane per vehicle, reading the
// engine's slabs (or an attached GPS + IMU estimator's estimate) and writing the engine's rates-command slab.  The C ABI is in
// include/agrifly_engine.h ("flight stage machine").  No step kernel knows about it.
//
// THE DEFINITION (tests/stage_machine_reference.py restates the three classes line by line in scalar Python,
// tests/stages_checker.py in numpy; kernel and checker must give the same bits, so the ORDER below is part of the contract).
// Contraction is off everywhere.  Only sin, cos (double) and sinf, cosf, asinf, acosf (float) are the device library's own:
// afe_stages_selftest_math evaluates the very helpers the kernel calls (afe_offboard_math.h).
//
//   1 BOOKKEEPING  change = stage != last;  last = stage;  t0 = now if change;  ts = (double)(now - t0) * 1e-6 (uint64 difference)
//   2 STATE READ   the follower's: X = anchor_x + (double)px, ... (afe_offboard_math.h load_state), or the estimator's estimate rows
//   3 SAFETY NET   notSeen = since > not_seen_timeout, since = +0 without an estimator, else (double)(now_est - t_update) * 1e-6 with
//                  both times on the estimator's own origin;  unsafePosition = any of p.x < min.x, p.x > max.x, .. (six comparisons);
//                  upsideDownAndLow = p.z < min_normal_height && (M(att) (0, 0, 1)).z < 0;  userUnsafe sticky;  safe = none of the four
//   4 THE SWITCH   in the reference's statement order; ns starts as stage and a later assignment overrides an earlier one:
//       WaitForStart  start -> SpoolUp.                                          message type 0
//       SpoolUp       !safe -> Emergency;  ts > spool_up_time -> Takeoff;  low battery -> Landing
//                     command (float(9.81 * spool_up_thrust_by_weight), 0, 0, 0)  type 5
//       Takeoff       change: init = p;  !safe -> Emergency;  frac = ts / takeoff_time, frac >= 1: -> Flight, frac = 1
//                     des = (1 - frac) * init + frac * desired, desVel = desAcc = +0;  low battery -> Landing;   Run, type 5
//       Flight        !safe -> Emergency;  low battery -> Landing;  frac = min(ts / get_into_action_time, 1)
//                     a = w * ts, (s, c) = sin, cos (a);  for traj 4 also (s4, c4) of (w * ts) * 4
//                       0  pos = desired, vel = acc = +0, yaw = 0
//                       1  r = 1, w = 0.5: pos = (cx + r c, cy + r s, desired.z + r 0), vel = (r w) (-s, c, 0), acc = (r w^2) (-c, -s, 0),
//                          yaw = desiredYaw + a          (pow(w, 2) is exact for 0.5, 1 and 2: the product w * w)
//                       2  w = 2: pos = desired + 1 (0, s, 0), vel = (1 w) (0, c, 0), acc = (1 w^2) (0, -s, 0), yaw = desiredYaw
//                       3  r = 0.5, w = 1: as 1, yaw = 0
//                       4  r = 0.5, w = 0.5: as 1 with z components c4, -s4, -c4, yaw = a
//                       5  pos = desired, vel = acc = +0, yaw = 0.2 * ts
//                     lastPos = (1 - frac) * desired + frac * pos, lastVel = frac * vel, lastAcc = frac * acc;  stop -> Landing;  Run, type 5
//       Landing       !safe -> Emergency;  frac = min(ts / get_into_action_time, 1);  cp = lastPos + ts * (0, 0, -landing_speed)
//                     cp.z < 0 -> Complete;  des = (1 - frac) * lastPos + frac * cp, desVel = (1 - frac) * lastVel + frac * (0, 0, -speed),
//                     desAcc = (1 - frac) * lastAcc + frac * (0, 0, 0);                                         Run, type 5
//       Complete      ready = 1 once ts > 1;                                     type 6 (idle)
//       Emergency     never left;                                                type 2 (kill)
//     The command of a tick is that of the stage the tick ENTERED with.  So an unsafe vehicle in SpoolUp whose time has passed goes
//     to Takeoff, one in Takeoff with frac >= 1 to Flight, low battery after unsafe to Landing, a landing below 0 after unsafe to
//     Complete: the reference's statement order, kept.
//   5 RUN          pf, vf, qf, dp, dv, da = float(..);  w, z = nat_freq, damping
//                  acc = ((dp - pf) * w) * w + (((dv - vf) * 2) * w) * z + da;     proper = acc + (0, 0, 9.81f)
//                  n = sqrtf(proper . proper);  if (double)n > 20: f = float(20.0 / (double)n), proper = f * proper  (Vec3f::operator*=
//                  binds the double quotient to a const float &: one narrowing, Vec3.hpp:155-158)
//                  if (double)proper.z < 0.5 * 9.81: proper.z = float(0.5 * 9.81)
//                  n = sqrtf(proper . proper);  dir = proper / n;  thrust = (double)(n * (M(qf)(0, 0, 1) . dir));  thrust < -1: thrust = -1
//                  att = tilt_attitude(dir) * FromRotationVector((0, 0, float(yaw)));  rates = (double) GetDesiredAngularVelocity(att, qf)
//                  DEAD BRANCHES: behind the z floor dir.z >= 4.905 / 20.6 > 0, so tilt_angle's cosAngle <= -1 arm (angle = pi) cannot be
//                  taken, and NaN apart the direction's norm is never 0.  The thrust floor IS live (an inverted vehicle).
//   6 CODEC        computed = float(thrust), float(rates) for type 5, four +0 otherwise;  sent = radio_quantise35 of each
//     DELAY LINE   the message (type, four floats) goes into the machine's own ring; the host keeps the due times (the follower's rule,
//                  afe_follower_ring_slots).  The newest due message is delivered: type 5 -> the four floats, have = 1; type 6 or 2 ->
//                  four +0, have = 0; type 0 -> nothing is written.  The on-device logic has no sticky FS_KILLED: Emergency is never
//                  left and kills every period, so the effect is the same.
//   7 COUNTERS     after the tick: vehicles per stage [0..6] and the ready ones [7], one ballot per counter and wave.
//
// NOT COVERED: the mocap node's variant of the class (the device mocap estimator keeps no last-good-measurement time, and its
// announce ring needs per-stage rules), PublishEstimate's Euler angles, delivery between ticks, rappids_headless.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <vector>

#include "afe_consumer.h"
#include "afe_estimator.h"
#include "afe_gps_estimator.h"
#include "afe_offboard_math.h"

namespace {

using namespace afe_offboard;

constexpr int kBlock = 256;
constexpr int64_t kBlocksPerLaunch = int64_t(1) << 22;   // a launch stays below 2^31 threads
constexpr int kMsgNone = 0, kMsgKill = 2, kMsgRates = 5, kMsgIdle = 6;   // RadioTypes.hpp:18-24
// byte rows
constexpr int kBStage = 0, kBLast = 1, kBSafety = 2, kBReady = 3, kBRequest = 4, kBWarn = 5, kBUser = 6, kBType = 7, kBytes = 8;
// double rows
constexpr int kDInit = 0, kDDes = 3, kDLastPos = 6, kDLastVel = 9, kDLastAcc = 12, kDDesYaw = 15, kDCmdYaw = 16, kDCentre = 17, kDoubles = 19;

struct Tune {
  float nat_freq, damping, tc_xy, tc_z;
  double min_x, min_y, min_z, max_x, max_y, max_z, min_normal_height, not_seen_timeout;
  double spool_time, spool_thrust, takeoff_time, action_time, landing_speed;
  int traj_id;
};

struct StagesArgs {
  // the engine's slabs (or the estimator's estimate rows): planar, `stride` elements between components
  const void *pos, *vel, *att;
  const double *anchor_xy;
  const unsigned long long *t_update;   // the estimator's last-good-update row (EST kernels only)
  float *rates_cmd;
  uint8_t *have_cmd;
  int64_t stride, n;
  // the machine's own slabs, the same stride
  uint8_t *bytes;                       // [kBytes]
  unsigned long long *t0_us;
  double *dbl;                          // [kDoubles]
  float *computed, *sent;               // [4] each
  float *ring;                          // [slots][4]
  uint8_t *ring_type;                   // [slots]
  unsigned long long *counters;         // [8], or NULL: not counted
  Tune tune;
};

struct Command {
  double thrust;
  V3 ang_vel;
};

// QuadcopterController::Run, QuadcopterController.cpp:11-74 (5 RUN above)
__device__ __forceinline__ Command run_position(const Tune &t, const V3 &pos, const V3 &vel, const Q4 &att, const V3 &desPos, const V3 &desVel,
                                                const V3 &desAcc, double yaw) {
#pragma clang fp contract(off)
  V3f pf, vf, dp, dv, da;
  pf.x = (float)pos.x; pf.y = (float)pos.y; pf.z = (float)pos.z;
  vf.x = (float)vel.x; vf.y = (float)vel.y; vf.z = (float)vel.z;
  dp.x = (float)desPos.x; dp.y = (float)desPos.y; dp.z = (float)desPos.z;
  dv.x = (float)desVel.x; dv.y = (float)desVel.y; dv.z = (float)desVel.z;
  da.x = (float)desAcc.x; da.y = (float)desAcc.y; da.z = (float)desAcc.z;
  Q4f qf;
  qf.w = (float)att.w; qf.x = (float)att.x; qf.y = (float)att.y; qf.z = (float)att.z;
  const float w = t.nat_freq, z = t.damping;
  V3f proper;
  proper.x = (((dp.x - pf.x) * w) * w + (((dv.x - vf.x) * 2) * w) * z + da.x) + 0.0f;
  proper.y = (((dp.y - pf.y) * w) * w + (((dv.y - vf.y) * 2) * w) * z + da.y) + 0.0f;
  proper.z = (((dp.z - pf.z) * w) * w + (((dv.z - vf.z) * 2) * w) * z + da.z) + 9.81f;
  const float n0 = sqrtf(vf_dot(proper, proper));
  if ((double)n0 > 20.0) {                                               // _maxProperAcc, :27-29
    const float f = (float)(20.0 / (double)n0);
    proper.x = f * proper.x; proper.y = f * proper.y; proper.z = f * proper.z;
  }
  if ((double)proper.z < 0.5 * 9.81) proper.z = (float)(0.5 * 9.81);     // _minVerticalProperAcceleration, :32-34
  const float n = sqrtf(vf_dot(proper, proper));
  V3f dir;
  dir.x = proper.x / n; dir.y = proper.y / n; dir.z = proper.z / n;
  V3f e3;
  e3.x = 0.0f; e3.y = 0.0f; e3.z = 1.0f;
  const V3f bz = mf_rotate(qf_matrix(qf), e3);
  Command c;
  c.thrust = (double)(n * vf_dot(bz, dir));
  if (c.thrust < -1.0) c.thrust = -1.0;                                  // _minProperAcc, :44-46
  V3f yv;
  yv.x = 0.0f; yv.y = 0.0f; yv.z = (float)yaw;
  const Q4f cmdAtt = qf_mul(tilt_attitude(dir), qf_from_rotvec(yv));
  const V3f we = desired_angular_velocity(cmdAtt, qf, t.tc_xy, t.tc_z);
  c.ang_vel.x = (double)we.x; c.ang_vel.y = (double)we.y; c.ang_vel.z = (double)we.z;
  return c;
}

__device__ __forceinline__ double min_first(double a, double b) { return b < a ? b : a; }   // std::min(a, b)

__global__ void __launch_bounds__(kBlock) afe_stages_init_kernel(StagesArgs g, int slots, double centre_y) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= g.n) return;
  const int64_t S = g.stride;
  for (int k = 0; k < kBytes; k++) g.bytes[k * S + v] = 0;
  g.bytes[kBLast * S + v] = 5;                                           // _lastFlightStage = StageComplete (:92)
  g.bytes[kBSafety * S + v] = 1;                                         // SafetyState(): vehicleNotSeen = true
  g.t0_us[v] = 0;
  for (int k = 0; k < kDoubles; k++) g.dbl[k * S + v] = 0.0;
  g.dbl[(kDCentre + 1) * S + v] = centre_y;
  for (int k = 0; k < 4; k++) { g.computed[k * S + v] = 0.0f; g.sent[k * S + v] = 0.0f; }
  for (int k = 0; k < 4 * slots; k++) g.ring[k * S + v] = 0.0f;
  for (int k = 0; k < slots; k++) g.ring_type[k * S + v] = 0;
}

// One period of ExampleVehicleStateMachine::Run for every vehicle.  write_slot: where this tick's message goes; deliver_slot: the
// newest message that is due (-1: none).  EST: the state is the estimator's estimate and now_est its clock; else now_est is unused.
// The stage switch only chooses the controller's inputs: run_position is called in ONE place.
template <typename T, bool EST>
__global__ void __launch_bounds__(kBlock) afe_stages_tick_kernel(StagesArgs g, unsigned long long now_us, unsigned long long now_est, int start_all,
                                                                 int stop_all, int write_slot, int deliver_slot) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t S = g.stride;
  int ns = -1, ready = 0;
  if (v < g.n) {
    const Tune &t = g.tune;
    uint8_t *B = g.bytes + v;
    double *D = g.dbl + v;
    // 1
    const int stage = B[kBStage * S];
    const bool change = stage != B[kBLast * S];
    unsigned long long t0 = g.t0_us[v];
    if (change) t0 = now_us;
    const double ts = (double)(now_us - t0) * 1e-6;
    // 2
    V3 p, vel;
    Q4 q;
    load_state<T>(g, v, p, vel, q);
    // 3
    double since = 0.0;
    if (EST) since = (double)(now_est - g.t_update[v]) * 1e-6;
    int safety = 0;
    if (since > t.not_seen_timeout) safety |= 1;
    if (p.x < t.min_x || p.x > t.max_x || p.y < t.min_y || p.y > t.max_y || p.z < t.min_z || p.z > t.max_z) safety |= 2;
    if (p.z < t.min_normal_height) {
      V3 e3;
      e3.x = 0.0; e3.y = 0.0; e3.z = 1.0;
      if (m_rotate(q_matrix(q), e3).z < 0.0) safety |= 4;
    }
    if (B[kBUser * S]) safety |= 8;
    const bool safe = safety == 0;
    const int request = B[kBRequest * S];
    const bool start = start_all || (request & 1), stop = stop_all || (request & 2);
    const bool low_batt = (B[kBWarn * S] & 0x01) != 0;                    // WARN_LOW_BATT, TelemetryPacket.hpp:22
    // 4
    ns = stage;
    ready = B[kBReady * S];
    int type = kMsgNone;
    bool run = false;
    float c0 = 0.0f;
    V3 desPos, desVel, desAcc;
    desPos.x = desPos.y = desPos.z = 0.0;
    desVel = desPos; desAcc = desPos;
    double yaw = D[kDCmdYaw * S];
    V3 des;
    des.x = D[(kDDes + 0) * S]; des.y = D[(kDDes + 1) * S]; des.z = D[(kDDes + 2) * S];
    if (stage == 0) {
      if (start) ns = 1;
    } else if (stage == 1) {
      if (!safe) ns = 6;
      type = kMsgRates;
      c0 = (float)(9.81 * t.spool_thrust);
      if (ts > t.spool_time) ns = 2;
      if (low_batt) ns = 4;
    } else if (stage == 2) {
      V3 init;
      if (change) {
        init = p;
        D[(kDInit + 0) * S] = p.x; D[(kDInit + 1) * S] = p.y; D[(kDInit + 2) * S] = p.z;
      } else {
        init.x = D[(kDInit + 0) * S]; init.y = D[(kDInit + 1) * S]; init.z = D[(kDInit + 2) * S];
      }
      if (!safe) ns = 6;
      double frac = ts / t.takeoff_time;
      if (frac >= 1.0) { ns = 3; frac = 1.0; }
      const double a = 1 - frac;
      desPos.x = a * init.x + frac * des.x; desPos.y = a * init.y + frac * des.y; desPos.z = a * init.z + frac * des.z;
      type = kMsgRates; run = true;
      if (low_batt) ns = 4;
    } else if (stage == 3) {
      if (!safe) ns = 6;
      if (low_batt) ns = 4;
      const double frac = min_first(ts / t.action_time, 1.0);
      V3 cp = des, cv, ca;
      cv.x = cv.y = cv.z = 0.0;
      ca = cv;
      const int id = t.traj_id;
      if (id == 0) yaw = 0;
      else if (id == 5) yaw = 0.2 * ts;
      else if (id == 2) {
        const double arg = 2.0 * ts, k1 = 1.0 * 2.0, k2 = 1.0 * (2.0 * 2.0);
        double s, c;
        dm_sincos(arg, &s, &c);
        cp.x = des.x + 1.0 * 0.0; cp.y = des.y + 1.0 * s; cp.z = des.z + 1.0 * 0.0;
        cv.x = k1 * 0.0; cv.y = k1 * c; cv.z = k1 * 0.0;
        ca.x = k2 * 0.0; ca.y = k2 * (-s); ca.z = k2 * 0.0;
        yaw = D[kDDesYaw * S];
      } else {                                                           // 1, 3, 4: the circles
        const double r = id == 1 ? 1.0 : 0.5, w = id == 3 ? 1.0 : 0.5;
        const double arg = w * ts, k1 = r * w, k2 = r * (w * w);
        double s, c, zc = 0.0, zv = 0.0, za = 0.0;
        dm_sincos(arg, &s, &c);
        if (id == 4) {
          double s4, c4;
          dm_sincos(arg * 4, &s4, &c4);
          zc = c4; zv = -s4; za = -c4;
        }
        cp.x = D[(kDCentre + 0) * S] + r * c; cp.y = D[(kDCentre + 1) * S] + r * s; cp.z = des.z + r * zc;
        cv.x = k1 * (-s); cv.y = k1 * c; cv.z = k1 * zv;
        ca.x = k2 * (-c); ca.y = k2 * (-s); ca.z = k2 * za;
        yaw = id == 1 ? D[kDDesYaw * S] + arg : id == 3 ? 0.0 : arg;
      }
      const double a = 1 - frac;
      desPos.x = a * des.x + frac * cp.x; desPos.y = a * des.y + frac * cp.y; desPos.z = a * des.z + frac * cp.z;
      desVel.x = frac * cv.x; desVel.y = frac * cv.y; desVel.z = frac * cv.z;
      desAcc.x = frac * ca.x; desAcc.y = frac * ca.y; desAcc.z = frac * ca.z;
      D[(kDLastPos + 0) * S] = desPos.x; D[(kDLastPos + 1) * S] = desPos.y; D[(kDLastPos + 2) * S] = desPos.z;
      D[(kDLastVel + 0) * S] = desVel.x; D[(kDLastVel + 1) * S] = desVel.y; D[(kDLastVel + 2) * S] = desVel.z;
      D[(kDLastAcc + 0) * S] = desAcc.x; D[(kDLastAcc + 1) * S] = desAcc.y; D[(kDLastAcc + 2) * S] = desAcc.z;
      D[kDCmdYaw * S] = yaw;
      type = kMsgRates; run = true;
      if (stop) ns = 4;
    } else if (stage == 4) {
      if (!safe) ns = 6;
      const double frac = min_first(ts / t.action_time, 1.0), down = -t.landing_speed;
      V3 lp, lv, la, cp;
      lp.x = D[(kDLastPos + 0) * S]; lp.y = D[(kDLastPos + 1) * S]; lp.z = D[(kDLastPos + 2) * S];
      lv.x = D[(kDLastVel + 0) * S]; lv.y = D[(kDLastVel + 1) * S]; lv.z = D[(kDLastVel + 2) * S];
      la.x = D[(kDLastAcc + 0) * S]; la.y = D[(kDLastAcc + 1) * S]; la.z = D[(kDLastAcc + 2) * S];
      cp.x = lp.x + ts * 0.0; cp.y = lp.y + ts * 0.0; cp.z = lp.z + ts * down;
      if (cp.z < 0) ns = 5;
      const double a = 1 - frac;
      desPos.x = a * lp.x + frac * cp.x; desPos.y = a * lp.y + frac * cp.y; desPos.z = a * lp.z + frac * cp.z;
      desVel.x = a * lv.x + frac * 0.0; desVel.y = a * lv.y + frac * 0.0; desVel.z = a * lv.z + frac * down;
      desAcc.x = a * la.x + frac * 0.0; desAcc.y = a * la.y + frac * 0.0; desAcc.z = a * la.z + frac * 0.0;
      type = kMsgRates; run = true;
    } else if (stage == 5) {
      type = kMsgIdle;
      if (ts > 1.0) ready = 1;
    } else {
      type = kMsgKill;
    }
    // 5, 6
    float c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
    if (run) {
      const Command c = run_position(t, p, vel, q, desPos, desVel, desAcc, yaw);
      c0 = (float)c.thrust; c1 = (float)c.ang_vel.x; c2 = (float)c.ang_vel.y; c3 = (float)c.ang_vel.z;
    }
    const float s0 = radio_quantise35(c0), s1 = radio_quantise35(c1), s2 = radio_quantise35(c2), s3 = radio_quantise35(c3);
    float d0 = s0, d1 = s1, d2 = s2, d3 = s3;
    int dtype = type;
    if (deliver_slot >= 0 && deliver_slot != write_slot) {
      const float *R = g.ring + (int64_t)deliver_slot * 4 * S + v;
      d0 = R[0]; d1 = R[S]; d2 = R[2 * S]; d3 = R[3 * S];
      dtype = g.ring_type[(int64_t)deliver_slot * S + v];
    }
    g.computed[v] = c0; g.computed[S + v] = c1; g.computed[2 * S + v] = c2; g.computed[3 * S + v] = c3;
    g.sent[v] = s0; g.sent[S + v] = s1; g.sent[2 * S + v] = s2; g.sent[3 * S + v] = s3;
    {
      float *W = g.ring + (int64_t)write_slot * 4 * S + v;
      W[0] = s0; W[S] = s1; W[2 * S] = s2; W[3 * S] = s3;
      g.ring_type[(int64_t)write_slot * S + v] = (uint8_t)type;
    }
    if (deliver_slot >= 0 && dtype != kMsgNone) {
      const bool rates = dtype == kMsgRates;
      g.rates_cmd[v] = rates ? d0 : 0.0f; g.rates_cmd[S + v] = rates ? d1 : 0.0f;
      g.rates_cmd[2 * S + v] = rates ? d2 : 0.0f; g.rates_cmd[3 * S + v] = rates ? d3 : 0.0f;
      g.have_cmd[v] = rates ? 1 : 0;
    }
    B[kBStage * S] = (uint8_t)ns;
    B[kBLast * S] = (uint8_t)stage;
    B[kBSafety * S] = (uint8_t)safety;
    B[kBReady * S] = (uint8_t)ready;
    B[kBType * S] = (uint8_t)type;
    g.t0_us[v] = t0;
  }
  // 7
  if (g.counters) {
    const bool lead = (threadIdx.x & 63) == 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const unsigned long long mask = __ballot(k < 7 ? ns == k : ready != 0);
      if (lead && mask) atomicAdd(g.counters + k, (unsigned long long)__popcll(mask));
    }
  }
}

__global__ void __launch_bounds__(kBlock) afe_stages_math_f64_kernel(int op, int64_t n, const double *x, double *y) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double s, c;
  dm_sincos(x[i], &s, &c);
  y[i] = op == 0 ? s : c;
}
__global__ void __launch_bounds__(kBlock) afe_stages_math_f32_kernel(int op, int64_t n, const float *x, float *y) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float s, c;
  fm_sincosf(x[i], &s, &c);
  y[i] = op == 2 ? s : op == 3 ? c : op == 4 ? fm_asinf(x[i]) : fm_acosf(x[i]);
}

size_t up256(size_t x) { return (x + 255) & ~size_t(255); }

}  // namespace

struct afe_stages {
  afe_engine *engine = nullptr;     // borrowed
  int device = 0;
  int64_t n = 0, stride = 0;
  int slots = 0;
  uint64_t period_us = 0, delay_us = 0;
  uint64_t n_ticks = 0, seq = 0;    // seq: messages sent so far; message k lives in slot k % slots
  std::deque<uint64_t> due;         // due times of the messages in flight, in send order
  afe_gps_estimator *gps = nullptr; // borrowed; attached: the state read is its estimate
  afe::DevBuf arena;
  StagesArgs args;                  // the machine's part of the kernel arguments
};

namespace {

// estimated: the call reads estState; now_est: the estimator's clock at this moment
int enter(afe_stages *s, hipStream_t *stream, StagesArgs *g, int *elem, bool want_cmd_slabs, bool estimated, uint64_t *now_est) {
  afe::EngineAccess acc;
  int rc = afe::engine_enter(s->engine, &acc);
  if (rc != AFE_OK) return rc;
  const afe_device_view &view = acc.view;
  if (view.n_vehicles != s->n || view.stride != s->stride || acc.device != s->device) return AFE_ERR_INVALID_ARG;
  *stream = acc.stream;
  *g = s->args;
  g->pos = view.pos; g->vel = view.vel; g->att = view.att;
  g->anchor_xy = view.pos_anchor_xy;
  g->t_update = nullptr;
  *elem = view.state_elem_size;
  if (estimated && s->gps) {                                   // GetCurrentEstimate(), no prediction ahead
    uint64_t n_ticks = 0, now = 0, origin = 0;
    rc = afe_logic_ticks(s->engine, &n_ticks);
    if (rc != AFE_OK) return rc;
    afe::EstimatorLink link;
    rc = afe::gps_estimator_link(s->gps, n_ticks, &link);
    if (rc != AFE_OK) return rc;
    rc = afe::gps_estimator_last_update(s->gps, &g->t_update, &origin);
    if (rc != AFE_OK) return rc;
    rc = afe_time_us(s->engine, &now);
    if (rc != AFE_OK) return rc;
    if (now < origin) return AFE_ERR_OUT_OF_RANGE;             // (the engine's clock was set back)
    *now_est = now - origin;
    g->pos = link.pos; g->vel = link.vel; g->att = link.att;
    g->anchor_xy = link.zero_anchor_xy;
    *elem = 8;
  }
  if (want_cmd_slabs) return afe::engine_rates_slabs(s->engine, &g->rates_cmd, &g->have_cmd);
  return AFE_OK;
}

template <typename F>
int for_each_launch(int64_t n, F &&launch) {
  const int64_t per = kBlocksPerLaunch * kBlock;
  if (n > per) return AFE_ERR_OUT_OF_RANGE;      // (one launch covers 2^30 vehicles: more than an engine holds)
  if (n <= 0) return AFE_OK;
  launch(dim3((unsigned)((n + kBlock - 1) / kBlock)));
  return hipGetLastError() == hipSuccess ? AFE_OK : AFE_ERR_HIP;
}

// host planar [comps][count] <-> the machine's planar [comps][stride] at `first`; the stream has been waited for
bool put_rows(void *dev, size_t esz, int comps, int64_t stride, int64_t first, int64_t count, const void *host) {
  return hipMemcpy2D((char *)dev + (size_t)first * esz, (size_t)stride * esz, host, (size_t)count * esz, (size_t)count * esz, (size_t)comps,
                     hipMemcpyHostToDevice) == hipSuccess;
}
bool get_rows(const void *dev, size_t esz, int comps, int64_t stride, int64_t first, int64_t count, void *host) {
  return hipMemcpy2D(host, (size_t)count * esz, (const char *)dev + (size_t)first * esz, (size_t)stride * esz, (size_t)count * esz, (size_t)comps,
                     hipMemcpyDeviceToHost) == hipSuccess;
}

// [first, first + count) against the machine, nothing touched
int enter_rows(afe_stages *s, int64_t first, int64_t count) {
  if (!s || first < 0 || count < 0) return AFE_ERR_INVALID_ARG;
  if (first > s->n || count > s->n - first) return AFE_ERR_OUT_OF_RANGE;   // (no sum: it can wrap)
  return AFE_OK;
}
// through the engine's gate, then its stream drained: the copies that follow are synchronous
int drain(afe_stages *s) {
  hipStream_t stream = nullptr;
  StagesArgs g;
  int elem = 0;
  const int rc = enter(s, &stream, &g, &elem, false, false, nullptr);
  if (rc != AFE_OK) return rc;
  return hipStreamSynchronize(stream) == hipSuccess ? AFE_OK : AFE_ERR_HIP;
}

// a planar double row group of the machine from a host array; the follower's conventions for count == 0 and NULL
int set_doubles(afe_stages *s, int64_t first, int64_t count, const double *host, int row, int comps) {
  const int arc = enter_rows(s, first, count);
  if (arc != AFE_OK) return arc;
  if (!host) return AFE_ERR_INVALID_ARG;
  if (count == 0) return AFE_OK;
  const int rc = drain(s);
  if (rc != AFE_OK) return rc;
  return put_rows(s->args.dbl + (size_t)row * (size_t)s->stride, 8, comps, s->stride, first, count, host) ? AFE_OK : AFE_ERR_HIP;
}
int fill_bytes(afe_stages *s, int64_t first, int64_t count, int row, int value) {
  const int arc = enter_rows(s, first, count);
  if (arc != AFE_OK) return arc;
  if (count == 0) return AFE_OK;
  const int rc = drain(s);
  if (rc != AFE_OK) return rc;
  const std::vector<uint8_t> host((size_t)count, (uint8_t)value);         // (a synchronous copy, like every other setter)
  return put_rows(s->args.bytes + (size_t)row * (size_t)s->stride, 1, 1, s->stride, first, count, host.data()) ? AFE_OK : AFE_ERR_HIP;
}

bool tuning_row(int type, float *nat_freq, float *damping, float *tc_xy, float *tc_z) {
  afe_follower_config f;
  if (afe_follower_default_config(type, &f) != AFE_OK) return false;     // QuadcopterConstants.hpp, as the follower derives them
  *nat_freq = f.nat_freq; *damping = f.damping; *tc_xy = f.att_time_const_xy; *tc_z = f.att_time_const_z;
  return true;
}

bool positive(double x) { return std::isfinite(x) && x > 0; }

}  // namespace

extern "C" int afe_stages_default_config(int quadcopter_type, afe_stages_config *cfg) {
  if (!cfg) return AFE_ERR_INVALID_ARG;
  afe_stages_config c;
  std::memset(&c, 0, sizeof(c));
  if (!tuning_row(quadcopter_type, &c.nat_freq, &c.damping, &c.att_time_const_xy, &c.att_time_const_z)) return AFE_ERR_INVALID_ARG;
  c.struct_bytes = sizeof(c);
  c.period_us = 20000;                 // mainLoopFrequency = 50, main.cpp
  c.delay_us = 30000;
  c.min_corner[0] = -100; c.min_corner[1] = -100; c.min_corner[2] = -2.0;   // ExampleVehicleStateMachine.cpp:88
  c.max_corner[0] = 100; c.max_corner[1] = 100; c.max_corner[2] = 20;
  c.min_normal_height = 0.0;
  c.not_seen_timeout_s = 0.5;          // SafetyNet.hpp:57
  c.spool_up_time_s = 0.5;             // :145-146
  c.spool_up_thrust_by_weight = 0.25;
  c.takeoff_time_s = 2.0;              // :185
  c.get_into_action_time_s = 2.0;      // :222, :323
  c.landing_speed = 0.5;               // :322
  c.traj_id = 3;                       // :219
  *cfg = c;
  return AFE_OK;
}

extern "C" int afe_stages_create(afe_engine *e, const afe_stages_config *cfg, afe_stages **out) {
  if (!e || !cfg || !out || cfg->struct_bytes < sizeof(afe_stages_config)) return AFE_ERR_INVALID_ARG;
  if (!(cfg->att_time_const_xy > 0) || !(cfg->att_time_const_z > 0) || !std::isfinite(cfg->nat_freq) || !std::isfinite(cfg->damping) ||
      !positive(cfg->takeoff_time_s) || !positive(cfg->get_into_action_time_s) || !std::isfinite(cfg->spool_up_time_s) ||
      !std::isfinite(cfg->spool_up_thrust_by_weight) || !std::isfinite(cfg->landing_speed) || !std::isfinite(cfg->min_normal_height) ||
      !std::isfinite(cfg->not_seen_timeout_s))
    return AFE_ERR_INVALID_ARG;
  for (int k = 0; k < 3; k++) if (!(cfg->min_corner[k] < cfg->max_corner[k])) return AFE_ERR_INVALID_ARG;   // SafetyNet.hpp:68-70's assert
  if (cfg->traj_id < 0 || cfg->traj_id > 5) return AFE_ERR_INVALID_ARG;
  int slots = 0;
  int rc = afe_follower_ring_slots(cfg->period_us, cfg->delay_us, &slots);
  if (rc != AFE_OK) return rc;
  afe::EngineAccess acc;
  rc = afe::engine_enter(e, &acc);
  if (rc != AFE_OK) return rc;
  rc = afe::engine_device_resident(e);
  if (rc != AFE_OK) return rc;
  float *rates_cmd = nullptr;
  uint8_t *have_cmd = nullptr;
  rc = afe::engine_rates_slabs(e, &rates_cmd, &have_cmd);
  if (rc != AFE_OK) return rc;
  afe_stages *s = new afe_stages();
  s->engine = e; s->device = acc.device; s->n = acc.view.n_vehicles; s->stride = acc.view.stride;
  s->slots = slots; s->period_us = cfg->period_us; s->delay_us = cfg->delay_us;
  const size_t S = (size_t)s->stride;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += up256(bytes); return o; };
  const size_t o_bytes = take(S * kBytes), o_t0 = take(S * 8), o_dbl = take(S * kDoubles * 8), o_comp = take(S * 4 * 4), o_sent = take(S * 4 * 4),
               o_ring = take(S * 4 * 4 * (size_t)slots), o_rtype = take(S * (size_t)slots), o_cnt = take(64);
  if (!s->arena.alloc(off)) { (void)hipGetLastError(); delete s; return AFE_ERR_HIP; }
  unsigned char *A = s->arena.as<unsigned char>();
  std::memset(&s->args, 0, sizeof(s->args));
  StagesArgs &g = s->args;
  g.n = s->n; g.stride = s->stride;
  g.bytes = A + o_bytes; g.t0_us = (unsigned long long *)(A + o_t0); g.dbl = (double *)(A + o_dbl);
  g.computed = (float *)(A + o_comp); g.sent = (float *)(A + o_sent); g.ring = (float *)(A + o_ring); g.ring_type = A + o_rtype;
  g.counters = (unsigned long long *)(A + o_cnt);
  Tune &t = g.tune;
  t.nat_freq = cfg->nat_freq; t.damping = cfg->damping; t.tc_xy = cfg->att_time_const_xy; t.tc_z = cfg->att_time_const_z;
  t.min_x = cfg->min_corner[0]; t.min_y = cfg->min_corner[1]; t.min_z = cfg->min_corner[2];
  t.max_x = cfg->max_corner[0]; t.max_y = cfg->max_corner[1]; t.max_z = cfg->max_corner[2];
  t.min_normal_height = cfg->min_normal_height; t.not_seen_timeout = cfg->not_seen_timeout_s;
  t.spool_time = cfg->spool_up_time_s; t.spool_thrust = cfg->spool_up_thrust_by_weight; t.takeoff_time = cfg->takeoff_time_s;
  t.action_time = cfg->get_into_action_time_s; t.landing_speed = cfg->landing_speed; t.traj_id = cfg->traj_id;
  const hipStream_t stream = acc.stream;
  const double centre_y = cfg->traj_id == 1 ? -2.0 : 0.0;                  // :236, :264, :279
  rc = hipMemsetAsync(A, 0, off, stream) == hipSuccess ? AFE_OK : AFE_ERR_HIP;     // (the padding beyond n included)
  if (rc == AFE_OK)
    rc = for_each_launch(g.n, [&](dim3 grid) { hipLaunchKernelGGL(afe_stages_init_kernel, grid, dim3(kBlock), 0, stream, g, slots, centre_y); });
  if (rc == AFE_OK && hipStreamSynchronize(stream) != hipSuccess) rc = AFE_ERR_HIP;
  if (rc != AFE_OK) { (void)hipGetLastError(); (void)afe_stages_destroy(s); return rc; }
  *out = s;
  return AFE_OK;
}

extern "C" int afe_stages_destroy(afe_stages *s) {
  if (!s) return AFE_ERR_INVALID_ARG;
  (void)hipSetDevice(s->device);
  (void)hipDeviceSynchronize();
  delete s;
  return AFE_OK;
}

extern "C" int afe_stages_info(const afe_stages *s, int64_t *n_vehicles, int *slots, uint64_t *n_ticks, int *in_flight) {
  if (!s) return AFE_ERR_INVALID_ARG;
  if (n_vehicles) *n_vehicles = s->n;
  if (slots) *slots = s->slots;
  if (n_ticks) *n_ticks = s->n_ticks;
  if (in_flight) *in_flight = (int)s->due.size();
  return AFE_OK;
}

extern "C" int afe_stages_set_desired_position(afe_stages *s, int64_t first, int64_t count, const double *pos3) {
  return set_doubles(s, first, count, pos3, kDDes, 3);
}
extern "C" int afe_stages_set_desired_yaw(afe_stages *s, int64_t first, int64_t count, const double *yaw) {
  return set_doubles(s, first, count, yaw, kDDesYaw, 1);
}
extern "C" int afe_stages_set_centre(afe_stages *s, int64_t first, int64_t count, const double *xy2) {
  return set_doubles(s, first, count, xy2, kDCentre, 2);
}
extern "C" int afe_stages_set_unsafe(afe_stages *s, int64_t first, int64_t count) { return fill_bytes(s, first, count, kBUser, 1); }
extern "C" int afe_stages_request(afe_stages *s, int64_t first, int64_t count, int start, int stop) {
  return fill_bytes(s, first, count, kBRequest, (start ? 1 : 0) | (stop ? 2 : 0));
}
extern "C" int afe_stages_set_warnings(afe_stages *s, int64_t first, int64_t count, const uint8_t *warnings) {
  const int arc = enter_rows(s, first, count);
  if (arc != AFE_OK) return arc;
  if (!warnings) return AFE_ERR_INVALID_ARG;
  if (count == 0) return AFE_OK;
  const int rc = drain(s);
  if (rc != AFE_OK) return rc;
  return put_rows(s->args.bytes + (size_t)kBWarn * (size_t)s->stride, 1, 1, s->stride, first, count, warnings) ? AFE_OK : AFE_ERR_HIP;
}

extern "C" int afe_stages_get(afe_stages *s, int64_t first, int64_t count, const afe_stages_fields *f) {
  const int arc = enter_rows(s, first, count);
  if (arc != AFE_OK) return arc;
  if (!f || f->struct_bytes < sizeof(afe_stages_fields)) return AFE_ERR_INVALID_ARG;
  if (!f->stage && !f->last_stage && !f->t0_us && !f->safety && !f->ready && !f->init_pos3 && !f->desired_pos3 && !f->last_pos3 && !f->last_vel3 &&
      !f->last_acc3 && !f->cmd_yaw && !f->computed4 && !f->sent4 && !f->msg_type)
    return AFE_ERR_INVALID_ARG;
  if (count == 0) return AFE_OK;
  const int rc = drain(s);
  if (rc != AFE_OK) return rc;
  const StagesArgs &g = s->args;
  const int64_t S = s->stride;
  auto byte_row = [&](int row, uint8_t *host) { return !host || get_rows(g.bytes + (size_t)row * (size_t)S, 1, 1, S, first, count, host); };
  auto dbl_rows = [&](int row, int comps, double *host) { return !host || get_rows(g.dbl + (size_t)row * (size_t)S, 8, comps, S, first, count, host); };
  if (!byte_row(kBStage, f->stage) || !byte_row(kBLast, f->last_stage) || !byte_row(kBSafety, f->safety) || !byte_row(kBReady, f->ready) ||
      !byte_row(kBType, f->msg_type) || (f->t0_us && !get_rows(g.t0_us, 8, 1, S, first, count, f->t0_us)) || !dbl_rows(kDInit, 3, f->init_pos3) ||
      !dbl_rows(kDDes, 3, f->desired_pos3) || !dbl_rows(kDLastPos, 3, f->last_pos3) || !dbl_rows(kDLastVel, 3, f->last_vel3) ||
      !dbl_rows(kDLastAcc, 3, f->last_acc3) || !dbl_rows(kDCmdYaw, 1, f->cmd_yaw) ||
      (f->computed4 && !get_rows(g.computed, 4, 4, S, first, count, f->computed4)) || (f->sent4 && !get_rows(g.sent, 4, 4, S, first, count, f->sent4)))
    return AFE_ERR_HIP;
  return AFE_OK;
}

extern "C" int afe_stages_tick(afe_stages *s, int should_start, int should_stop, int64_t *counts8) {
  if (!s) return AFE_ERR_INVALID_ARG;
  hipStream_t stream = nullptr;
  StagesArgs g;
  int elem = 0;
  uint64_t now_est = 0;
  int rc = enter(s, &stream, &g, &elem, true, true, &now_est);
  if (rc != AFE_OK) return rc;
  uint64_t now_us = 0;
  rc = afe_time_us(s->engine, &now_us);
  if (rc != AFE_OK) return rc;
  // the delay line's bookkeeping (CommunicationsDelay.hpp:18-33), as the follower keeps it: this tick's message is sent, then
  // every message that is due is delivered in send order -- the newest of them is what the vehicle is left with
  size_t n_due = 0;
  while (n_due < s->due.size() && s->due[n_due] <= now_us) n_due++;
  if (s->due.size() - n_due + 1 > (size_t)s->slots) return AFE_ERR_OUT_OF_RANGE;   // ticks closer together than the period: the ring is full
  const uint64_t oldest = s->seq - s->due.size();
  const int write_slot = (int)(s->seq % (uint64_t)s->slots);
  int deliver_slot = n_due ? (int)((oldest + n_due - 1) % (uint64_t)s->slots) : -1;
  const bool own_due = s->delay_us == 0 && n_due == s->due.size();
  if (own_due) deliver_slot = write_slot;
  if (counts8) {
    if (hipMemsetAsync(g.counters, 0, 64, stream) != hipSuccess) return AFE_ERR_HIP;
  } else g.counters = nullptr;
  const unsigned long long now = now_us, est_now = now_est;
  const int start = should_start ? 1 : 0, stop = should_stop ? 1 : 0;
  rc = for_each_launch(g.n, [&](dim3 grid) {
    if (g.t_update)
      hipLaunchKernelGGL((afe_stages_tick_kernel<double, true>), grid, dim3(kBlock), 0, stream, g, now, est_now, start, stop, write_slot, deliver_slot);
    else if (elem == 8)
      hipLaunchKernelGGL((afe_stages_tick_kernel<double, false>), grid, dim3(kBlock), 0, stream, g, now, est_now, start, stop, write_slot, deliver_slot);
    else
      hipLaunchKernelGGL((afe_stages_tick_kernel<float, false>), grid, dim3(kBlock), 0, stream, g, now, est_now, start, stop, write_slot, deliver_slot);
  });
  if (rc != AFE_OK) return rc;
  if (deliver_slot >= 0) {                                       // an onboard computer is told of the delivery (have_cmd above):
    afe::RadioMailbox mail;                                      // each vehicle's delivered type, type 0 was handed nothing
    afe::engine_mailbox(s->engine, &mail);
    rc = afe::onboard_stamp((void *)stream, mail, 0, g.n, now_us, -1, g.ring_type + (int64_t)deliver_slot * g.stride);
    if (rc != AFE_OK) return rc;
  }
  for (size_t k = 0; k < n_due; k++) s->due.pop_front();
  if (!own_due) s->due.push_back(now_us + s->delay_us);
  s->seq++;
  s->n_ticks++;
  if (counts8) {
    unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyAsync(c, g.counters, 64, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
      return AFE_ERR_HIP;
    for (int k = 0; k < 8; k++) counts8[k] = (int64_t)c[k];
  }
  return AFE_OK;
}

extern "C" int afe_stages_attach_gps_estimator(afe_stages *s, afe_gps_estimator *gps) {
  if (!s) return AFE_ERR_INVALID_ARG;
  if (gps) {
    const int rc = afe::gps_estimator_check_engine(gps, s->engine);
    if (rc != AFE_OK) return rc;
  }
  s->gps = gps;
  return AFE_OK;
}

extern "C" int afe_stages_selftest_math(int device, int op, int64_t n, const void *x, void *y) {
  if (!x || !y || op < 0 || op > 5 || n < 0) return AFE_ERR_INVALID_ARG;
  if (n == 0) return AFE_OK;
  if (n > kBlocksPerLaunch * kBlock) return AFE_ERR_OUT_OF_RANGE;
  const int prc = afe::pick_gfx950(device, &device);
  if (prc != AFE_OK) return prc;
  const size_t bytes = (size_t)n * (op < 2 ? 8 : 4);
  afe::DevBuf dx, dy;
  if (!dx.upload(x, bytes) || !dy.alloc(bytes)) { (void)hipGetLastError(); return AFE_ERR_HIP; }
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
  if (op < 2) hipLaunchKernelGGL(afe_stages_math_f64_kernel, grid, dim3(kBlock), 0, nullptr, op, n, dx.as<double>(), dy.as<double>());
  else hipLaunchKernelGGL(afe_stages_math_f32_kernel, grid, dim3(kBlock), 0, nullptr, op, n, dx.as<float>(), dy.as<float>());
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return AFE_ERR_HIP;
  return dy.download(y, bytes) ? AFE_OK : AFE_ERR_HIP;
}
