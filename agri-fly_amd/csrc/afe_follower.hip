// afe_follower.hip -- the trajectory follower: the offboard side of the radio on the device.  Plan adoption, the tracking
// reference, the tracking controller, the radio codec and the communications delay, one lane per vehicle, reading the
// engine's slabs and writing its rates-command slab.  The C ABI is in include/agrifly_engine.h ("trajectory follower").
// No step kernel knows about it: what it delivers is what afe_set_rates_commands would have uploaded.
//
// THE DEFINITION (tests/follower_checker.py restates it in numpy, operation for operation; kernels and checker must give
// the same bits, so the ORDER of the operations below is part of the contract).  Contraction is off everywhere; + - * /
// sqrt and the conversions are correctly rounded on gfx950 and in numpy.  Only sinf, cosf, asinf, acosf (float) and acos
// (double) are the device library's own: afe_follower_selftest_math evaluates the fm_ helpers of afe_offboard_math.h (where
// the quaternion, matrix and codec forms named below live, shared with afe_stages.hip) for a host that wants the device's values.
//
//   STATE READ    X = anchor_x + (double)px, Y = anchor_y + (double)py, Z = (double)pz (as afe_get_state forms them);
//                 velocity and attitude widened to double.  Nothing is normalised.
//   QUATERNIONS   a * b is Rotation.hpp:124-131 with this = a, r1 = b; inv(q) = (q0, -q1, -q2, -q3); M(q) is the 3x3 of
//                 Rotation.hpp:196-220; M v = (M0 x + M1 y) + M2 z per row, left to right.
//
//   PLANNER INPUTS (main.cpp:490-495; the acceleration is the vehicle's own, thrust along body z, as tests/orchard_flight.py
//   forms it):    cam = att * mount     Mi = M(inv(cam))     Ma = M(att)
//                 vel0 = Mi vel         acc0 = Mi (Ma2 T, Ma5 T, Ma8 T - 9.81), T = previous_thrust
//                 grav = Mi (0, 0, -9.81)                    cost = Mi (goal - (X, Y, Z))
//
//   REFERENCE (main.cpp:558-608), double:
//                 tt = (double)(now - t_plan_us) * 1e-6  (the difference as uint64)     running = planned && tt < tf
//                 te = running ? tt + lookahead : tf
//                 p, v, a = the Horner forms of planned_trajectory.hpp at te; araw = a; v = a = +0 when not running
//                 if p.z < 0: p.z = 0, v.z = 0 if v.z < 0, a.z = 0 if a.z < 0
//                 Mt = M(trajAtt)      refPos = Mt p + offset      refVel = Mt v      refAcc = Mt a
//                 thrust = sqrt(d.d), d = araw - g                 (d.d = (dx dx + dy dy) + dz dz)
//                 n0 = f0 / |f0|, f0 = a(te) - g;  n1 the same at te + omega_step;  c = n0 x n1 (Vec3.hpp:106-109), len = |c|
//                 dot = n0.n1;  omega = +0 if len <= 1e-6 or not dot < 1, else (acos(dot) / omega_step) * (c / len)
//                 refAngVel = M(inv(att) * trajAtt) omega
//                 not planned: refPos = hold, refVel = refAcc = refAngVel = +0, thrust = hover_thrust, running = 0
//
//   CONTROLLER (QuadcopterController.cpp:76-132, QuadcopterPositionController.hpp:22-28, QuadcopterAttitudeController.hpp:
//   35-68, desired yaw 0), float unless said otherwise; pf, vf, qf, rp, rv = float(X..), float(vel), float(att),
//   float(refPos), float(refVel):
//                 accErr = ((rp - pf) * w) * w + (((rv - vf) * 2) * w) * z + 0
//                 bz = M(qf) (0, 0, 1)        cmdThrust = thrust + double(accErr . bz)                       (double)
//                 s = (refAcc + double(accErr)) + double(0, 0, 9.81f)  (double)   nrm = float(sqrt(s.s))
//                 dir = float(s / double(nrm))       cosA = dir . (0, 0, 1)
//                 angle = cosA >= 1 ? 0 : cosA <= -1 ? float(pi) : acosf(cosA)
//                 ax = (0, 0, 1) x dir        n = |ax|
//                 refAtt = identity if n < 1e-6f, else FromRotationVector(ax * (angle / n)) (Rotation.hpp:84-97; identity
//                 below 4.84813681e-6f) and then refAtt * identity
//                 err = inv(refAtt) * qf      rot = ToRotationVector(err) (Rotation.hpp:144-161; the norm is held at 1 for
//                 asinf, as tests/offboard_stub.py does)
//                 zb = M(inv(err)) (0, 0, 1)  rax = zb x (0, 0, 1)  cosR = zb . (0, 0, 1)
//                 an = cosR >= 1 ? 0 : cosR <= -1 ? float(pi) : acosf(cosR)       rax = 0 if |rax| < 1e-12f else rax / |rax|
//                 k3 = 1 / tc_z, k12 = 1 / tc_xy       angVelErr = (-k3) * rot - ((k12 - k3) * an) * rax
//                 cmdAngVel = refAngVel + double(angVelErr)  (double)        previous_thrust = cmdThrust
//                 computed = float(cmdThrust), float(cmdAngVel)
//   CODEC         sent = each of the four through encodeToRadioByte / decodeFromRadioBytes with limit 35
//                 (RadioTypes.hpp:73-116, afe_codecs.cpp): saturation codes, the 65536 -> 0 wrap and NaN -> 0 included
//   DELAY LINE    (CommunicationsDelay.hpp:18-33) the message goes into the ring; due = now + delay_us.  Due times are the
//                 same for all vehicles: the host keeps them and hands the kernel the slot to write and the slot to deliver.
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

// the quaternion, matrix and codec helpers, the device library's functions (fm_*) and load_state: shared with the flight
// stage machine (afe_stages.hip)
using namespace afe_offboard;

constexpr int kBlock = 256;
constexpr int kMaxSlots = 16;
constexpr int64_t kBlocksPerLaunch = int64_t(1) << 22;   // a launch stays below 2^31 threads
constexpr int kRefWords = 14;

// planned_trajectory.hpp:42-51, one axis: k5 .. k0 are coefficients [0..5] of that axis
struct Poly1 { double k5, k4, k3, k2, k1, k0; };
__device__ __forceinline__ double poly_pos(const Poly1 &c, double t) {
#pragma clang fp contract(off)
  return ((((c.k5 * t + c.k4) * t + c.k3) * t + c.k2) * t + c.k1) * t + c.k0;
}
__device__ __forceinline__ double poly_vel(const Poly1 &c, double t) {
#pragma clang fp contract(off)
  return (((5 * c.k5 * t + 4 * c.k4) * t + 3 * c.k3) * t + 2 * c.k2) * t + c.k1;
}
__device__ __forceinline__ double poly_acc(const Poly1 &c, double t) {
#pragma clang fp contract(off)
  return ((20 * c.k5 * t + 12 * c.k4) * t + 6 * c.k3) * t + 2 * c.k2;
}
// planned_trajectory.hpp:26-29
__device__ __forceinline__ V3 traj_normal(const Poly1 &cx, const Poly1 &cy, const Poly1 &cz, const V3 &g, double t) {
#pragma clang fp contract(off)
  V3 f;
  f.x = poly_acc(cx, t) - g.x; f.y = poly_acc(cy, t) - g.y; f.z = poly_acc(cz, t) - g.z;
  const double len = sqrt(v_dot(f, f));
  V3 o;
  o.x = f.x / len; o.y = f.y / len; o.z = f.z / len;
  return o;
}
// planned_trajectory.hpp:30-39
__device__ __forceinline__ V3 traj_omega(const Poly1 &cx, const Poly1 &cy, const Poly1 &cz, const V3 &g, double t, double step) {
#pragma clang fp contract(off)
  const V3 n0 = traj_normal(cx, cy, cz, g, t), n1 = traj_normal(cx, cy, cz, g, t + step);
  const V3 turn = v_cross(n0, n1);
  const double len = sqrt(v_dot(turn, turn));
  const double dot = v_dot(n0, n1);
  V3 o;
  o.x = 0.0; o.y = 0.0; o.z = 0.0;
  if (len <= 1e-6 || !(dot < 1.0)) return o;
  const double rate = fm_acos(dot) / step;
  o.x = rate * (turn.x / len); o.y = rate * (turn.y / len); o.z = rate * (turn.z / len);
  return o;
}

struct Tuning {
  double lookahead, omega_step, hover_thrust;
  float nat_freq, damping, tc_xy, tc_z;
  double mount[4];
};

struct FollowerArgs {
  // the engine's slabs: planar, `stride` elements between components
  const void *pos, *vel, *att;
  const double *anchor_xy;
  float *rates_cmd;
  uint8_t *have_cmd;
  int64_t stride, n;
  // the follower's own slabs, the same stride
  uint8_t *planned;
  double *coeffs;            // [18]: coeffs[6][3] of afe_plan_output, row-major
  double *tf;
  unsigned long long *t_plan_us;
  double *traj_att;          // [4]
  double *offset, *grav, *hold, *goal;   // [3] each
  double *prev_thrust;
  float *computed, *sent;    // [4] each
  float *ring;               // [slots][4]
  double *ref;               // [14]: what the last tick tracked
  // planner inputs and what goes with them: planar [3][n] / [4][n], as the planner reads them
  double *in_vel, *in_acc, *in_grav, *in_cost, *in_pos, *in_cam;
  unsigned long long *counter;
  Tuning tune;
};

template <typename T>
__global__ void __launch_bounds__(kBlock) afe_follower_init_kernel(FollowerArgs g, int slots) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= g.n) return;
  const int64_t S = g.stride;
  V3 p, vel;
  Q4 q;
  load_state<T>(g, v, p, vel, q);
  g.planned[v] = 0;
  for (int k = 0; k < 18; k++) g.coeffs[k * S + v] = 0.0;
  g.tf[v] = 0.0;
  g.t_plan_us[v] = 0;
  g.traj_att[v] = 1.0; g.traj_att[S + v] = 0.0; g.traj_att[2 * S + v] = 0.0; g.traj_att[3 * S + v] = 0.0;
  g.offset[v] = 0.0; g.offset[S + v] = 0.0; g.offset[2 * S + v] = 0.0;
  g.grav[v] = 0.0; g.grav[S + v] = 0.0; g.grav[2 * S + v] = 0.0;
  g.hold[v] = p.x; g.hold[S + v] = p.y; g.hold[2 * S + v] = p.z;        // hold and goal: where the vehicle is now
  g.goal[v] = p.x; g.goal[S + v] = p.y; g.goal[2 * S + v] = p.z;
  g.prev_thrust[v] = g.tune.hover_thrust;
  for (int k = 0; k < 4; k++) { g.computed[k * S + v] = 0.0f; g.sent[k * S + v] = 0.0f; }
  for (int k = 0; k < 4 * slots; k++) g.ring[k * S + v] = 0.0f;
  for (int k = 0; k < kRefWords; k++) g.ref[k * S + v] = 0.0;
}

// main.cpp:490-495 and the goal vector, for the planner; camera attitude and position as they stand, for the adoption
template <typename T>
__global__ void __launch_bounds__(kBlock) afe_follower_inputs_kernel(FollowerArgs g) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= g.n) return;
  const int64_t S = g.stride, N = g.n;
  V3 p, vel;
  Q4 q;
  load_state<T>(g, v, p, vel, q);
  Q4 mount;
  mount.w = g.tune.mount[0]; mount.x = g.tune.mount[1]; mount.y = g.tune.mount[2]; mount.z = g.tune.mount[3];
  const Q4 cam = q_mul(q, mount);
  const M9 Mi = q_matrix(q_inv(cam)), Ma = q_matrix(q);
  const double thrust = g.prev_thrust[v];
  V3 aw, gw, to;
  aw.x = Ma.m[2] * thrust; aw.y = Ma.m[5] * thrust; aw.z = Ma.m[8] * thrust - 9.81;
  gw.x = 0.0; gw.y = 0.0; gw.z = -9.81;
  to.x = g.goal[v] - p.x; to.y = g.goal[S + v] - p.y; to.z = g.goal[2 * S + v] - p.z;
  const V3 v0 = m_rotate(Mi, vel), a0 = m_rotate(Mi, aw), gc = m_rotate(Mi, gw), cc = m_rotate(Mi, to);
  g.in_vel[v] = v0.x; g.in_vel[N + v] = v0.y; g.in_vel[2 * N + v] = v0.z;
  g.in_acc[v] = a0.x; g.in_acc[N + v] = a0.y; g.in_acc[2 * N + v] = a0.z;
  g.in_grav[v] = gc.x; g.in_grav[N + v] = gc.y; g.in_grav[2 * N + v] = gc.z;
  g.in_cost[v] = cc.x; g.in_cost[N + v] = cc.y; g.in_cost[2 * N + v] = cc.z;
  g.in_pos[v] = p.x; g.in_pos[N + v] = p.y; g.in_pos[2 * N + v] = p.z;
  g.in_cam[v] = cam.w; g.in_cam[N + v] = cam.x; g.in_cam[2 * N + v] = cam.y; g.in_cam[3 * N + v] = cam.z;
}

// main.cpp:518-528: a vehicle whose planner found something takes the plan over, the others keep what they had
__global__ void __launch_bounds__(kBlock) afe_follower_adopt_kernel(FollowerArgs g, const afe_plan_output *out, unsigned long long now_us) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t S = g.stride, N = g.n;
  bool found = false;
  if (v < g.n) {
    const afe_plan_output &o = out[v];
    found = o.found != 0;
    if (found) {
      for (int k = 0; k < 18; k++) g.coeffs[k * S + v] = o.coeffs[k / 3][k % 3];
      g.tf[v] = o.tf;
      g.t_plan_us[v] = now_us;
      for (int k = 0; k < 4; k++) g.traj_att[k * S + v] = g.in_cam[k * N + v];
      for (int k = 0; k < 3; k++) {
        g.offset[k * S + v] = g.in_pos[k * N + v];
        g.grav[k * S + v] = g.in_grav[k * N + v];
      }
      g.planned[v] = 1;
    }
  }
  const unsigned long long mask = __ballot(found);
  if ((threadIdx.x & 63) == 0 && mask) atomicAdd(g.counter, (unsigned long long)__popcll(mask));
}

struct Reference {
  V3 pos, vel, acc, ang_vel;
  double thrust;
  bool running;
};

__device__ __forceinline__ Reference tracking_reference(const FollowerArgs &g, int64_t v, const Q4 &att, unsigned long long now_us) {
#pragma clang fp contract(off)
  const int64_t S = g.stride;
  Reference r;
  r.vel.x = r.vel.y = r.vel.z = 0.0;
  r.acc = r.vel; r.ang_vel = r.vel;
  r.running = false;
  if (!g.planned[v]) {
    r.pos.x = g.hold[v]; r.pos.y = g.hold[S + v]; r.pos.z = g.hold[2 * S + v];
    r.thrust = g.tune.hover_thrust;
    return r;
  }
  const double *C = g.coeffs + v;
  Poly1 cx, cy, cz;
  cx.k5 = C[0 * S]; cy.k5 = C[1 * S]; cz.k5 = C[2 * S];
  cx.k4 = C[3 * S]; cy.k4 = C[4 * S]; cz.k4 = C[5 * S];
  cx.k3 = C[6 * S]; cy.k3 = C[7 * S]; cz.k3 = C[8 * S];
  cx.k2 = C[9 * S]; cy.k2 = C[10 * S]; cz.k2 = C[11 * S];
  cx.k1 = C[12 * S]; cy.k1 = C[13 * S]; cz.k1 = C[14 * S];
  cx.k0 = C[15 * S]; cy.k0 = C[16 * S]; cz.k0 = C[17 * S];
  const double tf = g.tf[v];
  const double tt = (double)(now_us - g.t_plan_us[v]) * 1e-6;
  r.running = tt < tf;
  const double te = r.running ? tt + g.tune.lookahead : tf;
  V3 p, vel, acc, araw, grav, off;
  p.x = poly_pos(cx, te); p.y = poly_pos(cy, te); p.z = poly_pos(cz, te);
  vel.x = poly_vel(cx, te); vel.y = poly_vel(cy, te); vel.z = poly_vel(cz, te);
  araw.x = poly_acc(cx, te); araw.y = poly_acc(cy, te); araw.z = poly_acc(cz, te);
  acc = araw;
  if (!r.running) { vel.x = vel.y = vel.z = 0.0; acc = vel; }
  if (p.z < 0.0) {
    p.z = 0.0;
    if (vel.z < 0.0) vel.z = 0.0;
    if (acc.z < 0.0) acc.z = 0.0;
  }
  Q4 ta;
  ta.w = g.traj_att[v]; ta.x = g.traj_att[S + v]; ta.y = g.traj_att[2 * S + v]; ta.z = g.traj_att[3 * S + v];
  grav.x = g.grav[v]; grav.y = g.grav[S + v]; grav.z = g.grav[2 * S + v];
  off.x = g.offset[v]; off.y = g.offset[S + v]; off.z = g.offset[2 * S + v];
  const M9 Mt = q_matrix(ta);
  const V3 rp = m_rotate(Mt, p);
  r.pos.x = rp.x + off.x; r.pos.y = rp.y + off.y; r.pos.z = rp.z + off.z;
  r.vel = m_rotate(Mt, vel);
  r.acc = m_rotate(Mt, acc);
  V3 d;
  d.x = araw.x - grav.x; d.y = araw.y - grav.y; d.z = araw.z - grav.z;
  r.thrust = sqrt(v_dot(d, d));
  const V3 om = traj_omega(cx, cy, cz, grav, te, g.tune.omega_step);
  r.ang_vel = m_rotate(q_matrix(q_mul(q_inv(att), ta)), om);
  return r;
}

struct Command {
  double thrust;
  V3 ang_vel;
};

// QuadcopterController::RunTracking, QuadcopterController.cpp:76-132, desired yaw 0
__device__ __forceinline__ Command run_tracking(const Tuning &t, const V3 &pos, const V3 &vel, const Q4 &att, const Reference &r) {
#pragma clang fp contract(off)
  V3f pf, vf, rp, rv;
  pf.x = (float)pos.x; pf.y = (float)pos.y; pf.z = (float)pos.z;
  vf.x = (float)vel.x; vf.y = (float)vel.y; vf.z = (float)vel.z;
  rp.x = (float)r.pos.x; rp.y = (float)r.pos.y; rp.z = (float)r.pos.z;
  rv.x = (float)r.vel.x; rv.y = (float)r.vel.y; rv.z = (float)r.vel.z;
  Q4f qf;
  qf.w = (float)att.w; qf.x = (float)att.x; qf.y = (float)att.y; qf.z = (float)att.z;
  const float w = t.nat_freq, z = t.damping;
  V3f accErr;
  accErr.x = ((rp.x - pf.x) * w) * w + (((rv.x - vf.x) * 2) * w) * z + 0.0f;
  accErr.y = ((rp.y - pf.y) * w) * w + (((rv.y - vf.y) * 2) * w) * z + 0.0f;
  accErr.z = ((rp.z - pf.z) * w) * w + (((rv.z - vf.z) * 2) * w) * z + 0.0f;
  V3f e3;
  e3.x = 0.0f; e3.y = 0.0f; e3.z = 1.0f;
  const V3f bz = mf_rotate(qf_matrix(qf), e3);
  Command c;
  c.thrust = r.thrust + (double)vf_dot(accErr, bz);
  V3 s;
  s.x = (r.acc.x + (double)accErr.x) + (double)0.0f;
  s.y = (r.acc.y + (double)accErr.y) + (double)0.0f;
  s.z = (r.acc.z + (double)accErr.z) + (double)9.81f;
  const float nrm = (float)sqrt(v_dot(s, s));
  V3f dir;
  dir.x = (float)(s.x / (double)nrm); dir.y = (float)(s.y / (double)nrm); dir.z = (float)(s.z / (double)nrm);
  Q4f ident;
  ident.w = 1.0f; ident.x = 0.0f; ident.y = 0.0f; ident.z = 0.0f;
  const Q4f refAtt = qf_mul(tilt_attitude(dir), ident);                  // * FromRotationVector((0, 0, yaw = 0))
  const V3f we = desired_angular_velocity(refAtt, qf, t.tc_xy, t.tc_z);
  c.ang_vel.x = r.ang_vel.x + (double)we.x;
  c.ang_vel.y = r.ang_vel.y + (double)we.y;
  c.ang_vel.z = r.ang_vel.z + (double)we.z;
  return c;
}

// One offboard period: reference, controller, codec, delay line.  write_slot: where this tick's message goes;
// deliver_slot: the newest message that is due (-1: none) -- it becomes the engine's rates command.
// ANNOUNCE (an estimator is attached, and the state read is its prediction): SetPredictedValues(cmdAngVel, att * e3 * cmdThrust
// - (0, 0, 9.81)), main.cpp:647-649, the doubles before any narrowing, into the estimator's ring slot `announce` (acc 3, angVel 3).
template <typename T, bool ANNOUNCE>
__global__ void __launch_bounds__(kBlock) afe_follower_tick_kernel(FollowerArgs g, unsigned long long now_us, int write_slot, int deliver_slot,
                                                                   double *announce) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t S = g.stride;
  bool running = false;
  if (v < g.n) {
    V3 p, vel;
    Q4 q;
    load_state<T>(g, v, p, vel, q);
    const Reference r = tracking_reference(g, v, q, now_us);
    running = r.running;
    const Command c = run_tracking(g.tune, p, vel, q, r);
    g.prev_thrust[v] = c.thrust;
    if (ANNOUNCE) {
      V3 e3;
      e3.x = 0.0; e3.y = 0.0; e3.z = 1.0;
      const V3 up = m_rotate(q_matrix(q), e3);
      double *A = announce + v;
      A[0 * S] = up.x * c.thrust - 0.0; A[1 * S] = up.y * c.thrust - 0.0; A[2 * S] = up.z * c.thrust - 9.81;
      A[3 * S] = c.ang_vel.x; A[4 * S] = c.ang_vel.y; A[5 * S] = c.ang_vel.z;
    }
    float cmd[4], sent[4];
    cmd[0] = (float)c.thrust; cmd[1] = (float)c.ang_vel.x; cmd[2] = (float)c.ang_vel.y; cmd[3] = (float)c.ang_vel.z;
#pragma unroll
    for (int k = 0; k < 4; k++) sent[k] = radio_quantise35(cmd[k]);
    float due[4];
#pragma unroll
    for (int k = 0; k < 4; k++) due[k] = sent[k];
    if (deliver_slot >= 0 && deliver_slot != write_slot) {
#pragma unroll
      for (int k = 0; k < 4; k++) due[k] = g.ring[((int64_t)deliver_slot * 4 + k) * S + v];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      g.computed[k * S + v] = cmd[k];
      g.sent[k * S + v] = sent[k];
      g.ring[((int64_t)write_slot * 4 + k) * S + v] = sent[k];
    }
    if (deliver_slot >= 0) {
#pragma unroll
      for (int k = 0; k < 4; k++) g.rates_cmd[k * S + v] = due[k];
      g.have_cmd[v] = 1;
    }
    double *R = g.ref + v;
    R[0 * S] = r.pos.x; R[1 * S] = r.pos.y; R[2 * S] = r.pos.z;
    R[3 * S] = r.vel.x; R[4 * S] = r.vel.y; R[5 * S] = r.vel.z;
    R[6 * S] = r.acc.x; R[7 * S] = r.acc.y; R[8 * S] = r.acc.z;
    R[9 * S] = r.thrust;
    R[10 * S] = r.ang_vel.x; R[11 * S] = r.ang_vel.y; R[12 * S] = r.ang_vel.z;
    R[13 * S] = r.running ? 1.0 : 0.0;
  }
  if (g.counter) {
    const unsigned long long mask = __ballot(running);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(g.counter, (unsigned long long)__popcll(mask));
  }
}

__global__ void __launch_bounds__(kBlock) afe_follower_math_f32_kernel(int op, int64_t n, const float *x, float *y) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float s, c;
  fm_sincosf(x[i], &s, &c);
  y[i] = op == 0 ? s : op == 1 ? c : op == 2 ? fm_asinf(x[i]) : fm_acosf(x[i]);
}
__global__ void __launch_bounds__(kBlock) afe_follower_math_f64_kernel(int64_t n, const double *x, double *y) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  y[i] = fm_acos(x[i]);
}

size_t up256(size_t x) { return (x + 255) & ~size_t(255); }
bool range_bad(int64_t first, int64_t count) { return first < 0 || count < 0; }

// QuadcopterConstants.hpp: posControl_natFreq, posControl_damping, attControl_timeConst_xy, attControl_timeConst_z
bool tuning_row(int type, float *nat_freq, float *damping, float *tc_xy, float *tc_z) {
  *nat_freq = 2.0f; *damping = 0.7f;                                     // :34-35, :222-223
  switch (type) {
    case 1: *tc_xy = 0.40f; *tc_z = 1.0f; return true;                   // :81, :39
    case 2: *tc_xy = 0.20f; *tc_z = 1.0f; return true;                   // :37, :39
    case 4: *tc_xy = 0.0914f; *tc_z = 0.5089f; return true;              // :185, :187
    case 5: {                                                            // :225-228, derived in float
      const float av_xy = 0.04f, av_z = av_xy * 5;
      *tc_xy = av_xy * 2; *tc_z = av_z * 2;
      return true;
    }
    default: return false;
  }
}

}  // namespace

struct afe_follower {
  afe_engine *engine = nullptr;     // borrowed
  int device = 0;
  int64_t n = 0, stride = 0;
  int slots = 0;
  uint64_t period_us = 0, delay_us = 0;
  uint64_t n_ticks = 0, seq = 0;    // seq: messages sent so far; message k lives in slot k % slots
  std::deque<uint64_t> due;         // due times of the messages in flight, in send order (the oldest is message seq - size)
  afe_estimator *est = nullptr;     // borrowed; attached: the state read is its prediction, and a tick announces to it
  afe_gps_estimator *gps = nullptr; // borrowed; attached: the state read is its estimate, and nothing is announced
  afe::DevBuf arena;
  FollowerArgs args;                // the follower's part of the kernel arguments
};

namespace {

// estimated: the call reads estState -- with an estimator attached that is its prediction buffer, which looks like an fp64
// engine's slabs with anchors of +0, so the <double> kernels read it as they read the truth
int enter(afe_follower *f, hipStream_t *stream, FollowerArgs *g, int *elem, bool want_cmd_slabs, bool estimated = false) {
  afe::EngineAccess acc;
  const int rc = afe::engine_enter(f->engine, &acc);
  if (rc != AFE_OK) return rc;
  const afe_device_view &view = acc.view;
  if (view.n_vehicles != f->n || view.stride != f->stride || acc.device != f->device) return AFE_ERR_INVALID_ARG;
  *stream = acc.stream;
  *g = f->args;
  g->pos = view.pos; g->vel = view.vel; g->att = view.att;
  g->anchor_xy = view.pos_anchor_xy;
  *elem = view.state_elem_size;
  if (estimated && f->est) {
    uint64_t now_us = 0;
    int rc = afe_time_us(f->engine, &now_us);
    if (rc != AFE_OK) return rc;
    afe::EstimatorLink link;
    rc = afe::estimator_link(f->est, now_us, &link);
    if (rc != AFE_OK) return rc;
    g->pos = link.pos; g->vel = link.vel; g->att = link.att;
    g->anchor_xy = link.zero_anchor_xy;
    *elem = 8;
  }
  if (estimated && f->gps) {                                   // EstGetState: GetCurrentEstimate(), no prediction ahead
    uint64_t n_ticks = 0;
    int rc = afe_logic_ticks(f->engine, &n_ticks);
    if (rc != AFE_OK) return rc;
    afe::EstimatorLink link;
    rc = afe::gps_estimator_link(f->gps, n_ticks, &link);
    if (rc != AFE_OK) return rc;
    g->pos = link.pos; g->vel = link.vel; g->att = link.att;
    g->anchor_xy = link.zero_anchor_xy;
    *elem = 8;
  }
  if (want_cmd_slabs) return afe::engine_rates_slabs(f->engine, &g->rates_cmd, &g->have_cmd);
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

// host planar [comps][count] <-> the follower's planar [comps][stride] at `first`; the stream has been waited for
bool put_rows(void *dev, size_t esz, int comps, int64_t stride, int64_t first, int64_t count, const void *host) {
  return hipMemcpy2D((char *)dev + (size_t)first * esz, (size_t)stride * esz, host, (size_t)count * esz, (size_t)count * esz, (size_t)comps,
                     hipMemcpyHostToDevice) == hipSuccess;
}
bool get_rows(const void *dev, size_t esz, int comps, int64_t stride, int64_t first, int64_t count, void *host) {
  return hipMemcpy2D(host, (size_t)count * esz, (const char *)dev + (size_t)first * esz, (size_t)stride * esz, (size_t)count * esz, (size_t)comps,
                     hipMemcpyDeviceToHost) == hipSuccess;
}

// [first, first + count) against the follower, nothing touched
int enter_rows(afe_follower *f, int64_t first, int64_t count) {
  if (!f || range_bad(first, count)) return AFE_ERR_INVALID_ARG;
  if (first > f->n || count > f->n - first) return AFE_ERR_OUT_OF_RANGE;   // (no sum: it can wrap)
  return AFE_OK;
}
// through the engine's gate, then its stream drained: the copies that follow are synchronous
int drain(afe_follower *f) {
  hipStream_t stream = nullptr;
  FollowerArgs g;
  int elem = 0;
  const int rc = enter(f, &stream, &g, &elem, false);
  if (rc != AFE_OK) return rc;
  return hipStreamSynchronize(stream) == hipSuccess ? AFE_OK : AFE_ERR_HIP;
}

int launch_inputs(const FollowerArgs &g, int elem, hipStream_t stream) {
  return for_each_launch(g.n, [&](dim3 grid) {
    if (elem == 8) hipLaunchKernelGGL(afe_follower_inputs_kernel<double>, grid, dim3(kBlock), 0, stream, g);
    else hipLaunchKernelGGL(afe_follower_inputs_kernel<float>, grid, dim3(kBlock), 0, stream, g);
  });
}

struct AdoptCtx {
  afe_follower *f;
  FollowerArgs g;
  hipStream_t stream;
  uint64_t now_us;
  int64_t n_found;
};

// called by the planner's host side while it still holds its scratch: the plans are in `dev_out`
int adopt_plans(void *ctx_, const afe_plan_output *dev_out) {
  AdoptCtx *ctx = (AdoptCtx *)ctx_;
  const FollowerArgs &g = ctx->g;
  hipStream_t stream = ctx->stream;
  if (hipMemsetAsync(g.counter, 0, 8, stream) != hipSuccess) return AFE_ERR_HIP;
  const int rc = for_each_launch(g.n, [&](dim3 grid) {
    hipLaunchKernelGGL(afe_follower_adopt_kernel, grid, dim3(kBlock), 0, stream, g, dev_out, (unsigned long long)ctx->now_us);
  });
  if (rc != AFE_OK) return rc;
  unsigned long long found = 0;
  if (hipMemcpyAsync(&found, g.counter, 8, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
    return AFE_ERR_HIP;
  ctx->n_found = (int64_t)found;
  return AFE_OK;
}

}  // namespace

extern "C" int afe_follower_ring_slots(uint64_t period_us, uint64_t delay_us, int *slots) {
  if (!slots) return AFE_ERR_INVALID_ARG;
  if (period_us == 0) return AFE_ERR_OUT_OF_RANGE;
  const uint64_t k = delay_us / period_us;
  if (k > (uint64_t)(kMaxSlots - 2)) return AFE_ERR_OUT_OF_RANGE;
  *slots = (int)k + 2;
  return AFE_OK;
}

extern "C" int afe_follower_default_config(int quadcopter_type, afe_follower_config *cfg) {
  if (!cfg) return AFE_ERR_INVALID_ARG;
  afe_follower_config c;
  std::memset(&c, 0, sizeof(c));
  if (!tuning_row(quadcopter_type, &c.nat_freq, &c.damping, &c.att_time_const_xy, &c.att_time_const_z)) return AFE_ERR_INVALID_ARG;
  c.struct_bytes = sizeof(c);
  c.period_us = 10000;
  c.delay_us = 30000;
  c.lookahead_s = 0.04;      // main.cpp:567
  c.omega_step_s = 0.02;     // main.cpp:601
  const int rc = afe_camera_default_mount(c.mount);
  if (rc != AFE_OK) return rc;
  c.hover_thrust = 9.81;
  *cfg = c;
  return AFE_OK;
}

extern "C" int afe_follower_create(afe_engine *e, const afe_follower_config *cfg, afe_follower **out) {
  if (!e || !cfg || !out || cfg->struct_bytes < sizeof(afe_follower_config)) return AFE_ERR_INVALID_ARG;
  if (!(cfg->att_time_const_xy > 0) || !(cfg->att_time_const_z > 0) || !std::isfinite(cfg->nat_freq) || !std::isfinite(cfg->damping) ||
      !std::isfinite(cfg->lookahead_s) || !(cfg->omega_step_s > 0) || !std::isfinite(cfg->hover_thrust))
    return AFE_ERR_INVALID_ARG;
  for (int k = 0; k < 4; k++) if (!std::isfinite(cfg->mount[k])) return AFE_ERR_INVALID_ARG;
  int slots = 0;
  int rc = afe_follower_ring_slots(cfg->period_us, cfg->delay_us, &slots);
  if (rc != AFE_OK) return rc;
  afe::EngineAccess acc;
  rc = afe::engine_enter(e, &acc);
  if (rc != AFE_OK) return rc;
  float *rates_cmd = nullptr;
  uint8_t *have_cmd = nullptr;
  rc = afe::engine_rates_slabs(e, &rates_cmd, &have_cmd);
  if (rc != AFE_OK) return rc;
  afe_follower *f = new afe_follower();
  f->engine = e; f->device = acc.device; f->n = acc.view.n_vehicles; f->stride = acc.view.stride;
  f->slots = slots; f->period_us = cfg->period_us; f->delay_us = cfg->delay_us;
  const size_t S = (size_t)f->stride, N = (size_t)std::max<int64_t>(f->n, 1);
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += up256(bytes); return o; };
  const size_t o_planned = take(S), o_coeffs = take(S * 18 * 8), o_tf = take(S * 8), o_tplan = take(S * 8), o_tatt = take(S * 4 * 8),
               o_off = take(S * 3 * 8), o_grav = take(S * 3 * 8), o_hold = take(S * 3 * 8), o_goal = take(S * 3 * 8), o_prev = take(S * 8),
               o_comp = take(S * 4 * 4), o_sent = take(S * 4 * 4), o_ring = take(S * 4 * 4 * (size_t)slots), o_ref = take(S * kRefWords * 8),
               o_iv = take(N * 3 * 8), o_ia = take(N * 3 * 8), o_ig = take(N * 3 * 8), o_ic = take(N * 3 * 8), o_ip = take(N * 3 * 8),
               o_iq = take(N * 4 * 8), o_cnt = take(8);
  if (!f->arena.alloc(off)) { (void)hipGetLastError(); delete f; return AFE_ERR_HIP; }
  unsigned char *A = f->arena.as<unsigned char>();
  std::memset(&f->args, 0, sizeof(f->args));
  FollowerArgs &g = f->args;
  g.n = f->n; g.stride = f->stride;
  g.planned = A + o_planned; g.coeffs = (double *)(A + o_coeffs); g.tf = (double *)(A + o_tf);
  g.t_plan_us = (unsigned long long *)(A + o_tplan); g.traj_att = (double *)(A + o_tatt);
  g.offset = (double *)(A + o_off); g.grav = (double *)(A + o_grav); g.hold = (double *)(A + o_hold); g.goal = (double *)(A + o_goal);
  g.prev_thrust = (double *)(A + o_prev); g.computed = (float *)(A + o_comp); g.sent = (float *)(A + o_sent);
  g.ring = (float *)(A + o_ring); g.ref = (double *)(A + o_ref);
  g.in_vel = (double *)(A + o_iv); g.in_acc = (double *)(A + o_ia); g.in_grav = (double *)(A + o_ig); g.in_cost = (double *)(A + o_ic);
  g.in_pos = (double *)(A + o_ip); g.in_cam = (double *)(A + o_iq);
  g.counter = (unsigned long long *)(A + o_cnt);
  g.tune.lookahead = cfg->lookahead_s; g.tune.omega_step = cfg->omega_step_s; g.tune.hover_thrust = cfg->hover_thrust;
  g.tune.nat_freq = cfg->nat_freq; g.tune.damping = cfg->damping; g.tune.tc_xy = cfg->att_time_const_xy; g.tune.tc_z = cfg->att_time_const_z;
  for (int k = 0; k < 4; k++) g.tune.mount[k] = cfg->mount[k];
  FollowerArgs run = g;
  run.pos = acc.view.pos; run.vel = acc.view.vel; run.att = acc.view.att; run.anchor_xy = acc.view.pos_anchor_xy;
  const hipStream_t stream = acc.stream;
  const int elem = acc.view.state_elem_size;
  rc = hipMemsetAsync(A, 0, off, stream) == hipSuccess ? AFE_OK : AFE_ERR_HIP;     // (the padding beyond n included)
  if (rc == AFE_OK)
    rc = for_each_launch(run.n, [&](dim3 grid) {
      if (elem == 8) hipLaunchKernelGGL(afe_follower_init_kernel<double>, grid, dim3(kBlock), 0, stream, run, slots);
      else hipLaunchKernelGGL(afe_follower_init_kernel<float>, grid, dim3(kBlock), 0, stream, run, slots);
    });
  if (rc == AFE_OK && hipStreamSynchronize(stream) != hipSuccess) rc = AFE_ERR_HIP;
  if (rc != AFE_OK) { (void)hipGetLastError(); (void)afe_follower_destroy(f); return rc; }
  *out = f;
  return AFE_OK;
}

extern "C" int afe_follower_destroy(afe_follower *f) {
  if (!f) return AFE_ERR_INVALID_ARG;
  (void)hipSetDevice(f->device);
  (void)hipDeviceSynchronize();
  delete f;
  return AFE_OK;
}

extern "C" int afe_follower_info(const afe_follower *f, int64_t *n_vehicles, int *slots, uint64_t *n_ticks, int *in_flight) {
  if (!f) return AFE_ERR_INVALID_ARG;
  if (n_vehicles) *n_vehicles = f->n;
  if (slots) *slots = f->slots;
  if (n_ticks) *n_ticks = f->n_ticks;
  if (in_flight) *in_flight = (int)f->due.size();
  return AFE_OK;
}

static int set_vec3(afe_follower *f, int64_t first, int64_t count, const double *pos3, bool goal) {
  const int arc = enter_rows(f, first, count);
  if (arc != AFE_OK) return arc;
  if (!pos3) return AFE_ERR_INVALID_ARG;
  if (count == 0) return AFE_OK;
  const int rc = drain(f);
  if (rc != AFE_OK) return rc;
  return put_rows(goal ? f->args.goal : f->args.hold, 8, 3, f->stride, first, count, pos3) ? AFE_OK : AFE_ERR_HIP;
}
extern "C" int afe_follower_set_hold(afe_follower *f, int64_t first, int64_t count, const double *pos3) { return set_vec3(f, first, count, pos3, false); }
extern "C" int afe_follower_set_goal(afe_follower *f, int64_t first, int64_t count, const double *pos3) { return set_vec3(f, first, count, pos3, true); }

extern "C" int afe_follower_set_plans(afe_follower *f, int64_t first, int64_t count, const uint8_t *planned, const double *coeffs, const double *tf,
                                      const uint64_t *t_plan_us, const double *traj_att4, const double *offset3, const double *grav3) {
  const int arc = enter_rows(f, first, count);
  if (arc != AFE_OK) return arc;
  if (!planned && !coeffs && !tf && !t_plan_us && !traj_att4 && !offset3 && !grav3) return AFE_ERR_INVALID_ARG;
  if (count == 0) return AFE_OK;
  const int rc = drain(f);
  if (rc != AFE_OK) return rc;
  const FollowerArgs &g = f->args;
  const int64_t S = f->stride;
  if ((planned && !put_rows(g.planned, 1, 1, S, first, count, planned)) || (coeffs && !put_rows(g.coeffs, 8, 18, S, first, count, coeffs)) ||
      (tf && !put_rows(g.tf, 8, 1, S, first, count, tf)) || (t_plan_us && !put_rows(g.t_plan_us, 8, 1, S, first, count, t_plan_us)) ||
      (traj_att4 && !put_rows(g.traj_att, 8, 4, S, first, count, traj_att4)) || (offset3 && !put_rows(g.offset, 8, 3, S, first, count, offset3)) ||
      (grav3 && !put_rows(g.grav, 8, 3, S, first, count, grav3)))
    return AFE_ERR_HIP;
  return AFE_OK;
}

extern "C" int afe_follower_get_plans(afe_follower *f, int64_t first, int64_t count, uint8_t *planned, double *coeffs, double *tf,
                                      uint64_t *t_plan_us, double *traj_att4, double *offset3, double *grav3) {
  const int arc = enter_rows(f, first, count);
  if (arc != AFE_OK) return arc;
  if (!planned && !coeffs && !tf && !t_plan_us && !traj_att4 && !offset3 && !grav3) return AFE_ERR_INVALID_ARG;
  if (count == 0) return AFE_OK;
  const int rc = drain(f);
  if (rc != AFE_OK) return rc;
  const FollowerArgs &g = f->args;
  const int64_t S = f->stride;
  if ((planned && !get_rows(g.planned, 1, 1, S, first, count, planned)) || (coeffs && !get_rows(g.coeffs, 8, 18, S, first, count, coeffs)) ||
      (tf && !get_rows(g.tf, 8, 1, S, first, count, tf)) || (t_plan_us && !get_rows(g.t_plan_us, 8, 1, S, first, count, t_plan_us)) ||
      (traj_att4 && !get_rows(g.traj_att, 8, 4, S, first, count, traj_att4)) || (offset3 && !get_rows(g.offset, 8, 3, S, first, count, offset3)) ||
      (grav3 && !get_rows(g.grav, 8, 3, S, first, count, grav3)))
    return AFE_ERR_HIP;
  return AFE_OK;
}

extern "C" int afe_follower_get_reference(afe_follower *f, int64_t first, int64_t count, double *ref14) {
  const int arc = enter_rows(f, first, count);
  if (arc != AFE_OK) return arc;
  if (!ref14) return AFE_ERR_INVALID_ARG;
  if (count == 0) return AFE_OK;
  const int rc = drain(f);
  if (rc != AFE_OK) return rc;
  return get_rows(f->args.ref, 8, kRefWords, f->stride, first, count, ref14) ? AFE_OK : AFE_ERR_HIP;
}

extern "C" int afe_follower_get_command(afe_follower *f, int64_t first, int64_t count, float *computed4, float *sent4) {
  const int arc = enter_rows(f, first, count);
  if (arc != AFE_OK) return arc;
  if (!computed4 && !sent4) return AFE_ERR_INVALID_ARG;
  if (count == 0) return AFE_OK;
  const int rc = drain(f);
  if (rc != AFE_OK) return rc;
  if ((computed4 && !get_rows(f->args.computed, 4, 4, f->stride, first, count, computed4)) ||
      (sent4 && !get_rows(f->args.sent, 4, 4, f->stride, first, count, sent4)))
    return AFE_ERR_HIP;
  return AFE_OK;
}

extern "C" int afe_follower_planner_inputs(afe_follower *f, double *vel0, double *acc0, double *grav, double *cost_vec) {
  if (!f || (!vel0 && !acc0 && !grav && !cost_vec)) return AFE_ERR_INVALID_ARG;
  if (f->n == 0) return AFE_OK;
  hipStream_t stream = nullptr;
  FollowerArgs g;
  int elem = 0;
  int rc = enter(f, &stream, &g, &elem, false, true);
  if (rc != AFE_OK) return rc;
  rc = launch_inputs(g, elem, stream);
  if (rc != AFE_OK) return rc;
  if (hipStreamSynchronize(stream) != hipSuccess) return AFE_ERR_HIP;
  const size_t bytes = (size_t)f->n * 24;
  if ((vel0 && hipMemcpy(vel0, g.in_vel, bytes, hipMemcpyDeviceToHost) != hipSuccess) ||
      (acc0 && hipMemcpy(acc0, g.in_acc, bytes, hipMemcpyDeviceToHost) != hipSuccess) ||
      (grav && hipMemcpy(grav, g.in_grav, bytes, hipMemcpyDeviceToHost) != hipSuccess) ||
      (cost_vec && hipMemcpy(cost_vec, g.in_cost, bytes, hipMemcpyDeviceToHost) != hipSuccess))
    return AFE_ERR_HIP;
  return AFE_OK;
}

extern "C" int afe_follower_plan(afe_follower *f, const afe_planner_config *cfg, const void *dev_depth_images, const double *samples,
                                 int n_candidates, afe_plan_output *out, uint8_t *flags, int64_t *n_found, float *kernel_ms) {
  if (!f || !cfg || !dev_depth_images || !samples || n_candidates <= 0) return AFE_ERR_INVALID_ARG;
  if (f->n == 0) { if (n_found) *n_found = 0; return AFE_OK; }
  AdoptCtx ctx;
  ctx.f = f; ctx.n_found = 0;
  int elem = 0;
  int rc = enter(f, &ctx.stream, &ctx.g, &elem, false, true);
  if (rc != AFE_OK) return rc;
  uint64_t now_us = 0;
  rc = afe_time_us(f->engine, &now_us);
  if (rc != AFE_OK) return rc;
  ctx.now_us = now_us;
  rc = launch_inputs(ctx.g, elem, ctx.stream);
  if (rc != AFE_OK) return rc;
  // the planner launches on the null stream, and a caller-owned stream may be non-blocking: the inputs must be there
  if (hipStreamSynchronize(ctx.stream) != hipSuccess) return AFE_ERR_HIP;
  afe::PlanDeviceIO io;
  io.vel0 = ctx.g.in_vel; io.acc0 = ctx.g.in_acc; io.grav = ctx.g.in_grav; io.cost_vec = ctx.g.in_cost;
  io.adopt = adopt_plans; io.ctx = &ctx;
  rc = afe::plan_device_resident(f->device, cfg, f->n, dev_depth_images, samples, n_candidates, io, out, flags, kernel_ms);
  if (rc != AFE_OK) return rc;
  if (n_found) *n_found = ctx.n_found;
  return AFE_OK;
}

extern "C" int afe_follower_tick(afe_follower *f, int64_t *n_tracking) {
  if (!f) return AFE_ERR_INVALID_ARG;
  hipStream_t stream = nullptr;
  FollowerArgs g;
  int elem = 0;
  int rc = enter(f, &stream, &g, &elem, true, true);
  if (rc != AFE_OK) return rc;
  uint64_t now_us = 0;
  rc = afe_time_us(f->engine, &now_us);
  if (rc != AFE_OK) return rc;
  double *announce = nullptr, announce_from = 0;
  if (f->est) {
    rc = afe::estimator_announce_begin(f->est, now_us, &announce, &announce_from);
    if (rc != AFE_OK) return rc;
  }
  // the delay line's bookkeeping (CommunicationsDelay.hpp:18-33): this tick's message is sent, then every message that
  // is due is delivered in send order -- the newest of them is what the vehicle is left with
  size_t n_due = 0;
  while (n_due < f->due.size() && f->due[n_due] <= now_us) n_due++;
  if (f->due.size() - n_due + 1 > (size_t)f->slots) return AFE_ERR_OUT_OF_RANGE;   // ticks closer together than the period: the ring is full
  const uint64_t oldest = f->seq - f->due.size();
  const int write_slot = (int)(f->seq % (uint64_t)f->slots);
  int deliver_slot = n_due ? (int)((oldest + n_due - 1) % (uint64_t)f->slots) : -1;
  const bool own_due = f->delay_us == 0 && n_due == f->due.size();
  if (own_due) deliver_slot = write_slot;
  if (n_tracking) {
    if (hipMemsetAsync(g.counter, 0, 8, stream) != hipSuccess) return AFE_ERR_HIP;
  } else g.counter = nullptr;
  if (f->n > 0) {
    rc = for_each_launch(g.n, [&](dim3 grid) {
      if (announce)
        hipLaunchKernelGGL((afe_follower_tick_kernel<double, true>), grid, dim3(kBlock), 0, stream, g, (unsigned long long)now_us, write_slot, deliver_slot, announce);
      else if (elem == 8)
        hipLaunchKernelGGL((afe_follower_tick_kernel<double, false>), grid, dim3(kBlock), 0, stream, g, (unsigned long long)now_us, write_slot, deliver_slot, announce);
      else
        hipLaunchKernelGGL((afe_follower_tick_kernel<float, false>), grid, dim3(kBlock), 0, stream, g, (unsigned long long)now_us, write_slot, deliver_slot, announce);
    });
    if (rc != AFE_OK) return rc;
    if (deliver_slot >= 0) {                                   // an onboard computer is told of the delivery (have_cmd = 1 above)
      afe::RadioMailbox mail;
      afe::engine_mailbox(f->engine, &mail);
      rc = afe::onboard_stamp((void *)stream, mail, 0, g.n, now_us, 5, nullptr);
      if (rc != AFE_OK) return rc;
    }
  }
  if (f->est) afe::estimator_announce_commit(f->est, announce_from);
  for (size_t k = 0; k < n_due; k++) f->due.pop_front();
  if (!own_due) f->due.push_back(now_us + f->delay_us);
  f->seq++;
  f->n_ticks++;
  if (n_tracking) {
    unsigned long long tracking = 0;
    if (hipMemcpyAsync(&tracking, g.counter, 8, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
      return AFE_ERR_HIP;
    *n_tracking = (int64_t)tracking;
  }
  return AFE_OK;
}

extern "C" int afe_follower_attach_estimator(afe_follower *f, afe_estimator *est) {
  if (!f) return AFE_ERR_INVALID_ARG;
  if (est) {
    if (f->gps) return AFE_ERR_INVALID_ARG;                    // one kind of estimator at a time
    const int rc = afe::estimator_check_engine(est, f->engine);
    if (rc != AFE_OK) return rc;
  }
  f->est = est;
  return AFE_OK;
}

extern "C" int afe_follower_attach_gps_estimator(afe_follower *f, afe_gps_estimator *gps) {
  if (!f) return AFE_ERR_INVALID_ARG;
  if (gps) {
    if (f->est) return AFE_ERR_INVALID_ARG;                    // one kind of estimator at a time
    const int rc = afe::gps_estimator_check_engine(gps, f->engine);
    if (rc != AFE_OK) return rc;
  }
  f->gps = gps;
  return AFE_OK;
}

extern "C" int afe_follower_selftest_math(int device, int op, int64_t n, const void *x, void *y) {
  if (!x || !y || op < 0 || op > 4 || n < 0) return AFE_ERR_INVALID_ARG;
  if (n == 0) return AFE_OK;
  if (n > kBlocksPerLaunch * kBlock) return AFE_ERR_OUT_OF_RANGE;
  const int prc = afe::pick_gfx950(device, &device);
  if (prc != AFE_OK) return prc;
  const size_t bytes = (size_t)n * (op == 4 ? 8 : 4);
  afe::DevBuf dx, dy;
  if (!dx.upload(x, bytes) || !dy.alloc(bytes)) { (void)hipGetLastError(); return AFE_ERR_HIP; }
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
  if (op == 4) hipLaunchKernelGGL(afe_follower_math_f64_kernel, grid, dim3(kBlock), 0, nullptr, n, dx.as<double>(), dy.as<double>());
  else hipLaunchKernelGGL(afe_follower_math_f32_kernel, grid, dim3(kBlock), 0, nullptr, op, n, dx.as<float>(), dy.as<float>());
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return AFE_ERR_HIP;
  return dy.download(y, bytes) ? AFE_OK : AFE_ERR_HIP;
}
