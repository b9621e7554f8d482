// afe_estimator.hip -- Offboard::MocapStateEstimator and its PredictionPipe for a whole ensemble on the device: the block of
// the Rappids_Simulator loop between the vehicle and the controller (main.cpp:451-457 UpdateWithMeasurement at 200 Hz,
// :468-469 GetPrediction(0.03), :647-649 SetPredictedValues).  One lane per vehicle, reading the engine's slabs; the
// trajectory follower (afe_follower.hip) reads the prediction buffer in place of the truth when one is attached.  The C ABI
// is in include/agrifly_engine.h ("mocap state estimator").
//
// THE DEFINITION is cli/mocap_estimator.hpp, line by line (tests/offboard_reference.py is the same in scalar Python and
// tests/estimator_checker.py restates it in numpy, vectorised; kernels and checker must give the same bits, so the ORDER
// of the operations is part of the contract).  All arithmetic is double.  Contraction is off everywhere; + - * / sqrt and
// the conversions are correctly rounded on gfx950 and in numpy.  Only sin, cos, asin, acos and exp are the device library's
// own: afe_estimator_selftest_math evaluates the very helpers the kernels call.
//
//   STATE READ   X = anchor_x + (double)px, Y = anchor_y + (double)py, Z = (double)pz, the attitude widened to double (as
//                load_state<T> of afe_follower.hip).  Nothing is normalised.
//   MEASURE      MocapStateEstimator.cpp:121-258 (cli/mocap_estimator.hpp Measure).  First measurement: the state is the
//                measurement, rates +0, fresh variances (:51-59: 25, 25 / 1, 400), nothing else.  Otherwise the propagate
//                loop (:131-176): at = validAt * 1e-6; stop when at + 1e-6 >= now; (message, span) = Active(at); h = now - at,
//                and h = span if h > span + 1e-6; x += v h; v += acc h; q = q * FromRotationVector(w h) (Rotation.hpp:84-97);
//                w = keep w + (1 - keep) cmd, keep = exp(-h / rate_time_constant), 1 when ballistic; validAt +=
//                uint64(0.5 + h 1e6); both covariances grow as F V F' + Q with the dense product's operand order (:157-172).
//                Gate (:181-205): dP = |pos - x| / sqrt(3 (P.vv + sigma_pos^2)), dA = 2 acos(|r0|) / sqrt(A.vv + sigma_att^2),
//                r = inv(att) * q (Rotation.hpp:124-131, :138-142); an outlier with fewer than ten rejections in a row is
//                counted and skipped; otherwise (after Reset() if there were ten) the gain update (:207-242) through
//                ToRotationVector / FromRotationVector (Rotation.hpp:144-161, :84-97) and (I - g [1 0]) V.  Symmetrise.
//   PREDICT      :62-119 (Predict): the same loop to ahead + wall on a copy; the position and attitude lines use the
//                FILTER'S OWN velocity and rate, not the extrapolated ones (kept).
//   ACTIVE       PredictionPipe.hpp:33-55: newest message first, the first with at + 1e-6 >= from; span = (the next newer
//                message's from, or 1e10) - from.
//
// QUIRKS OF THE REFERENCE, KEPT
//   * span is the active message's whole life from its ACTIVATION, not what is left of it at `at`: a step that starts late
//     in a message's life and is cut to span ends past the successor's activation (an overshooting step).
//   * "messages exist but none is active yet" is ballistic with a span of 1e10, exactly like "no messages".
//   * acos(|r0|) with |r0| a rounding above 1 (fp32 attitudes) is NaN, and NaN > gate is false: it passes the gate as "not
//     an outlier" and the NaN goes into the estimate.
//
// NOTHING HANGS.  Trip counts depend on times alone (h, span and validAt never see the state), so a NaN vehicle runs the
// trips of its neighbours.  The reference loops for ever on two equal activation times (h = 0); here the host refuses such
// an announce, and both loops carry a hard cap of slots + 2 trips: a lane that hits it raises the estimator's error word
// (host-visible), and every later call on the estimator answers AFE_ERR_OUT_OF_RANGE.
//
// LAYOUT.  Planar rows with the engine's stride S, all of one slab of 8-byte words (one base address in the kernel
// arguments; with one pointer a row the scalar registers spilled): est[13] (pos 3, vel 3, att 4, ang_vel 3), cov[6] (P.vv,
// P.vr, P.rr, A.vv, A.vr, A.rr: after Symmetrise vr and rv are the same bits -- (a + b) / 2 and (b + a) / 2 -- and before
// it they are both +0, so three words are stored and four computed with), validAt uint64, pred[13], stage[6], two rows of
// +0 (the prediction buffer's anchors), ring[slots][6] (acc 3, angVel 3); and started, rejectedInARow, rejected in a slab of
// uint32.  THE RING and its rule: afe_estimator_ring.h.  Activation times and the wall time are the host's and come in the
// kernel arguments; all times are relative to afe_time_us at creation (the restatement's Timers start at construction).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "afe_consumer.h"
#include "afe_estimator.h"
#include "afe_estimator_ring.h"

namespace {

constexpr int kBlock = 256;
constexpr int64_t kBlocksPerLaunch = int64_t(1) << 22;   // a launch stays below 2^31 threads
constexpr int kEstWords = 13, kCovWords = 6, kMsgWords = 6;
// rows of the one slab of 8-byte words (EstArgs::slab, `stride` words a row) and of the one of 4-byte words (EstArgs::flags)
constexpr int kRowEst = 0, kRowCov = 13, kRowValid = 19, kRowPred = 20, kRowStage = 33, kRowZero = 39, kRowRing = 41;
constexpr int kFlagStarted = 0, kFlagRow = 1, kFlagRejected = 2, kFlagWords = 3;
constexpr double kTick = afe::kEstimatorTick;
constexpr double kMinAngle = 4.84813681e-6;              // Rotation.hpp: one arc second

// ---- the device library's functions, through the helpers both the kernels and the self-test call --------------------------
// sine and cosine of one angle are asked for together: the helper is the pair, so that a merged call cannot give the kernel
// other bits than the self-test
__device__ __forceinline__ void em_sincos(double x, double *s, double *c) { *s = sin(x); *c = cos(x); }
__device__ __forceinline__ double em_asin(double x) { return asin(x); }
__device__ __forceinline__ double em_acos(double x) { return acos(x); }
__device__ __forceinline__ double em_exp(double x) { return exp(x); }

struct V3 { double x, y, z; };
struct Q4 { double w, x, y, z; };
struct Var { double vv, vr, rv, rr; };     // 2x2 covariance of (value, rate): [[vv, vr], [rv, rr]]

__device__ __forceinline__ Q4 q_mul(const Q4 &a, const Q4 &b) {          // Rotation.hpp:124-131, this = a, r1 = b
#pragma clang fp contract(off)
  Q4 c;
  c.w = b.w * a.w - b.x * a.x - b.y * a.y - b.z * a.z;
  c.x = b.x * a.w + b.w * a.x + b.z * a.y - b.y * a.z;
  c.y = b.y * a.w - b.z * a.x + b.w * a.y + b.x * a.z;
  c.z = b.z * a.w + b.y * a.x - b.x * a.y + b.w * a.z;
  return c;
}
__device__ __forceinline__ Q4 q_inv(const Q4 &q) { Q4 r; r.w = q.w; r.x = -q.x; r.y = -q.y; r.z = -q.z; return r; }
__device__ __forceinline__ double v_norm(const V3 &a) {                  // Vec3.hpp:113-116
#pragma clang fp contract(off)
  return sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
}
__device__ __forceinline__ V3 v_scale(const V3 &a, double k) {
#pragma clang fp contract(off)
  V3 o;
  o.x = a.x * k; o.y = a.y * k; o.z = a.z * k;
  return o;
}
// Rotation.hpp:84-97.  Without a branch (a lane below one arc second computes with theta = 1 and drops the result): the
// propagation loops are divergent enough as they are, and every level of it costs scalar registers.
__device__ __forceinline__ Q4 q_from_rotvec(const V3 &r) {
#pragma clang fp contract(off)
  const double theta = v_norm(r);
  const bool small = theta < kMinAngle;
  const double th = small ? 1.0 : theta;
  const double ux = r.x / th, uy = r.y / th, uz = r.z / th;
  double s, c;
  em_sincos(th * 0.5, &s, &c);
  Q4 q;
  q.w = small ? 1.0 : c; q.x = small ? 0.0 : s * ux; q.y = small ? 0.0 : s * uy; q.z = small ? 0.0 : s * uz;
  return q;
}
// Rotation.hpp:144-161
__device__ __forceinline__ V3 q_to_rotvec(const Q4 &q) {
#pragma clang fp contract(off)
  V3 n;
  if (q.w > 0.0) { n.x = q.x; n.y = q.y; n.z = q.z; }
  else { n.x = -q.x; n.y = -q.y; n.z = -q.z; }
  const double norm = v_norm(n);
  const double angle = em_asin(norm) * 2;
  const bool small = angle < kMinAngle;
  const V3 o = v_scale(n, angle / (small ? 1.0 : norm));
  V3 z;
  z.x = small ? 0.0 : o.x; z.y = small ? 0.0 : o.y; z.z = small ? 0.0 : o.z;
  return z;
}
// Rotation.hpp:138-142
__device__ __forceinline__ double q_angle(const Q4 &r) {
#pragma clang fp contract(off)
  return em_acos(fabs(r.w)) * 2.0;
}
// F V F' + Q, F = [[1, h], [0, 1]], Q = diag(h^4 s / 4, h^2 s)   (MocapStateEstimator.cpp:157-172)
__device__ __forceinline__ void grow(Var &V, double h, double s) {
#pragma clang fp contract(off)
  const double a = 1 * V.vv + h * V.rv, b = 1 * V.vr + h * V.rr;
  const double c = 0 * V.vv + 1 * V.rv, d = 0 * V.vr + 1 * V.rr;
  Var n;
  n.vv = (a * 1 + b * h) + h * h * h * h * s / 4;
  n.vr = (a * 0 + b * 1) + 0;
  n.rv = (c * 1 + d * h) + 0;
  n.rr = (c * 0 + d * 1) + h * h * s;
  V = n;
}
// (I - g [1 0]) V   (:236-242)
__device__ __forceinline__ void shrink(Var &V, double g0, double g1) {
#pragma clang fp contract(off)
  const double a = 1 - g0 * 1, b = 0 - g0 * 0, c = 0 - g1 * 1, d = 1 - g1 * 0;
  Var n;
  n.vv = a * V.vv + b * V.rv; n.vr = a * V.vr + b * V.rr;
  n.rv = c * V.vv + d * V.rv; n.rr = c * V.vr + d * V.rr;
  V = n;
}
__device__ __forceinline__ void symmetrise(Var &V) {
#pragma clang fp contract(off)
  Var n;
  n.vv = (V.vv + V.vv) * 0.5; n.vr = (V.vr + V.rv) * 0.5;
  n.rv = (V.rv + V.vr) * 0.5; n.rr = (V.rr + V.rr) * 0.5;
  V = n;
}

struct Noise {
  double rate_tc, gate, sigma_pos, sigma_att, sigma_acc, sigma_ang_acc;
};

// the host's view of the pipe for one call: activation times newest first, message j in slot (newest_slot - j) mod slots
struct Pipe {
  int n, newest_slot, slots, cap;          // cap: the loops' hard trip limit, slots + 2
  double from[afe::kEstimatorMaxSlots];
};

struct EstArgs {
  const void *pos, *att;                   // the engine's slabs
  const double *anchor_xy;
  int64_t stride, n;
  double *slab;                            // rows kRow*: est 13, cov 6, validAt (uint64), pred 13, stage 6, +0 2, ring slots * 6
  uint32_t *flags;                         // rows kFlag*: started, rejectedInARow, rejected
  unsigned long long *counter;
  uint32_t *error;                         // host memory, the device's address of it
  Noise noise;
};

struct State {
  V3 x, v, w;
  Q4 q;
};

struct Plan { V3 acc, ang_vel; bool free_fall; };

// PredictionPipe.hpp:33-55: the newest message already active at t, and how long it stays the newest -- from its activation
__device__ __forceinline__ Plan active(const EstArgs &g, const Pipe &pipe, int64_t v, double t, double &span) {
#pragma clang fp contract(off)
  const int64_t S = g.stride;
  // every lane walks the whole list (the trip count is the wave's, the activation times stay scalar) and keeps its first hit
  double next = 1e10;
  int found = -1;
  span = 1e10;
#pragma nounroll
  for (int j = 0; j < pipe.n; j++) {
    const double from = pipe.from[j];
    if (found < 0 && (t + kTick) >= from) {
      found = j;
      span = next - from;
    }
    next = from;
  }
  Plan p;
  p.acc.x = p.acc.y = p.acc.z = 0.0;
  p.ang_vel = p.acc;
  p.free_fall = found < 0;
  if (found >= 0) {
    int slot = pipe.newest_slot - found;
    if (slot < 0) slot += pipe.slots;
    const double *M = g.slab + (int64_t)(kRowRing + slot * kMsgWords) * S + v;
    p.acc.x = M[0]; p.acc.y = M[S]; p.acc.z = M[2 * S];
    p.ang_vel.x = M[3 * S]; p.ang_vel.y = M[4 * S]; p.ang_vel.z = M[5 * S];
  }
  return p;
}

template <typename T>
__device__ __forceinline__ void load_truth(const EstArgs &g, int64_t v, V3 &p, Q4 &q) {
#pragma clang fp contract(off)
  const int64_t S = g.stride;
  const T *P = (const T *)g.pos, *Q = (const T *)g.att;
  p.x = g.anchor_xy[v] + (double)P[v]; p.y = g.anchor_xy[S + v] + (double)P[S + v]; p.z = (double)P[2 * S + v];
  q.w = (double)Q[v]; q.x = (double)Q[S + v]; q.y = (double)Q[2 * S + v]; q.z = (double)Q[3 * S + v];
}
__device__ __forceinline__ State load_est(const double *E, int64_t S, int64_t v) {
  State s;
  s.x.x = E[v]; s.x.y = E[S + v]; s.x.z = E[2 * S + v];
  s.v.x = E[3 * S + v]; s.v.y = E[4 * S + v]; s.v.z = E[5 * S + v];
  s.q.w = E[6 * S + v]; s.q.x = E[7 * S + v]; s.q.y = E[8 * S + v]; s.q.z = E[9 * S + v];
  s.w.x = E[10 * S + v]; s.w.y = E[11 * S + v]; s.w.z = E[12 * S + v];
  return s;
}
__device__ __forceinline__ void store_est(double *E, int64_t S, int64_t v, const State &s) {
  E[v] = s.x.x; E[S + v] = s.x.y; E[2 * S + v] = s.x.z;
  E[3 * S + v] = s.v.x; E[4 * S + v] = s.v.y; E[5 * S + v] = s.v.z;
  E[6 * S + v] = s.q.w; E[7 * S + v] = s.q.x; E[8 * S + v] = s.q.y; E[9 * S + v] = s.q.z;
  E[10 * S + v] = s.w.x; E[11 * S + v] = s.w.y; E[12 * S + v] = s.w.z;
}
__device__ __forceinline__ void store_cov(double *C, int64_t S, int64_t v, const Var &P, const Var &A) {
  C[v] = P.vv; C[S + v] = P.vr; C[2 * S + v] = P.rr;
  C[3 * S + v] = A.vv; C[4 * S + v] = A.vr; C[5 * S + v] = A.rr;
}
// The stride again, as a value the compiler cannot tie to the first one: the row offsets of the stores behind a propagation
// loop are then formed behind the loop, not held in scalar registers across it (where they were spilled).
__device__ __forceinline__ int64_t stride_again(int64_t S) {
  asm volatile("" : "+s"(S));
  return S;
}
__device__ __forceinline__ void fresh_state(State &s) {
  s.x.x = s.x.y = s.x.z = 0.0;
  s.v = s.x; s.w = s.x;
  s.q.w = 1.0; s.q.x = s.q.y = s.q.z = 0.0;
}
__device__ __forceinline__ void fresh_variances(Var &P, Var &A) {          // MocapStateEstimator.cpp:51-59
  P.vv = 25.0; P.rr = 25.0; P.vr = P.rv = 0.0;
  A.vv = 1.0; A.rr = 400; A.vr = A.rv = 0.0;
}

// Reset() for vehicles [first, first + count): not started, the zero state, fresh variances, validAt = the wall time
__global__ void __launch_bounds__(kBlock) afe_estimator_reset_kernel(EstArgs g, int64_t first, int64_t count, unsigned long long wall_us, int clear_counters) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  const int64_t v = first + i, S = g.stride;
  State s;
  Var P, A;
  fresh_state(s);
  fresh_variances(P, A);
  store_est(g.slab + kRowEst * S, S, v, s);
  store_cov(g.slab + kRowCov * S, S, v, P, A);
  ((unsigned long long *)g.slab)[kRowValid * S + v] = wall_us;
  g.flags[kFlagStarted * S + v] = 0;
  if (clear_counters) { g.flags[kFlagRow * S + v] = 0; g.flags[kFlagRejected * S + v] = 0; }
}

// UpdateWithMeasurement for one vehicle; -> this call rejected the measurement.
// A vehicle at its FIRST measurement (:122-129: the state is the measurement, rates +0, fresh variances, nothing else) walks
// through everything on the zero state Reset() left it, without propagating, and is overwritten at the end.  A branch round
// the function would hold its mask in scalar registers across all of it, where the double functions' constants want every
// one of them; so the flag travels as a vector register and is looked at again only behind the update.
__device__ __forceinline__ bool measure_one(const EstArgs &g, const Pipe &pipe, int64_t v, const V3 &pos, const Q4 &att, unsigned long long wall_us,
                                            bool &capped) {
#pragma clang fp contract(off)
  const int64_t S = g.stride;
  uint32_t was_started = g.flags[kFlagStarted * S + v];
  State s;
  Var P, A;
  s = load_est(g.slab + kRowEst * S, S, v);
  const double *C = g.slab + kRowCov * S;
  P.vv = C[v]; P.vr = C[S + v]; P.rv = P.vr; P.rr = C[2 * S + v];
  A.vv = C[3 * S + v]; A.vr = C[4 * S + v]; A.rv = A.vr; A.rr = C[5 * S + v];
  const unsigned long long valid0 = ((const unsigned long long *)g.slab)[kRowValid * S + v];
  const uint32_t row0 = g.flags[kFlagRow * S + v];
  unsigned long long valid = valid0;
  uint32_t row = row0;
  const Noise &nz = g.noise;
  const double now = (double)wall_us * 1e-6;
  unsigned long long wall_lane = wall_us;            // Reset() wants it behind the loop: in a vector register, not a scalar pair held across it
  asm volatile("" : "+v"(wall_lane));
  // The propagate loop, with the WAVE's trip count: a lane that has arrived (or never left: now <= validAt) walks along
  // with h = 0 and keeps what it had, so the loop branches on scalar conditions alone.
  const bool behind = was_started != 0 && now > (double)valid * 1e-6;
  for (int trip = 0;; trip++) {
    const double at = (double)valid * 1e-6;
    const bool go = behind && !((at + kTick) >= now);
    if (!__any(go)) break;
    if (trip >= pipe.cap) { capped = go; break; }
    double span = 0;
    const Plan p = active(g, pipe, v, at, span);
    double h = now - at;
    if (h > (span + kTick)) h = span;
    if (!go) h = 0.0;
    State o;
    o.x.x = s.x.x + s.v.x * h; o.x.y = s.x.y + s.v.y * h; o.x.z = s.x.z + s.v.z * h;
    o.v.x = s.v.x + p.acc.x * h; o.v.y = s.v.y + p.acc.y * h; o.v.z = s.v.z + p.acc.z * h;
    o.q = q_mul(s.q, q_from_rotvec(v_scale(s.w, h)));
    double keep = em_exp(-h / nz.rate_tc);
    if (p.free_fall) keep = 1;
    o.w.x = keep * s.w.x + (1 - keep) * p.ang_vel.x;
    o.w.y = keep * s.w.y + (1 - keep) * p.ang_vel.y;
    o.w.z = keep * s.w.z + (1 - keep) * p.ang_vel.z;
    Var Pn = P, An = A;
    grow(Pn, h, nz.sigma_acc);
    grow(An, h, nz.sigma_ang_acc);
    if (go) {
      s = o; P = Pn; A = An;
      valid += (unsigned long long)(0.5 + h * 1e6);
    }
  }
  double sP = P.vv + nz.sigma_pos * nz.sigma_pos, sA = A.vv + nz.sigma_att * nz.sigma_att;
  V3 ex;
  ex.x = pos.x - s.x.x; ex.y = pos.y - s.x.y; ex.z = pos.z - s.x.z;
  const double dP = v_norm(ex) / sqrt(3 * sP);
  const double dA = q_angle(q_mul(q_inv(att), s.q)) / sqrt(sA);
  const bool outlier = (dP > nz.gate) || (dA > nz.gate);
  bool rejected_now = outlier && row < 10;
  // The gain update for every lane, taken by those that did not reject (a rejection is rare, and a branch round the update
  // would hold its mask in scalar registers across asin, sin and cos).
  State u = s;
  Var Pu = P, Au = A;
  const bool reset = !rejected_now && row >= 10;
  if (reset) {                                                           // Reset()
    fresh_state(u);
    fresh_variances(Pu, Au);
    sP = Pu.vv + nz.sigma_pos * nz.sigma_pos;
    sA = Au.vv + nz.sigma_att * nz.sigma_att;
  }
  {
    const double gP0 = Pu.vv * (1 / sP), gP1 = Pu.rv * (1 / sP);
    const double gA0 = Au.vv * (1 / sA), gA1 = Au.rv * (1 / sA);
    ex.x = pos.x - u.x.x; ex.y = pos.y - u.x.y; ex.z = pos.z - u.x.z;
    u.x.x = u.x.x + gP0 * ex.x; u.x.y = u.x.y + gP0 * ex.y; u.x.z = u.x.z + gP0 * ex.z;
    u.v.x = u.v.x + gP1 * ex.x; u.v.y = u.v.y + gP1 * ex.y; u.v.z = u.v.z + gP1 * ex.z;
    const V3 ea = q_to_rotvec(q_mul(q_inv(u.q), att));
    V3 ga;
    ga.x = gA0 * ea.x; ga.y = gA0 * ea.y; ga.z = gA0 * ea.z;
    u.q = q_mul(u.q, q_from_rotvec(ga));
    u.w.x = u.w.x + gA1 * ea.x; u.w.y = u.w.y + gA1 * ea.y; u.w.z = u.w.z + gA1 * ea.z;
    shrink(Pu, gP0, gP1);
    shrink(Au, gA0, gA1);
  }
  uint32_t started = reset ? 0 : 1;
  if (reset) valid = wall_lane;
  if (rejected_now) row++;
  else { row = 0; s = u; P = Pu; A = Au; }
  symmetrise(P);
  symmetrise(A);
  asm volatile("" : "+v"(was_started));                                  // (looked at again, not remembered as a mask)
  if (was_started == 0) {
    s.x = pos; s.q = att;
    s.v.x = s.v.y = s.v.z = 0.0;
    s.w = s.v;
    fresh_variances(P, A);
    valid = valid0; row = row0; started = 1;
    rejected_now = false;
  }
  const int64_t S2 = stride_again(S);
  if (rejected_now) g.flags[kFlagRejected * S2 + v] = g.flags[kFlagRejected * S2 + v] + 1;
  store_est(g.slab + kRowEst * S2, S2, v, s);
  store_cov(g.slab + kRowCov * S2, S2, v, P, A);
  ((unsigned long long *)g.slab)[kRowValid * S2 + v] = valid;
  g.flags[kFlagStarted * S2 + v] = started;
  g.flags[kFlagRow * S2 + v] = row;
  return rejected_now;
}

template <typename T>
__global__ void __launch_bounds__(kBlock) afe_estimator_measure_kernel(EstArgs g, Pipe pipe, unsigned long long wall_us) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  // lanes beyond n LEAVE: nothing below waits for them, so no mask of theirs has to sit in scalar registers across measure_one
  if (v >= g.n) return;
  V3 pos;
  Q4 att;
  load_truth<T>(g, v, pos, att);
  bool capped = false;
  const bool rejected_now = measure_one(g, pipe, v, pos, att, wall_us, capped);
  if (capped) __hip_atomic_store(g.error, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (g.counter) {                                                       // one ballot of the lanes still here, one atomic by the first that rejected
    const unsigned long long mask = __ballot(rejected_now);
    if (mask && (int)(threadIdx.x & 63) == __ffsll((long long)mask) - 1) atomicAdd(g.counter, (unsigned long long)__popcll(mask));
  }
}

// GetPrediction(ahead): the estimate extrapolated to ahead + wall into the prediction buffer; the state is not touched
__global__ void __launch_bounds__(kBlock) afe_estimator_predict_kernel(EstArgs g, Pipe pipe, unsigned long long wall_us, double ahead) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= g.n) return;
  const int64_t S = g.stride;
  const State f = load_est(g.slab + kRowEst * S, S, v);                                   // the filter's own: f.v and f.w stay in the lines below
  State e = f;
  const double until = ahead + (double)wall_us * 1e-6;
  double t = (double)((const unsigned long long *)g.slab)[kRowValid * S + v] * 1e-6;
  bool capped = false;
  for (int trip = 0;; trip++) {                                            // the wave's trip count, as in the measure kernel
    const bool go = (t + kTick) < until;
    if (!__any(go)) break;
    if (trip >= pipe.cap) { capped = go; break; }
    double span = 0;
    const Plan p = active(g, pipe, v, t, span);
    double h = until - t;
    if (h > (span + kTick)) h = span;
    if (!go) h = 0.0;
    State n;
    n.x.x = e.x.x + f.v.x * h + p.acc.x * h * h / 2;
    n.x.y = e.x.y + f.v.y * h + p.acc.y * h * h / 2;
    n.x.z = e.x.z + f.v.z * h + p.acc.z * h * h / 2;
    n.v.x = e.v.x + p.acc.x * h; n.v.y = e.v.y + p.acc.y * h; n.v.z = e.v.z + p.acc.z * h;
    n.q = q_mul(e.q, q_from_rotvec(v_scale(f.w, h)));
    double keep = em_exp(-h / g.noise.rate_tc);
    if (p.free_fall) keep = 1;
    n.w.x = keep * e.w.x + (1 - keep) * p.ang_vel.x;
    n.w.y = keep * e.w.y + (1 - keep) * p.ang_vel.y;
    n.w.z = keep * e.w.z + (1 - keep) * p.ang_vel.z;
    if (go) {
      e = n;
      t += h;
    }
  }
  const int64_t S2 = stride_again(S);
  store_est(g.slab + kRowPred * S2, S2, v, e);
  if (capped) __hip_atomic_store(g.error, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// SetPredictedValues from the staged host arrays: vehicles [first, first + count) take them, the others repeat the message
// before (prev_slot, -1: +0), so that a slot is always whole
__global__ void __launch_bounds__(kBlock) afe_estimator_announce_kernel(EstArgs g, int64_t first, int64_t count, int write_slot, int prev_slot) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= g.n) return;
  const int64_t S = g.stride;
  const bool mine = v >= first && v - first < count;
  double *W = g.slab + (int64_t)(kRowRing + write_slot * kMsgWords) * S + v;
  const double *R = mine ? g.slab + kRowStage * S + v : prev_slot >= 0 ? g.slab + (int64_t)(kRowRing + prev_slot * kMsgWords) * S + v : nullptr;
#pragma unroll
  for (int k = 0; k < kMsgWords; k++) W[k * S] = R ? R[k * S] : 0.0;
}

__global__ void __launch_bounds__(kBlock) afe_estimator_math_kernel(int op, int64_t n, const double *x, double *y) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double s, c;
  em_sincos(x[i], &s, &c);
  y[i] = op == 0 ? s : op == 1 ? c : op == 2 ? em_asin(x[i]) : op == 3 ? em_acos(x[i]) : em_exp(x[i]);
}

size_t up256(size_t x) { return (x + 255) & ~size_t(255); }

}  // namespace

struct afe_estimator {
  afe_engine *engine = nullptr;     // borrowed
  int device = 0;
  int64_t n = 0, stride = 0;
  uint64_t t0_us = 0;               // afe_time_us at creation: every time below is relative to it
  double delay_s = 0;
  uint64_t n_measures = 0;
  bool have_pred = false;
  uint64_t pred_stamp_us = 0;       // afe_time_us (absolute) of the last predict
  afe::EstimatorRing ring;
  afe::DevBuf arena;
  afe::PinnedBuf<hipHostMallocCoherent | hipHostMallocMapped> error_host;   // uint32: a loop hit its trip cap
  EstArgs args;
};

namespace {

bool failed(const afe_estimator *est) { return *(volatile const uint32_t *)est->error_host.get() != 0; }

struct Entry {
  hipStream_t stream;
  EstArgs g;
  int elem;
  uint64_t now_us, wall_us;
};

// through the engine's gate (a resident grid ends here); the handle against what it got; the clock
int enter(afe_estimator *est, Entry *en) {
  if (failed(est)) return AFE_ERR_OUT_OF_RANGE;
  afe::EngineAccess acc;
  int rc = afe::engine_enter(est->engine, &acc);
  if (rc != AFE_OK) return rc;
  const afe_device_view &view = acc.view;
  if (view.n_vehicles != est->n || view.stride != est->stride || acc.device != est->device) return AFE_ERR_INVALID_ARG;
  en->stream = acc.stream;
  en->g = est->args;
  en->g.pos = view.pos; en->g.att = view.att; en->g.anchor_xy = view.pos_anchor_xy;
  en->elem = view.state_elem_size;
  rc = afe_time_us(est->engine, &en->now_us);
  if (rc != AFE_OK) return rc;
  if (en->now_us < est->t0_us) return AFE_ERR_OUT_OF_RANGE;                // (the engine's clock was set back)
  en->wall_us = en->now_us - est->t0_us;
  return AFE_OK;
}

Pipe pipe_of(const afe_estimator *est) {
  Pipe p;
  std::memset(&p, 0, sizeof(p));
  const afe::EstimatorRing &r = est->ring;
  p.n = r.n_messages();
  p.slots = r.slots;
  p.cap = r.slots + 2;
  p.newest_slot = p.n ? r.newest_slot() : 0;
  for (int j = 0; j < p.n; j++) p.from[j] = r.from[(p.newest_slot - j + r.slots) % r.slots];
  return p;
}

dim3 grid_for(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }
bool launched() { return hipGetLastError() == hipSuccess; }

int enter_rows(afe_estimator *est, int64_t first, int64_t count) {
  if (!est || first < 0 || count < 0) return AFE_ERR_INVALID_ARG;
  if (first > est->n || count > est->n - first) return AFE_ERR_OUT_OF_RANGE;   // (no sum: it can wrap)
  return AFE_OK;
}
bool put_rows(void *dev, size_t esz, int comps, int64_t stride, int64_t first, int64_t count, const void *host) {
  return hipMemcpy2D((char *)dev + (size_t)first * esz, (size_t)stride * esz, host, (size_t)count * esz, (size_t)count * esz, (size_t)comps,
                     hipMemcpyHostToDevice) == hipSuccess;
}
bool get_rows(const void *dev, size_t esz, int comps, int64_t stride, int64_t first, int64_t count, void *host) {
  return hipMemcpy2D(host, (size_t)count * esz, (const char *)dev + (size_t)first * esz, (size_t)stride * esz, (size_t)count * esz, (size_t)comps,
                     hipMemcpyDeviceToHost) == hipSuccess;
}

}  // namespace

extern "C" int afe_estimator_default_config(afe_estimator_config *cfg) {
  if (!cfg) return AFE_ERR_INVALID_ARG;
  afe_estimator_config c;
  std::memset(&c, 0, sizeof(c));
  c.struct_bytes = sizeof(c);
  c.command_delay_s = 0.03;             // main.cpp:178
  c.rate_time_constant_s = 0.04;        // MocapStateEstimator.cpp:24-33
  c.gate = 6.0;
  c.sigma_pos = 0.02;
  c.sigma_att = 5 * M_PI / 180;
  c.sigma_acc = 1.0 * 9.81;
  c.sigma_ang_acc = 200;
  c.offboard_period_us = 10000;
  c.max_measure_gap_us = 10000;
  *cfg = c;
  return AFE_OK;
}

extern "C" int afe_estimator_ring_slots(const afe_estimator_config *cfg, int *slots) {
  if (!cfg || !slots || cfg->struct_bytes < sizeof(afe_estimator_config)) return AFE_ERR_INVALID_ARG;
  if (!(cfg->command_delay_s >= 0) || !(cfg->command_delay_s < 1e6)) return AFE_ERR_INVALID_ARG;
  const uint64_t delay_us = (uint64_t)std::ceil(cfg->command_delay_s * 1e6);
  const int k = afe::estimator_ring_slots(delay_us, cfg->offboard_period_us, cfg->max_measure_gap_us);
  if (k == 0) return AFE_ERR_OUT_OF_RANGE;
  *slots = k;
  return AFE_OK;
}

extern "C" int afe_estimator_create(afe_engine *e, const afe_estimator_config *cfg, afe_estimator **out) {
  if (!e || !cfg || !out || cfg->struct_bytes < sizeof(afe_estimator_config)) return AFE_ERR_INVALID_ARG;
  if (!(cfg->rate_time_constant_s > 0) || !std::isfinite(cfg->rate_time_constant_s) || !(cfg->gate > 0) || !(cfg->sigma_pos > 0) ||
      !(cfg->sigma_att > 0) || !(cfg->sigma_acc >= 0) || !(cfg->sigma_ang_acc >= 0) || !std::isfinite(cfg->sigma_pos) ||
      !std::isfinite(cfg->sigma_att) || !std::isfinite(cfg->sigma_acc) || !std::isfinite(cfg->sigma_ang_acc))
    return AFE_ERR_INVALID_ARG;
  int slots = 0;
  int rc = afe_estimator_ring_slots(cfg, &slots);
  if (rc != AFE_OK) return rc;
  afe::EngineAccess acc;
  rc = afe::engine_enter(e, &acc);
  if (rc != AFE_OK) return rc;
  rc = afe::engine_device_resident(e);
  if (rc != AFE_OK) return rc;
  uint64_t now_us = 0;
  rc = afe_time_us(e, &now_us);
  if (rc != AFE_OK) return rc;
  afe_estimator *est = new afe_estimator();
  est->engine = e; est->device = acc.device; est->n = acc.view.n_vehicles; est->stride = acc.view.stride;
  est->t0_us = now_us; est->delay_s = cfg->command_delay_s;
  est->ring.slots = slots;
  const size_t S = (size_t)est->stride;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += up256(bytes); return o; };
  const size_t o_slab = take(S * 8 * (size_t)(kRowRing + kMsgWords * slots)), o_flags = take(S * 4 * kFlagWords), o_cnt = take(8);
  uint32_t *err_dev = nullptr;
  if (!est->arena.alloc(off) || !est->error_host.alloc(64) ||
      hipHostGetDevicePointer((void **)&err_dev, est->error_host.get(), 0) != hipSuccess) {
    (void)hipGetLastError();
    delete est;
    return AFE_ERR_HIP;
  }
  *est->error_host.as<uint32_t>() = 0;
  unsigned char *A = est->arena.as<unsigned char>();
  std::memset(&est->args, 0, sizeof(est->args));
  EstArgs &g = est->args;
  g.n = est->n; g.stride = est->stride;
  g.slab = (double *)(A + o_slab); g.flags = (uint32_t *)(A + o_flags);
  g.anchor_xy = nullptr;
  g.counter = (unsigned long long *)(A + o_cnt);
  g.error = err_dev;
  g.noise.rate_tc = cfg->rate_time_constant_s; g.noise.gate = cfg->gate; g.noise.sigma_pos = cfg->sigma_pos;
  g.noise.sigma_att = cfg->sigma_att; g.noise.sigma_acc = cfg->sigma_acc; g.noise.sigma_ang_acc = cfg->sigma_ang_acc;
  const hipStream_t stream = acc.stream;
  rc = hipMemsetAsync(A, 0, off, stream) == hipSuccess ? AFE_OK : AFE_ERR_HIP;      // ring, padding and the +0 anchors included
  if (rc == AFE_OK && est->n > 0) {
    if (est->n > kBlocksPerLaunch * kBlock) rc = AFE_ERR_OUT_OF_RANGE;
    else {
      hipLaunchKernelGGL(afe_estimator_reset_kernel, grid_for(est->n), dim3(kBlock), 0, stream, g, (int64_t)0, est->n, 0ull, 1);
      if (!launched()) rc = AFE_ERR_HIP;
    }
  }
  if (rc == AFE_OK && hipStreamSynchronize(stream) != hipSuccess) rc = AFE_ERR_HIP;
  if (rc != AFE_OK) { (void)hipGetLastError(); (void)afe_estimator_destroy(est); return rc; }
  est->args.anchor_xy = g.slab + kRowZero * est->stride;                           // the +0 anchors, for the follower
  *out = est;
  return AFE_OK;
}

extern "C" int afe_estimator_destroy(afe_estimator *est) {
  if (!est) return AFE_ERR_INVALID_ARG;
  (void)hipSetDevice(est->device);
  (void)hipDeviceSynchronize();
  delete est;
  return AFE_OK;
}

extern "C" int afe_estimator_info(const afe_estimator *est, int64_t *n_vehicles, int *slots, uint64_t *n_measures, int *n_messages, uint32_t *error) {
  if (!est) return AFE_ERR_INVALID_ARG;
  if (n_vehicles) *n_vehicles = est->n;
  if (slots) *slots = est->ring.slots;
  if (n_measures) *n_measures = est->n_measures;
  if (n_messages) *n_messages = est->ring.n_messages();
  if (error) *error = failed(est) ? 1u : 0u;
  return AFE_OK;
}

extern "C" int afe_estimator_measure(afe_estimator *est, int64_t *n_rejected) {
  if (!est) return AFE_ERR_INVALID_ARG;
  Entry en;
  int rc = enter(est, &en);
  if (rc != AFE_OK) return rc;
  EstArgs &g = en.g;
  if (n_rejected) {
    if (hipMemsetAsync(g.counter, 0, 8, en.stream) != hipSuccess) return AFE_ERR_HIP;
  } else g.counter = nullptr;
  if (est->n > 0) {
    const Pipe pipe = pipe_of(est);
    if (en.elem == 8) hipLaunchKernelGGL(afe_estimator_measure_kernel<double>, grid_for(g.n), dim3(kBlock), 0, en.stream, g, pipe, (unsigned long long)en.wall_us);
    else hipLaunchKernelGGL(afe_estimator_measure_kernel<float>, grid_for(g.n), dim3(kBlock), 0, en.stream, g, pipe, (unsigned long long)en.wall_us);
    if (!launched()) return AFE_ERR_HIP;
  }
  est->ring.measured(en.wall_us);
  est->n_measures++;
  if (n_rejected) {
    unsigned long long k = 0;
    if (hipMemcpyAsync(&k, g.counter, 8, hipMemcpyDeviceToHost, en.stream) != hipSuccess || hipStreamSynchronize(en.stream) != hipSuccess)
      return AFE_ERR_HIP;
    *n_rejected = (int64_t)k;
    if (failed(est)) return AFE_ERR_OUT_OF_RANGE;
  }
  return AFE_OK;
}

extern "C" int afe_estimator_predict(afe_estimator *est, double ahead_s) {
  if (!est || !std::isfinite(ahead_s)) return AFE_ERR_INVALID_ARG;
  Entry en;
  const int rc = enter(est, &en);
  if (rc != AFE_OK) return rc;
  if (est->n > 0) {
    hipLaunchKernelGGL(afe_estimator_predict_kernel, grid_for(en.g.n), dim3(kBlock), 0, en.stream, en.g, pipe_of(est), (unsigned long long)en.wall_us, ahead_s);
    if (!launched()) return AFE_ERR_HIP;
  }
  est->have_pred = true;
  est->pred_stamp_us = en.now_us;
  return AFE_OK;
}

extern "C" int afe_estimator_get_prediction(afe_estimator *est, int64_t first, int64_t count, double *est13) {
  const int arc = enter_rows(est, first, count);
  if (arc != AFE_OK) return arc;
  if (!est13) return AFE_ERR_INVALID_ARG;
  if (!est->have_pred) return AFE_ERR_NOT_CONFIGURED;
  if (count == 0) return AFE_OK;
  Entry en;
  const int rc = enter(est, &en);
  if (rc != AFE_OK) return rc;
  if (hipStreamSynchronize(en.stream) != hipSuccess) return AFE_ERR_HIP;
  if (failed(est)) return AFE_ERR_OUT_OF_RANGE;
  return get_rows(est->args.slab + kRowPred * est->stride, 8, kEstWords, est->stride, first, count, est13) ? AFE_OK : AFE_ERR_HIP;
}

extern "C" int afe_estimator_announce(afe_estimator *est, int64_t first, int64_t count, const double *ang_vel3, const double *acc3) {
  const int arc = enter_rows(est, first, count);
  if (arc != AFE_OK) return arc;
  if (!ang_vel3 || !acc3) return AFE_ERR_INVALID_ARG;
  Entry en;
  int rc = enter(est, &en);
  if (rc != AFE_OK) return rc;
  const double from_s = (double)en.wall_us * 1e-6 + est->delay_s;         // PredictionPipe.hpp:25-31
  if (!est->ring.accepts(from_s)) return AFE_ERR_OUT_OF_RANGE;
  if (est->n > 0) {
    if (hipStreamSynchronize(en.stream) != hipSuccess) return AFE_ERR_HIP;
    double *stage = en.g.slab + kRowStage * est->stride;
    if (count > 0 && (!put_rows(stage, 8, 3, est->stride, first, count, acc3) || !put_rows(stage + 3 * est->stride, 8, 3, est->stride, first, count, ang_vel3)))
      return AFE_ERR_HIP;
    const int prev = est->ring.seq ? est->ring.newest_slot() : -1;
    hipLaunchKernelGGL(afe_estimator_announce_kernel, grid_for(en.g.n), dim3(kBlock), 0, en.stream, en.g, first, count, est->ring.write_slot(), prev);
    if (!launched()) return AFE_ERR_HIP;
  }
  est->ring.push(from_s);
  return AFE_OK;
}

extern "C" int afe_estimator_get_state(afe_estimator *est, int64_t first, int64_t count, double *est13, double *cov6, uint64_t *valid_at_us,
                                       uint8_t *started, uint32_t *rejected_in_a_row, uint32_t *rejected) {
  const int arc = enter_rows(est, first, count);
  if (arc != AFE_OK) return arc;
  if (!est13 && !cov6 && !valid_at_us && !started && !rejected_in_a_row && !rejected) return AFE_ERR_INVALID_ARG;
  if (count == 0) return AFE_OK;
  Entry en;
  const int rc = enter(est, &en);
  if (rc != AFE_OK) return rc;
  if (hipStreamSynchronize(en.stream) != hipSuccess) return AFE_ERR_HIP;
  if (failed(est)) return AFE_ERR_OUT_OF_RANGE;
  const EstArgs &g = est->args;
  const int64_t S = est->stride;
  if ((est13 && !get_rows(g.slab + kRowEst * S, 8, kEstWords, S, first, count, est13)) ||
      (cov6 && !get_rows(g.slab + kRowCov * S, 8, kCovWords, S, first, count, cov6)) ||
      (valid_at_us && !get_rows(g.slab + kRowValid * S, 8, 1, S, first, count, valid_at_us)) ||
      (rejected_in_a_row && !get_rows(g.flags + kFlagRow * S, 4, 1, S, first, count, rejected_in_a_row)) ||
      (rejected && !get_rows(g.flags + kFlagRejected * S, 4, 1, S, first, count, rejected)))
    return AFE_ERR_HIP;
  if (started) {                                                            // a 4-byte word on the device, a byte for the caller
    std::vector<uint32_t> word((size_t)count);
    if (!get_rows(g.flags + kFlagStarted * S, 4, 1, S, first, count, word.data())) return AFE_ERR_HIP;
    for (int64_t i = 0; i < count; i++) started[i] = word[(size_t)i] ? 1 : 0;
  }
  return AFE_OK;
}

extern "C" int afe_estimator_reset(afe_estimator *est, int64_t first, int64_t count) {
  const int arc = enter_rows(est, first, count);
  if (arc != AFE_OK) return arc;
  if (count == 0) return AFE_OK;
  Entry en;
  const int rc = enter(est, &en);
  if (rc != AFE_OK) return rc;
  hipLaunchKernelGGL(afe_estimator_reset_kernel, grid_for(count), dim3(kBlock), 0, en.stream, en.g, first, count, (unsigned long long)en.wall_us, 0);
  if (!launched()) return AFE_ERR_HIP;
  est->ring.was_reset(en.wall_us);
  return AFE_OK;
}

extern "C" int afe_estimator_selftest_math(int device, int op, int64_t n, const double *x, double *y) {
  if (!x || !y || op < 0 || op > 4 || n < 0) return AFE_ERR_INVALID_ARG;
  if (n == 0) return AFE_OK;
  if (n > kBlocksPerLaunch * kBlock) return AFE_ERR_OUT_OF_RANGE;
  const int prc = afe::pick_gfx950(device, &device);
  if (prc != AFE_OK) return prc;
  const size_t bytes = (size_t)n * 8;
  afe::DevBuf dx, dy;
  if (!dx.upload(x, bytes) || !dy.alloc(bytes)) { (void)hipGetLastError(); return AFE_ERR_HIP; }
  hipLaunchKernelGGL(afe_estimator_math_kernel, grid_for(n), dim3(kBlock), 0, nullptr, op, n, dx.as<double>(), dy.as<double>());
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return AFE_ERR_HIP;
  return dy.download(y, bytes) ? AFE_OK : AFE_ERR_HIP;
}

// ---- for the follower (afe_estimator.h) --------------------------------------------------------------------------------------
int afe::estimator_check_engine(const afe_estimator *est, const afe_engine *e) {
  return est && est->engine == e ? AFE_OK : AFE_ERR_INVALID_ARG;
}

int afe::estimator_link(afe_estimator *est, uint64_t now_us, EstimatorLink *out) {
  if (failed(est)) return AFE_ERR_OUT_OF_RANGE;
  if (!est->have_pred || est->pred_stamp_us != now_us) return AFE_ERR_NOT_CONFIGURED;
  const int64_t S = est->stride;
  const double *pred = est->args.slab + kRowPred * S;
  out->pos = pred; out->vel = pred + 3 * S; out->att = pred + 6 * S;
  out->zero_anchor_xy = est->args.anchor_xy;
  return AFE_OK;
}

int afe::estimator_announce_begin(afe_estimator *est, uint64_t now_us, double **slot, double *from_s) {
  if (failed(est)) return AFE_ERR_OUT_OF_RANGE;
  if (now_us < est->t0_us) return AFE_ERR_OUT_OF_RANGE;
  *from_s = (double)(now_us - est->t0_us) * 1e-6 + est->delay_s;
  if (!est->ring.accepts(*from_s)) return AFE_ERR_OUT_OF_RANGE;
  *slot = est->args.slab + (int64_t)(kRowRing + est->ring.write_slot() * kMsgWords) * est->stride;
  return AFE_OK;
}

void afe::estimator_announce_commit(afe_estimator *est, double from_s) { est->ring.push(from_s); }
