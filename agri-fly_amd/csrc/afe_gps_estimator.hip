// afe_gps_estimator.hip -- Offboard::GPSIMUStateEstimator for a whole ensemble on the device: the estimator the field node
// defaults to (ExampleVehicleStateMachine.cpp:11, :419), fed by CallbackIMU (:68-77, Predict on every IMU message, 500 Hz)
// and CallbackGPSEstimator (:79-85, UpdateWithMeasurement at 100 Hz) and read by EstGetState (:816-817, GetCurrentEstimate
// with no prediction ahead).  One lane per vehicle, reading the engine's slabs; the trajectory follower (afe_follower.hip)
// reads the estimate rows in place of the truth when one is attached.  The C ABI is in include/agrifly_engine.h
// ("GPS + IMU state estimator").
//
// THE DEFINITION is Components/Components/Offboard/GPSIMUStateEstimator.cpp, restated line by line in scalar Python
// (tests/gps_imu_reference.py) and in numpy (tests/gps_estimator_checker.py); kernels and checker must give the same bits,
// so the ORDER of the operations is part of the contract.  The class's own text is compiled where it lies by the test
// infrastructure's probe, against a recording dense stand-in for Eigen, and tests/test_gps_reference.py holds the
// restatement to what it recorded (tests/golden/gps_reference.npz): bit for bit outside Eigen, branch and finite /
// non-finite mask exactly, Eigen's finite results within derived bounds.  Everything is double, IEEE, uncontracted; + - * / sqrt and the
// conversions are correctly rounded on gfx950 and in numpy.  Only sin, cos and acosf are the device library's own:
// afe_gps_estimator_selftest_math evaluates the very helpers the kernels call.
//
// THE REFERENCE'S FLOAT AND OTHER QUIRKS, KEPT
//   * acosf(cosAngleError) (:90): the argument narrowed to float, the float result widened to double.  `if (errno)` is
//     restated as: |float(x)| > 1 gives double(M_PI) for x < 0 and 0 otherwise; a NaN argument gives NaN (acosf sets no
//     errno for it).  (Reset() at :68 has made the attitude the identity, so cosAngleError is the z component of a vector
//     divided by its own norm: no call through the ABI reaches the domain branch.  The definition's alignment is tested
//     on its own with other attitudes.)
//   * rotAx.GetNorm2() > 1e-6f (:84) compares against the float constant widened.
//   * measAcc.GetUnitVector() (:80; Vec3.hpp:126-129) divides by the norm NARROWED TO FLOAT and widened again.
//   * Vec3d(0, 0, -9.81f) (:117) is the float constant widened; the x and y sums with +0 are made.
//   * _lastMeasUpdateAttCorrection.z / 2.0f (:176-190) is a double division by 2.
//   * _lastMeasUpdateAttCorrection is not set by the constructor nor by Reset(): a Vec3d starts as NaN (Vec3.hpp:34-38).
//     The first ordinary Predict therefore makes the attitude rows and columns of the covariance NaN; the reference's
//     products are dense (NON-FINITE NUMBERS below), so the second makes all 81 entries NaN, and an update behind either
//     takes the singular branch; from there the filter runs.  (An update behind the alignment alone, with no ordinary
//     Predict between, is an ordinary update and overwrites the NaN correction: such a filter never restarts.)
//   * dt = _estimateTimer.GetSeconds<double>() (:107) is double(now_us - last_us) * 1e-6 (Timer.hpp:36-50).
//   * the first Predict calls Reset(), aligns the attitude to the measured gravity and returns (:67-103); an
//     UpdateWithMeasurement that arrives first sets _initialized, so the alignment never happens (:208-217).
//   * Rotationd::FromRotationVector, FromAxisAngle, Inverse, operator* and GetRotationMatrix as in Rotation.hpp (:66-97,
//     :124-137, :196-220), Rotate as :234-243.
//
// NON-FINITE NUMBERS are the dense algebra's.  f * _cov * f.transpose() (:195), H * (_cov * H.transpose()) (:224) and
//   (I - L H) * _cov (:255) are dense products in any evaluation by Eigen: they multiply by the structural zeros of f, H and
//   I - L H too, and 0 * NaN = 0 * Inf = NaN, whatever the order of summation.  So a covariance with ANY entry that is not
//   finite ("tainted") is non-finite in all 81 places after the next Predict, whatever f holds, and makes every entry of S
//   non-finite at the next UpdateWithMeasurement, which then takes :230-236.  The definition: a tainted covariance becomes
//   NaN everywhere in Predict (the dense product keeps an infinity at (i, j) for a lone infinity at (k, l) where f(i, k) and
//   f(j, l) are both non-zero; the mask is the same and nothing reads the difference before the restart), and a tainted
//   covariance is singular in the update.  For an untainted covariance the sparse order below and the dense products have
//   the same finite / non-finite mask (a non-finite entry of f or L meets every entry of its row either way), and the
//   finite bits are those of the sparse order; a zero keeps the sign the sparse order gives it (the dense sum's depends on
//   Eigen's order).  The kernels keep "tainted" as bit 1 of the per-vehicle `initialized` word: set where they store an
//   entry that is not finite, cleared by ResetVariance, recomputed by set_state when it is given a covariance.
//
// EVALUATION ORDER for finite numbers (Eigen's cannot be known here, so the definition fixes one).
//   Covariance prediction (:195): F = I + N, N the structurally non-zero off-identity entries of :133-191 (three dt, nine
//   of the velocity/attitude block, six off-diagonal of the attitude/attitude block).  T[i][j] = P[i][j] + sum_k N[i][k]
//   P[k][j], k ascending over row i's non-zeros, added left to right; C[i][j] = T[i][j] + sum_k T[i][k] N[j][k], k ascending
//   over row j's non-zeros; then the process noise as :197-202 writes it.
//   Update (:219-256): S = P[0:3][0:3] + sigma^2 I (the off-diagonal sums with +0 are made); det by cofactors along the
//   first row; Sinv = adj(S) (1 / det) entry by entry; L = P[:,0:3] Sinv, dx = L dpos, C = P - L P[0:3][:], each with k
//   ascending, (a b + c d) + e f; then 0.5 (C + C').  Singular (|det| < 1e-10, an entry of S not finite, or a
//   tainted covariance): :230-236.
//
// THE SAMPLE is what the simulator's GetAccelerometer / GetRateGyro return (Quadcopter_T.hpp:75-82): the logic's low-passed,
// mount-rotated values (QuadcopterLogic.hpp:40-52, :71-77).  The gyro value is the engine's own filter output (the ym1 rows
// of the slab rates_logic_tick keeps; no second filter).  The accelerometer is _R * Vec3f(acc) in float with the rounded
// products and sums of rates_logic_tick's mount product, through a LowPassFilterSecondOrder<float> (:22-64) with cutoff
// 100 rad/s (QuadcopterLogic.cpp:102) at float(logic period), coefficients computed on the host in float as afe_params.cpp
// does, state 0 at creation (:47).  It equals the reference vehicle's value only if the estimator is created before the
// first logic tick.
//
// LAYOUT.  Planar rows with the engine's stride S, one slab of 8-byte words and one base address in the kernel arguments:
// est[13] (pos 3, vel 3, att 4, angVel 3), two rows of +0 (so that est looks like an fp64 engine's slabs to the follower),
// cov[81] row major, corr[3] (_lastMeasUpdateAttCorrection), the time of the last Predict and of the last good update
// (uint64 us), and the accelerometer filter's xm0, xm1, ym0, ym1 (3 floats each: 12 float rows in 6 rows of words).
// initialized and numResets are a slab of 4-byte words; bit 0 of the first is _initialized, bit 1 "tainted".
//
// THE COVARIANCE IN PLACE.  Predict holds the three old attitude rows (27 doubles) and walks the pairs of position row i and
// velocity row 3 + i (the position row needs its own row and the old velocity row, which is loaded once and then serves
// its own update), then the attitude rows; each row of C is formed from its row of T before it is stored.  The
// update holds rows 0-2, loads the first three columns of the other rows for L, and then visits every pair (i, j), i <= j,
// once: both C[i][j] and C[j][i] are formed from words loaded once, and 0.5 (C[i][j] + C[j][i]) -- the same bits either way
// round -- is stored to both places.  Every word is read once and written once; nothing loops on data.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "afe_consumer.h"
#include "afe_device.h"
#include "afe_gps_estimator.h"

namespace {

constexpr int kBlock = 256;
constexpr int64_t kBlocksPerLaunch = int64_t(1) << 22;   // a launch stays below 2^31 threads
constexpr int kEstWords = 13, kCovWords = 81;
// rows of the one slab of 8-byte words (GpsArgs::slab, `stride` words a row) and of the one of 4-byte words (GpsArgs::flags)
constexpr int kRowEst = 0, kRowZero = 13, kRowCov = 15, kRowCorr = 96, kRowTPredict = 99, kRowTUpdate = 100, kRowLpf = 101, kRowEnd = 107;
constexpr int kFlagInit = 0, kFlagResets = 1, kFlagWords = 2;
constexpr uint32_t kInitBit = 1u, kTaintBit = 2u;        // of the kFlagInit word (NON-FINITE NUMBERS above)
constexpr double kMinAngle = 4.84813681e-6;              // Rotation.hpp: one arc second

// ---- the device library's functions, through the helpers both the kernels and the self-test call --------------------------
__device__ __forceinline__ void gm_sincos(double x, double *s, double *c) { *s = sin(x); *c = cos(x); }
__device__ __forceinline__ float gm_acosf(float x) { return acosf(x); }

struct V3 { double x, y, z; };
struct Q4 { double w, x, y, z; };

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
__device__ __forceinline__ double v_norm(const V3 &a) {                  // Vec3.hpp:101-119
#pragma clang fp contract(off)
  return sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
}
// Rotation.hpp:196-220
__device__ __forceinline__ void q_matrix(const Q4 &q, double R[9]) {
#pragma clang fp contract(off)
  const double r0 = q.w * q.w, r1 = q.x * q.x, r2 = q.y * q.y, r3 = q.z * q.z;
  R[0] = r0 + r1 - r2 - r3;
  R[1] = 2 * q.x * q.y - 2 * q.w * q.z;
  R[2] = 2 * q.x * q.z + 2 * q.w * q.y;
  R[3] = 2 * q.x * q.y + 2 * q.w * q.z;
  R[4] = r0 - r1 + r2 - r3;
  R[5] = 2 * q.y * q.z - 2 * q.w * q.x;
  R[6] = 2 * q.x * q.z - 2 * q.w * q.y;
  R[7] = 2 * q.y * q.z + 2 * q.w * q.x;
  R[8] = r0 - r1 - r2 + r3;
}
// Rotation.hpp:234-243
__device__ __forceinline__ V3 m_rotate(const double R[9], const V3 &a) {
#pragma clang fp contract(off)
  V3 o;
  o.x = R[0] * a.x + R[1] * a.y + R[2] * a.z;
  o.y = R[3] * a.x + R[4] * a.y + R[5] * a.z;
  o.z = R[6] * a.x + R[7] * a.y + R[8] * a.z;
  return o;
}
// Rotation.hpp:91-97: the unit vector is not checked
__device__ __forceinline__ Q4 q_from_axis_angle(const V3 &u, double angle) {
#pragma clang fp contract(off)
  double s, c;
  gm_sincos(angle * 0.5, &s, &c);
  Q4 q;
  q.w = c; q.x = s * u.x; q.y = s * u.y; q.z = s * u.z;
  return q;
}
// Rotation.hpp:84-89.  Without a branch: a lane below one arc second computes with theta = 1 and drops the result.
__device__ __forceinline__ Q4 q_from_rotvec(const V3 &r) {
#pragma clang fp contract(off)
  const double theta = v_norm(r);
  const bool small = theta < kMinAngle;
  const double th = small ? 1.0 : theta;
  V3 u;
  u.x = r.x / th; u.y = r.y / th; u.z = r.z / th;
  const Q4 a = q_from_axis_angle(u, th);
  Q4 q;
  q.w = small ? 1.0 : a.w; q.x = small ? 0.0 : a.x; q.y = small ? 0.0 : a.y; q.z = small ? 0.0 : a.z;
  return q;
}
// GPSIMUStateEstimator.cpp:90-98
__device__ __forceinline__ double align_angle(double cos_err) {
  const float xf = (float)cos_err;
  double angle = (double)gm_acosf(xf);
  if (fabsf(xf) > 1.0f) angle = cos_err < 0 ? (double)M_PI : 0.0;
  return angle;
}

struct GpsArgs {
  const void *pos;                         // the engine's slabs
  const double *anchor_xy;
  const float *acc, *lpf;                  // the raw accelerometer sample; the logic's filter state (gyro: rows 9-11 are ym1)
  const uint8_t *type;
  const afe::DevLogic *logic;              // per type: the mount matrix R
  int64_t stride, n;
  double *slab;                            // rows kRow*
  uint32_t *flags;                         // rows kFlag*
  unsigned long long *counter;
  double var_pos, var_vel, var_att;        // _initStdDev* squared
  double q_acc, q_gyro, r_pos;             // _measNoiseStdDev* squared
  float a1, a2, b0, b1, b2;                // the accelerometer low-pass
};

struct State {
  V3 x, v, w;
  Q4 q;
};

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
// the state of :35-39 / :210-214 / :230-234 around a position
__device__ __forceinline__ State fresh_state(const V3 &pos) {
  State s;
  s.x = pos;
  s.v.x = s.v.y = s.v.z = 0.0;
  s.w = s.v;
  s.q.w = 1.0; s.q.x = s.q.y = s.q.z = 0.0;
  return s;
}
// ResetVariance(), :46-54
__device__ __forceinline__ void store_fresh_cov(const GpsArgs &g, int64_t v) {
  double *C = g.slab + kRowCov * g.stride + v;
#pragma unroll
  for (int i = 0; i < 9; i++)
#pragma unroll
    for (int j = 0; j < 9; j++) C[(9 * i + j) * g.stride] = i != j ? 0.0 : i < 3 ? g.var_pos : i < 6 ? g.var_vel : g.var_att;
}
__device__ __forceinline__ float *lpf_rows(const GpsArgs &g) { return (float *)(g.slab + kRowLpf * g.stride); }

// Reset() for vehicles [first, first + count): :32-44, and (filter != 0) the accelerometer low-pass at 0
__global__ void __launch_bounds__(kBlock) afe_gps_estimator_reset_kernel(GpsArgs g, int64_t first, int64_t count, unsigned long long now_us, int filter,
                                                                         int construct) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  const int64_t v = first + i, S = g.stride;
  V3 zero;
  zero.x = zero.y = zero.z = 0.0;
  store_est(g.slab + kRowEst * S, S, v, fresh_state(zero));
  store_fresh_cov(g, v);
  unsigned long long *T = (unsigned long long *)g.slab;
  T[kRowTPredict * S + v] = now_us;
  T[kRowTUpdate * S + v] = now_us;
  g.flags[kFlagInit * S + v] = 0;
  g.flags[kFlagResets * S + v] = construct ? 1u : g.flags[kFlagResets * S + v] + 1u;
  if (construct) {                                                       // a Vec3d nobody has set: NaN (Vec3.hpp:34-38)
    const double nan = __builtin_nan("");
    g.slab[(kRowCorr + 0) * S + v] = nan; g.slab[(kRowCorr + 1) * S + v] = nan; g.slab[(kRowCorr + 2) * S + v] = nan;
  }
  if (filter) {
    float *F = lpf_rows(g);
#pragma unroll
    for (int k = 0; k < 12; k++) F[k * S + v] = 0.0f;
  }
}

// One row of C from one row of T (EVALUATION ORDER above): dt, nv[m][k] = N[3 + m][6 + k], na[m][k] = N[6 + m][6 + k] (the
// diagonal of na is not used)
__device__ __forceinline__ void c_row(const double t[9], double dt, const double nv[3][3], const double na[3][3], double c[9]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 3; j++) c[j] = t[j] + t[3 + j] * dt;
#pragma unroll
  for (int m = 0; m < 3; m++) c[3 + m] = ((t[3 + m] + t[6] * nv[m][0]) + t[7] * nv[m][1]) + t[8] * nv[m][2];
  c[6] = (t[6] + t[7] * na[0][1]) + t[8] * na[0][2];
  c[7] = (t[7] + t[6] * na[1][0]) + t[8] * na[1][2];
  c[8] = (t[8] + t[6] * na[2][0]) + t[7] * na[2][1];
}

// Predict(measAcc, measGyro) with the sample of the latest logic tick
__global__ void __launch_bounds__(kBlock) afe_gps_estimator_imu_kernel(GpsArgs g, unsigned long long now_us) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= g.n) return;
  const int64_t S = g.stride;
  // ---- the sample: QuadcopterLogic.hpp:47-52 and LowPassFilterSecondOrder.hpp:51-64 in float
  V3 acc, gyro;
  {
    const float *R = g.logic[g.type[v]].R;
    const float a[3] = {g.acc[v], g.acc[S + v], g.acc[2 * S + v]};
    float *F = lpf_rows(g);
    float out[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float in = ((0.0f + R[3 * k] * a[0]) + R[3 * k + 1] * a[1]) + R[3 * k + 2] * a[2];
      const float xm0 = F[k * S + v], xm1 = F[(3 + k) * S + v], ym0 = F[(6 + k) * S + v], ym1 = F[(9 + k) * S + v];
      float o = g.b2 * in;
      o = o + (+g.b0 * xm0 + g.b1 * xm1);
      o = o + (-g.a1 * ym0 - g.a2 * ym1);
      F[k * S + v] = xm1; F[(3 + k) * S + v] = in;
      F[(6 + k) * S + v] = ym1; F[(9 + k) * S + v] = o;
      out[k] = o;
    }
    acc.x = (double)out[0]; acc.y = (double)out[1]; acc.z = (double)out[2];
    gyro.x = (double)g.lpf[9 * S + v]; gyro.y = (double)g.lpf[10 * S + v]; gyro.z = (double)g.lpf[11 * S + v];
  }
  unsigned long long *T = (unsigned long long *)g.slab;
  double *E = g.slab + kRowEst * S;
  const uint32_t word = g.flags[kFlagInit * S + v];
  if (word == 0) {                                                        // :67-103
    V3 zero;
    zero.x = zero.y = zero.z = 0.0;
    State s = fresh_state(zero);                                          // Reset()
    store_fresh_cov(g, v);
    T[kRowTPredict * S + v] = now_us;
    T[kRowTUpdate * S + v] = now_us;
    g.flags[kFlagResets * S + v] = g.flags[kFlagResets * S + v] + 1u;
    g.flags[kFlagInit * S + v] = kInitBit;
    double R[9];
    q_matrix(q_inv(s.q), R);
    V3 e3;
    e3.x = 0.0; e3.y = 0.0; e3.z = 1.0;
    const V3 expected = m_rotate(R, e3);
    const double nf = (double)(float)v_norm(acc);                         // Vec3.hpp:126-129
    V3 unit;
    unit.x = acc.x / nf; unit.y = acc.y / nf; unit.z = acc.z / nf;
    const double cos_err = expected.x * unit.x + expected.y * unit.y + expected.z * unit.z;
    V3 ax;
    ax.x = unit.y * expected.z - unit.z * expected.y;
    ax.y = unit.z * expected.x - unit.x * expected.z;
    ax.z = unit.x * expected.y - unit.y * expected.x;
    const double an = v_norm(ax);
    if (an > (double)1e-6f) { const double d = v_norm(ax); ax.x = ax.x / d; ax.y = ax.y / d; ax.z = ax.z / d; }
    else { ax.x = 1.0; ax.y = 0.0; ax.z = 0.0; }
    s.q = q_mul(s.q, q_from_axis_angle(ax, align_angle(cos_err)));
    store_est(E, S, v, s);
    return;
  }
  const double dt = (double)(now_us - T[kRowTPredict * S + v]) * 1e-6;   // Timer.hpp:36-50
  T[kRowTPredict * S + v] = now_us;
  State s = load_est(E, S, v);
  double R[9];
  q_matrix(s.q, R);
  {                                                                       // :113-121
    const V3 ra = m_rotate(R, acc);
    V3 a;
    a.x = ra.x + 0.0; a.y = ra.y + 0.0; a.z = ra.z + (double)(-9.81f);
    State o;
    o.x.x = s.x.x + dt * s.v.x; o.x.y = s.x.y + dt * s.v.y; o.x.z = s.x.z + dt * s.v.z;
    o.v.x = s.v.x + dt * a.x; o.v.y = s.v.y + dt * a.y; o.v.z = s.v.z + dt * a.z;
    V3 rv;
    rv.x = dt * gyro.x; rv.y = dt * gyro.y; rv.z = dt * gyro.z;
    o.q = q_mul(s.q, q_from_rotvec(rv));
    o.w = gyro;
    store_est(E, S, v, o);
  }
  // ---- N (:133-191)
  double nv[3][3], na[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    nv[i][0] = dt * (+acc.y * R[3 * i + 2] - acc.z * R[3 * i + 1]);
    nv[i][1] = dt * (-acc.x * R[3 * i + 2] + acc.z * R[3 * i + 0]);
    nv[i][2] = dt * (+acc.x * R[3 * i + 1] - acc.y * R[3 * i + 0]);
  }
  {
    double *K = g.slab + kRowCorr * S + v;
    const double gx = dt * gyro.x + K[0] / 2.0, gy = dt * gyro.y + K[S] / 2.0, gz = dt * gyro.z + K[2 * S] / 2.0;
    na[0][0] = na[1][1] = na[2][2] = 0.0;
    na[1][0] = -gz; na[2][0] = +gy;
    na[0][1] = +gz; na[2][1] = -gx;
    na[0][2] = -gy; na[1][2] = +gx;
    K[0] = 0.0; K[S] = 0.0; K[2 * S] = 0.0;                               // :192
  }
  // ---- the covariance in place (:195-202)
  // a tainted covariance: NaN in all 81 places (the lane computes as the others do and stores NaN); an untainted one
  // becomes tainted by the first entry stored that is not finite
  const bool taint = (word & kTaintBit) != 0;
  const double nan = __builtin_nan("");
  bool bad = false;
  double *C = g.slab + kRowCov * S + v;
  double A[3][9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int j = 0; j < 9; j++) A[r][j] = C[(9 * (6 + r) + j) * S];
  const double pn_v = g.q_acc * dt * dt, pn_a = g.q_gyro * dt * dt;
#pragma unroll
  for (int i = 0; i < 3; i++) {                                           // position row i and velocity row 3 + i: the old
    double V[9], t[9], c[9];                                              // velocity row is loaded once and serves both
#pragma unroll
    for (int j = 0; j < 9; j++) V[j] = C[(9 * (3 + i) + j) * S];
#pragma unroll
    for (int j = 0; j < 9; j++) t[j] = C[(9 * i + j) * S] + dt * V[j];
    c_row(t, dt, nv, na, c);
#pragma unroll
    for (int j = 0; j < 9; j++) { bad = bad || !isfinite(c[j]); C[(9 * i + j) * S] = taint ? nan : c[j]; }
#pragma unroll
    for (int j = 0; j < 9; j++) t[j] = ((V[j] + nv[i][0] * A[0][j]) + nv[i][1] * A[1][j]) + nv[i][2] * A[2][j];
    c_row(t, dt, nv, na, c);
    c[3 + i] = c[3 + i] + pn_v;
#pragma unroll
    for (int j = 0; j < 9; j++) { bad = bad || !isfinite(c[j]); C[(9 * (3 + i) + j) * S] = taint ? nan : c[j]; }
  }
  {                                                                       // attitude rows
    double t[3][9];
#pragma unroll
    for (int j = 0; j < 9; j++) {
      t[0][j] = (A[0][j] + na[0][1] * A[1][j]) + na[0][2] * A[2][j];
      t[1][j] = (A[1][j] + na[1][0] * A[0][j]) + na[1][2] * A[2][j];
      t[2][j] = (A[2][j] + na[2][0] * A[0][j]) + na[2][1] * A[1][j];
    }
#pragma unroll
    for (int r = 0; r < 3; r++) {
      double c[9];
      c_row(t[r], dt, nv, na, c);
      c[6 + r] = c[6 + r] + pn_a;
#pragma unroll
      for (int j = 0; j < 9; j++) { bad = bad || !isfinite(c[j]); C[(9 * (6 + r) + j) * S] = taint ? nan : c[j]; }
    }
  }
  if (bad && !taint) g.flags[kFlagInit * S + v] = kInitBit | kTaintBit;
}

// UpdateWithMeasurement(the engine's position)
template <typename T>
__global__ void __launch_bounds__(kBlock) afe_gps_estimator_measure_kernel(GpsArgs g, unsigned long long now_us) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= g.n) return;
  const int64_t S = g.stride;
  V3 meas;
  {
    const T *P = (const T *)g.pos;
    meas.x = g.anchor_xy[v] + (double)P[v]; meas.y = g.anchor_xy[S + v] + (double)P[S + v]; meas.z = (double)P[2 * S + v];
  }
  double *E = g.slab + kRowEst * S;
  double *C = g.slab + kRowCov * S + v;
  const uint32_t word = g.flags[kFlagInit * S + v];
  bool reinit = word == 0;                                                // :208-217
  bool singular = false;
  double P0[3][9];
  double det = 0.0, co[3][3];
  if (!reinit) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 9; j++) P0[i][j] = C[(9 * i + j) * S];
    double Sm[3][3];
    bool finite = (word & kTaintBit) == 0;                                // dense: a tainted covariance makes S non-finite
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        Sm[i][j] = P0[i][j] + (i == j ? g.r_pos : 0.0);
        finite = finite && isfinite(Sm[i][j]);
      }
    // adj(S), entry by entry
    co[0][0] = Sm[1][1] * Sm[2][2] - Sm[1][2] * Sm[2][1];
    co[0][1] = Sm[0][2] * Sm[2][1] - Sm[0][1] * Sm[2][2];
    co[0][2] = Sm[0][1] * Sm[1][2] - Sm[0][2] * Sm[1][1];
    co[1][0] = Sm[1][2] * Sm[2][0] - Sm[1][0] * Sm[2][2];
    co[1][1] = Sm[0][0] * Sm[2][2] - Sm[0][2] * Sm[2][0];
    co[1][2] = Sm[0][2] * Sm[1][0] - Sm[0][0] * Sm[1][2];
    co[2][0] = Sm[1][0] * Sm[2][1] - Sm[1][1] * Sm[2][0];
    co[2][1] = Sm[0][1] * Sm[2][0] - Sm[0][0] * Sm[2][1];
    co[2][2] = Sm[0][0] * Sm[1][1] - Sm[0][1] * Sm[1][0];
    det = (Sm[0][0] * (Sm[1][1] * Sm[2][2] - Sm[1][2] * Sm[2][1]) - Sm[0][1] * (Sm[1][0] * Sm[2][2] - Sm[1][2] * Sm[2][0])) +
          Sm[0][2] * (Sm[1][0] * Sm[2][1] - Sm[1][1] * Sm[2][0]);
    singular = fabs(det) < 1e-10 || !finite;                               // :228
    reinit = singular;
  }
  if (g.counter) {                                                        // one ballot of the lanes still here, one atomic by the first
    const unsigned long long mask = __ballot(singular);
    if (mask && (int)(threadIdx.x & 63) == __ffsll((long long)mask) - 1) atomicAdd(g.counter, (unsigned long long)__popcll(mask));
  }
  if (reinit) {                                                           // :209-216, :230-236
    if (word != kInitBit) g.flags[kFlagInit * S + v] = kInitBit;          // ResetVariance() clears the taint
    store_est(E, S, v, fresh_state(meas));
    store_fresh_cov(g, v);
    return;
  }
  bool bad = false;                                                       // an entry stored that is not finite taints
  const double rdet = 1 / det;
  double Si[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) Si[i][j] = co[i][j] * rdet;
  // L = P[:, 0:3] Sinv: rows 0-2 from what is held, rows 3-8 from their first three words
  double L[9][3];
#pragma unroll
  for (int i = 0; i < 9; i++) {
    double p[3];
#pragma unroll
    for (int k = 0; k < 3; k++) p[k] = i < 3 ? P0[i][k] : C[(9 * i + k) * S];
#pragma unroll
    for (int j = 0; j < 3; j++) L[i][j] = (p[0] * Si[0][j] + p[1] * Si[1][j]) + p[2] * Si[2][j];
    // C[i][0:3] and C[0:3][i] for i >= 3 need p again: the pairs (k, i), k < 3, are made here
    if (i >= 3) {
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const double cki = P0[k][i] - ((L[k][0] * P0[0][i] + L[k][1] * P0[1][i]) + L[k][2] * P0[2][i]);
        const double cik = p[k] - ((L[i][0] * P0[0][k] + L[i][1] * P0[1][k]) + L[i][2] * P0[2][k]);
        const double sym = 0.5 * (cki + cik);
        bad = bad || !isfinite(sym);
        C[(9 * k + i) * S] = sym; C[(9 * i + k) * S] = sym;
      }
    }
  }
  State s = load_est(E, S, v);
  {                                                                       // :243-252
    const double d0 = meas.x - s.x.x, d1 = meas.y - s.x.y, d2 = meas.z - s.x.z;
    double dx[9];
#pragma unroll
    for (int i = 0; i < 9; i++) dx[i] = (L[i][0] * d0 + L[i][1] * d1) + L[i][2] * d2;
    s.x.x = s.x.x + dx[0]; s.x.y = s.x.y + dx[1]; s.x.z = s.x.z + dx[2];
    s.v.x = s.v.x + dx[3]; s.v.y = s.v.y + dx[4]; s.v.z = s.v.z + dx[5];
    V3 corr;
    corr.x = dx[6]; corr.y = dx[7]; corr.z = dx[8];
    s.q = q_mul(s.q, q_from_rotvec(corr));
    double *K = g.slab + kRowCorr * S + v;
    K[0] = corr.x; K[S] = corr.y; K[2 * S] = corr.z;
    store_est(E, S, v, s);
  }
  // the pairs inside rows and columns 0-2 (held), then those inside 3-8 (each word loaded once)
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = i; j < 3; j++) {
      const double cij = P0[i][j] - ((L[i][0] * P0[0][j] + L[i][1] * P0[1][j]) + L[i][2] * P0[2][j]);
      const double cji = P0[j][i] - ((L[j][0] * P0[0][i] + L[j][1] * P0[1][i]) + L[j][2] * P0[2][i]);
      const double sym = 0.5 * (cij + cji);
      bad = bad || !isfinite(sym);
      C[(9 * i + j) * S] = sym; C[(9 * j + i) * S] = sym;
    }
#pragma unroll
  for (int i = 3; i < 9; i++)
#pragma unroll
    for (int j = i; j < 9; j++) {
      const double pij = C[(9 * i + j) * S], pji = C[(9 * j + i) * S];
      const double cij = pij - ((L[i][0] * P0[0][j] + L[i][1] * P0[1][j]) + L[i][2] * P0[2][j]);
      const double cji = pji - ((L[j][0] * P0[0][i] + L[j][1] * P0[1][i]) + L[j][2] * P0[2][i]);
      const double sym = 0.5 * (cij + cji);
      bad = bad || !isfinite(sym);
      C[(9 * i + j) * S] = sym; C[(9 * j + i) * S] = sym;
    }
  if (bad) g.flags[kFlagInit * S + v] = kInitBit | kTaintBit;
  ((unsigned long long *)g.slab)[kRowTUpdate * S + v] = now_us;          // :257
}

// set_state: mark vehicles [first, first + count) initialised; with a covariance given, tainted is what that covariance says
__global__ void __launch_bounds__(kBlock) afe_gps_estimator_mark_kernel(GpsArgs g, int64_t first, int64_t count, int have_cov) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  const int64_t S = g.stride, v = first + i;
  uint32_t taint = g.flags[kFlagInit * S + v] & kTaintBit;
  if (have_cov) {
    const double *C = g.slab + kRowCov * S + v;
    bool bad = false;
    for (int k = 0; k < kCovWords; k++) bad = bad || !isfinite(C[k * S]);
    taint = bad ? kTaintBit : 0u;
  }
  g.flags[kFlagInit * S + v] = kInitBit | taint;
}

__global__ void __launch_bounds__(kBlock) afe_gps_estimator_math_kernel(int op, int64_t n, const double *x, double *y) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double s, c;
  gm_sincos(x[i], &s, &c);
  y[i] = op == 0 ? s : op == 1 ? c : (double)gm_acosf((float)x[i]);
}

size_t up256(size_t x) { return (x + 255) & ~size_t(255); }

}  // namespace

struct afe_gps_estimator {
  afe_engine *engine = nullptr;     // borrowed
  int device = 0;
  int64_t n = 0, stride = 0;
  uint64_t t0_us = 0;               // afe_time_us at creation: every time is relative to it
  uint64_t n_imu = 0, n_measures = 0, last_tick = 0;
  float cutoff = 100.0f;
  afe::DevBuf arena;
  GpsArgs args;
};

namespace {

struct Entry {
  hipStream_t stream;
  GpsArgs g;
  int elem;
  uint64_t now_us, n_ticks;
  float period;
};

// through the engine's gate (a resident grid ends here); the handle against what it got; the clock and the logic
int enter(afe_gps_estimator *est, Entry *en) {
  afe::EngineAccess acc;
  int rc = afe::engine_enter(est->engine, &acc);
  if (rc != AFE_OK) return rc;
  const afe_device_view &view = acc.view;
  if (view.n_vehicles != est->n || view.stride != est->stride || acc.device != est->device) return AFE_ERR_INVALID_ARG;
  en->stream = acc.stream;
  en->g = est->args;
  en->g.pos = view.pos; en->g.anchor_xy = view.pos_anchor_xy; en->g.acc = view.acc; en->g.type = view.type_index;
  en->elem = view.state_elem_size;
  rc = afe::engine_logic_filter(est->engine, &en->g.lpf, &en->g.logic, &en->period, &en->n_ticks);
  if (rc != AFE_OK) return rc;
  uint64_t now = 0;
  rc = afe_time_us(est->engine, &now);
  if (rc != AFE_OK) return rc;
  if (now < est->t0_us) return AFE_ERR_OUT_OF_RANGE;                       // (the engine's clock was set back)
  en->now_us = now - est->t0_us;
  return AFE_OK;
}

dim3 grid_for(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }
bool launched() { return hipGetLastError() == hipSuccess; }

int enter_rows(afe_gps_estimator *est, int64_t first, int64_t count) {
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

// LowPassFilterSecondOrder<float, ...>::Initialise, LowPassFilterSecondOrder.hpp:22-49 (as afe_params.cpp expand_logic)
void lowpass_coefficients(float dt, float wc, GpsArgs *g) {
  const float sqrt2 = float(std::sqrt(2.0));
  g->a1 = (dt * dt * wc * wc - 2 * sqrt2 * dt * wc + 4) / (dt * dt * wc * wc + 2 * sqrt2 * dt * wc + 4);
  g->a2 = 2 * (dt * dt * wc * wc - 4) / (dt * dt * wc * wc + 2 * sqrt2 * dt * wc + 4);
  g->b0 = dt * dt * wc * wc / (dt * dt * wc * wc + 2 * sqrt2 * dt * wc + 4);
  g->b1 = dt * dt * wc * wc / (dt * dt * wc * wc + 2 * sqrt2 * dt * wc + 4);
  g->b2 = 2 * dt * dt * wc * wc / (dt * dt * wc * wc + 2 * sqrt2 * dt * wc + 4);
}

bool sigma_ok(double s, bool positive) { return std::isfinite(s) && (positive ? s > 0 : s >= 0); }

}  // namespace

extern "C" int afe_gps_estimator_default_config(afe_gps_estimator_config *cfg) {
  if (!cfg) return AFE_ERR_INVALID_ARG;
  afe_gps_estimator_config c;
  std::memset(&c, 0, sizeof(c));
  c.struct_bytes = sizeof(c);
  c.init_sigma_pos = 3.0;                               // GPSIMUStateEstimator.cpp:21-27
  c.init_sigma_vel = 3.0;
  c.init_sigma_att = 10.0 * double(M_PI) / 180.0;
  c.sigma_acc = 5;
  c.sigma_gyro = 0.1;
  c.sigma_pos = 0.25;
  c.accel_lowpass_cutoff = 100.0f;                      // QuadcopterLogic.cpp:102
  *cfg = c;
  return AFE_OK;
}

extern "C" int afe_gps_estimator_create(afe_engine *e, const afe_gps_estimator_config *cfg, afe_gps_estimator **out) {
  if (!e || !cfg || !out || cfg->struct_bytes < sizeof(afe_gps_estimator_config)) return AFE_ERR_INVALID_ARG;
  if (!sigma_ok(cfg->init_sigma_pos, false) || !sigma_ok(cfg->init_sigma_vel, false) || !sigma_ok(cfg->init_sigma_att, false) ||
      !sigma_ok(cfg->sigma_acc, false) || !sigma_ok(cfg->sigma_gyro, false) || !sigma_ok(cfg->sigma_pos, false) ||
      !sigma_ok(cfg->accel_lowpass_cutoff, true))
    return AFE_ERR_INVALID_ARG;
  afe::EngineAccess acc;
  int rc = afe::engine_enter(e, &acc);
  if (rc != AFE_OK) return rc;
  rc = afe::engine_device_resident(e);
  if (rc != AFE_OK) return rc;
  const float *lpf = nullptr;
  const afe::DevLogic *logic = nullptr;
  float period = 0;
  uint64_t ticks = 0, now_us = 0;
  rc = afe::engine_logic_filter(e, &lpf, &logic, &period, &ticks);
  if (rc != AFE_OK) return rc;
  rc = afe_time_us(e, &now_us);
  if (rc != AFE_OK) return rc;
  afe_gps_estimator *est = new afe_gps_estimator();
  est->engine = e; est->device = acc.device; est->n = acc.view.n_vehicles; est->stride = acc.view.stride;
  est->t0_us = now_us; est->cutoff = cfg->accel_lowpass_cutoff;
  const size_t S = (size_t)est->stride;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += up256(bytes); return o; };
  const size_t o_slab = take(S * 8 * (size_t)kRowEnd), o_flags = take(S * 4 * kFlagWords), o_cnt = take(8);
  if (!est->arena.alloc(off)) {
    (void)hipGetLastError();
    delete est;
    return AFE_ERR_HIP;
  }
  unsigned char *A = est->arena.as<unsigned char>();
  std::memset(&est->args, 0, sizeof(est->args));
  GpsArgs &g = est->args;
  g.n = est->n; g.stride = est->stride;
  g.slab = (double *)(A + o_slab); g.flags = (uint32_t *)(A + o_flags);
  g.counter = (unsigned long long *)(A + o_cnt);
  g.var_pos = cfg->init_sigma_pos * cfg->init_sigma_pos;
  g.var_vel = cfg->init_sigma_vel * cfg->init_sigma_vel;
  g.var_att = cfg->init_sigma_att * cfg->init_sigma_att;
  g.q_acc = cfg->sigma_acc * cfg->sigma_acc;
  g.q_gyro = cfg->sigma_gyro * cfg->sigma_gyro;
  g.r_pos = cfg->sigma_pos * cfg->sigma_pos;
  const hipStream_t stream = acc.stream;
  rc = hipMemsetAsync(A, 0, off, stream) == hipSuccess ? AFE_OK : AFE_ERR_HIP;      // padding and the +0 anchors included
  if (rc == AFE_OK && est->n > 0) {
    if (est->n > kBlocksPerLaunch * kBlock) rc = AFE_ERR_OUT_OF_RANGE;
    else {
      hipLaunchKernelGGL(afe_gps_estimator_reset_kernel, grid_for(est->n), dim3(kBlock), 0, stream, g, (int64_t)0, est->n, 0ull, 1, 1);
      if (!launched()) rc = AFE_ERR_HIP;
    }
  }
  if (rc == AFE_OK && hipStreamSynchronize(stream) != hipSuccess) rc = AFE_ERR_HIP;
  if (rc != AFE_OK) { (void)hipGetLastError(); (void)afe_gps_estimator_destroy(est); return rc; }
  *out = est;
  return AFE_OK;
}

extern "C" int afe_gps_estimator_destroy(afe_gps_estimator *est) {
  if (!est) return AFE_ERR_INVALID_ARG;
  (void)hipSetDevice(est->device);
  (void)hipDeviceSynchronize();
  delete est;
  return AFE_OK;
}

extern "C" int afe_gps_estimator_info(const afe_gps_estimator *est, int64_t *n_vehicles, uint64_t *n_imu, uint64_t *n_measures, uint64_t *last_tick) {
  if (!est) return AFE_ERR_INVALID_ARG;
  if (n_vehicles) *n_vehicles = est->n;
  if (n_imu) *n_imu = est->n_imu;
  if (n_measures) *n_measures = est->n_measures;
  if (last_tick) *last_tick = est->last_tick;
  return AFE_OK;
}

extern "C" int afe_gps_estimator_imu(afe_gps_estimator *est) {
  if (!est) return AFE_ERR_INVALID_ARG;
  Entry en;
  const int rc = enter(est, &en);
  if (rc != AFE_OK) return rc;
  // every sample exactly once: the tick after the one consumed last (the first call: any tick at all)
  if (est->n_imu == 0 ? en.n_ticks < 1 : en.n_ticks != est->last_tick + 1) return AFE_ERR_NOT_CONFIGURED;
  if (est->n > 0) {
    lowpass_coefficients(en.period, est->cutoff, &en.g);
    hipLaunchKernelGGL(afe_gps_estimator_imu_kernel, grid_for(en.g.n), dim3(kBlock), 0, en.stream, en.g, (unsigned long long)en.now_us);
    if (!launched()) return AFE_ERR_HIP;
  }
  est->last_tick = en.n_ticks;
  est->n_imu++;
  return AFE_OK;
}

extern "C" int afe_gps_estimator_measure(afe_gps_estimator *est, int64_t *n_reinitialised) {
  if (!est) return AFE_ERR_INVALID_ARG;
  Entry en;
  const int rc = enter(est, &en);
  if (rc != AFE_OK) return rc;
  GpsArgs &g = en.g;
  if (n_reinitialised) {
    if (hipMemsetAsync(g.counter, 0, 8, en.stream) != hipSuccess) return AFE_ERR_HIP;
  } else g.counter = nullptr;
  if (est->n > 0) {
    if (en.elem == 8) hipLaunchKernelGGL(afe_gps_estimator_measure_kernel<double>, grid_for(g.n), dim3(kBlock), 0, en.stream, g, (unsigned long long)en.now_us);
    else hipLaunchKernelGGL(afe_gps_estimator_measure_kernel<float>, grid_for(g.n), dim3(kBlock), 0, en.stream, g, (unsigned long long)en.now_us);
    if (!launched()) return AFE_ERR_HIP;
  }
  est->n_measures++;
  if (n_reinitialised) {
    unsigned long long k = 0;
    if (hipMemcpyAsync(&k, g.counter, 8, hipMemcpyDeviceToHost, en.stream) != hipSuccess || hipStreamSynchronize(en.stream) != hipSuccess)
      return AFE_ERR_HIP;
    *n_reinitialised = (int64_t)k;
  }
  return AFE_OK;
}

extern "C" int afe_gps_estimator_get_state(afe_gps_estimator *est, int64_t first, int64_t count, double *est13, double *cov81, uint64_t *last_predict_us,
                                           uint64_t *last_update_us, uint8_t *initialized, uint32_t *num_resets) {
  const int arc = enter_rows(est, first, count);
  if (arc != AFE_OK) return arc;
  if (!est13 && !cov81 && !last_predict_us && !last_update_us && !initialized && !num_resets) return AFE_ERR_INVALID_ARG;
  if (count == 0) return AFE_OK;
  Entry en;
  const int rc = enter(est, &en);
  if (rc != AFE_OK) return rc;
  if (hipStreamSynchronize(en.stream) != hipSuccess) return AFE_ERR_HIP;
  const GpsArgs &g = est->args;
  const int64_t S = est->stride;
  if ((est13 && !get_rows(g.slab + kRowEst * S, 8, kEstWords, S, first, count, est13)) ||
      (cov81 && !get_rows(g.slab + kRowCov * S, 8, kCovWords, S, first, count, cov81)) ||
      (last_predict_us && !get_rows(g.slab + kRowTPredict * S, 8, 1, S, first, count, last_predict_us)) ||
      (last_update_us && !get_rows(g.slab + kRowTUpdate * S, 8, 1, S, first, count, last_update_us)) ||
      (num_resets && !get_rows(g.flags + kFlagResets * S, 4, 1, S, first, count, num_resets)))
    return AFE_ERR_HIP;
  if (initialized) {                                                        // a 4-byte word on the device, a byte for the caller
    std::vector<uint32_t> word((size_t)count);
    if (!get_rows(g.flags + kFlagInit * S, 4, 1, S, first, count, word.data())) return AFE_ERR_HIP;
    for (int64_t i = 0; i < count; i++) initialized[i] = word[(size_t)i] ? 1 : 0;
  }
  return AFE_OK;
}

extern "C" int afe_gps_estimator_set_state(afe_gps_estimator *est, int64_t first, int64_t count, const double *est13, const double *cov81,
                                           const double *corr3) {
  const int arc = enter_rows(est, first, count);
  if (arc != AFE_OK) return arc;
  if (!est13 && !cov81 && !corr3) return AFE_ERR_INVALID_ARG;
  if (count == 0) return AFE_OK;
  Entry en;
  const int rc = enter(est, &en);
  if (rc != AFE_OK) return rc;
  if (hipStreamSynchronize(en.stream) != hipSuccess) return AFE_ERR_HIP;
  const GpsArgs &g = est->args;
  const int64_t S = est->stride;
  if ((est13 && !put_rows(g.slab + kRowEst * S, 8, kEstWords, S, first, count, est13)) ||
      (cov81 && !put_rows(g.slab + kRowCov * S, 8, kCovWords, S, first, count, cov81)) ||
      (corr3 && !put_rows(g.slab + kRowCorr * S, 8, 3, S, first, count, corr3)))
    return AFE_ERR_HIP;
  hipLaunchKernelGGL(afe_gps_estimator_mark_kernel, grid_for(count), dim3(kBlock), 0, en.stream, en.g, first, count, cov81 ? 1 : 0);
  return launched() ? AFE_OK : AFE_ERR_HIP;
}

extern "C" int afe_gps_estimator_reset(afe_gps_estimator *est, int64_t first, int64_t count) {
  const int arc = enter_rows(est, first, count);
  if (arc != AFE_OK) return arc;
  if (count == 0) return AFE_OK;
  Entry en;
  const int rc = enter(est, &en);
  if (rc != AFE_OK) return rc;
  hipLaunchKernelGGL(afe_gps_estimator_reset_kernel, grid_for(count), dim3(kBlock), 0, en.stream, en.g, first, count, (unsigned long long)en.now_us, 1, 0);
  return launched() ? AFE_OK : AFE_ERR_HIP;
}

extern "C" int afe_gps_estimator_selftest_math(int device, int op, int64_t n, const double *x, double *y) {
  if (!x || !y || op < 0 || op > 2 || n < 0) return AFE_ERR_INVALID_ARG;
  if (n == 0) return AFE_OK;
  if (n > kBlocksPerLaunch * kBlock) return AFE_ERR_OUT_OF_RANGE;
  const int prc = afe::pick_gfx950(device, &device);
  if (prc != AFE_OK) return prc;
  const size_t bytes = (size_t)n * 8;
  afe::DevBuf dx, dy;
  if (!dx.upload(x, bytes) || !dy.alloc(bytes)) { (void)hipGetLastError(); return AFE_ERR_HIP; }
  hipLaunchKernelGGL(afe_gps_estimator_math_kernel, grid_for(n), dim3(kBlock), 0, nullptr, op, n, dx.as<double>(), dy.as<double>());
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return AFE_ERR_HIP;
  return dy.download(y, bytes) ? AFE_OK : AFE_ERR_HIP;
}

// ---- for the follower (afe_gps_estimator.h) -------------------------------------------------------------------------------------
int afe::gps_estimator_check_engine(const afe_gps_estimator *est, const afe_engine *e) {
  return est && est->engine == e ? AFE_OK : AFE_ERR_INVALID_ARG;
}

int afe::gps_estimator_link(afe_gps_estimator *est, uint64_t n_ticks, EstimatorLink *out) {
  if (est->n_imu == 0 || est->last_tick != n_ticks) return AFE_ERR_NOT_CONFIGURED;
  const int64_t S = est->stride;
  const double *E = est->args.slab + kRowEst * S;
  out->pos = E; out->vel = E + 3 * S; out->att = E + 6 * S;
  out->zero_anchor_xy = est->args.slab + kRowZero * S;
  return AFE_OK;
}

int afe::gps_estimator_last_update(afe_gps_estimator *est, const unsigned long long **t_update_us, uint64_t *origin_us) {
  if (!est || !t_update_us || !origin_us) return AFE_ERR_INVALID_ARG;
  *t_update_us = (const unsigned long long *)est->args.slab + kRowTUpdate * est->stride;
  *origin_us = est->t0_us;
  return AFE_OK;
}
