// afe_onboard.hip -- the onboard flight computer: what Onboard::QuadcopterLogic::Run does at a logic tick beyond the rates slice
// the step kernel runs (Components/Components/Logic/QuadcopterLogic.cpp:164-219, QuadcopterLogic.hpp, and the complementary
// branch of KalmanFilter6DOF::Predict, KalmanFilter6DOF.cpp:70-147), with what Quadcopter_T.cpp:163-185 hands it, for the case
// WITHOUT UWB ranging.  One lane per vehicle, planar slabs of its own, one kernel per logic tick behind the step that fired it.
// The C ABI is in include/agrifly_engine.h ("onboard flight computer").  No step kernel knows about it.
//
// THE DEFINITION (tests/onboard_checker.py restates it in numpy; kernel and checker must give the same bits, so the ORDER below
// is part of the contract).  Everything is float, contraction is off, division and square root are IEEE, as in rates_logic_tick
// (afe_kernels.hip).  Only sinf, cosf, acosf, asinf, atan2f are the device library's own: afe_onboard_selftest_math evaluates the
// very helpers the kernel calls (afe_offboard_math.h).  T is the clock of the tick: the engine clock at the START of the step
// that fired it.  A Timer is the uint64 time of its last reset; GetSeconds_f() is float(T - reset) * 1e-6f.
//
//   0 RADIO        a mailbox entry with arrival <= T is SetRadioMessage at its arrival time ta: flags and type are taken, the radio
//                  timer is reset to ta, _monitorCmdRate.Update() runs at ta, the entry is cleared.  Update() is
//                  dt = float(ta - reset) * 1e-6f;  lpDt = c * lpDt + (1 - c) * dt;  reset += uint64(dt * 1e6f)  (AdjustTimeBySeconds
//                  truncates: the timer drifts by the microseconds the product loses, as in the reference)
//   1 BATTERY      voltageFiltered = second-order low-pass of the vehicle's voltage slab (LowPassFilterSecondOrder.hpp:51-64)
//   2 IMU          acc = _R * raw accelerometer sample of the engine, low-passed;  temperature low-pass of 25;  gyro = the engine's own
//                  filter output (rows 9-11 of its lpf slab)
//   3 MONITOR      _cycleCounter++;  _monitorMainLoopPeriod.Update() at T
//   4 PREDICT      first call: att = identity, angVel = 0, estimate timer = T, reset timer = T (GetWasResetSinceLastCheck), then
//                  att = att * FromAxisAngle(axis, angle) with expAcc = M(att^-1) e3, u = acc / |acc|, cos = expAcc . u,
//                  axis = u x expAcc, normalised if its norm > 1e-6f else (1, 0, 0), angle = guarded_acosf(cos)
//                  later: dt = float(T - estimate timer) * 1e-6f, timer = T;  angVel = gyro;  att = att * FromRotationVector(gyro * dt);
//                  the same axis and angle from the new att;  att = att * FromAxisAngle(axis, (dt / 4.0f) * angle)
//   5 PARSE        a new message changes the state unless it is PANIC or KILLED: 2 -> KILLED (the first one records reason 7),
//                  4 -> ACCELERATION, 5 -> RATES, 6 -> IDLE, 3 -> FULLY_AUTONOMOUS (never delivered: afe_onboard_radio refuses it)
//   6 WARNINGS     0x01 voltageFiltered <= 1.05f * threshold;  0x02 |cmd lpDt - radio period| > 0.1f * radio period;
//                  0x10 float(T - radio timer) * 1e-6f > 3 * radio period;  0x08 |main lpDt - period| > 0.05f * period;
//                  0x04 float(T - reset timer) * 1e-6f < 0.02f
//   7 PANIC        only if the motors ran after the PREVIOUS tick: reason = 0;  estimated z (0) < -2 and not flag 0x02 -> 1 (cannot
//                  fire, kept);  T - uwb timer > 1 500 000 and state FULLY_AUTONOMOUS -> 2 (cannot fire, kept);
//                  (M(att) e3).z < 0 and not flag 0x02 -> 3;  T - radio timer > 1 500 000 -> 4;  voltageFiltered <= threshold -> 5.
//                  A later check overrides an earlier one.  reason != 0 in a safety-critical state (not 0, 1, 3, 4) that is not
//                  PANIC already: state = PANIC, first panic reason = reason.
//   8 CONTROLLER   RATES: the step kernel's command stands; the four forces are recomputed for telemetry from the rates command AS THE
//                  SLAB HOLDS IT NOW.  A delivery made between the ticking step and this tick is held back for parsing (item 0) but
//                  its floats are in the slab already: for that one tick the forces of a rates-state vehicle come from the new
//                  command while the motor command is the step kernel's from the old one.  Deliver between ticks.
//                  ACCELERATION: RunControllerExternalAcceleration (QuadcopterLogic.cpp:459-526) -> four motor speeds into the
//                  engine's command slab.  Everything else: zeros into the command slab and the forces.
//                  motors running = any of the four commands in force > 0.
//   9 COUNTERS     after the tick: vehicles per state [0..6], per first panic reason [7..14], with any warning bit [15].
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "afe_consumer.h"
#include "afe_device.h"
#include "afe_offboard_math.h"

namespace {

using namespace afe_offboard;
using afe::DevLogic;

constexpr int kBlock = 256;
constexpr int64_t kBlocksPerLaunch = int64_t(1) << 22;   // a launch stays below 2^31 threads
// float rows
constexpr int kFAtt = 0, kFAngVel = 4, kFAccLp = 7, kFBattLp = 19, kFTempLp = 23, kFMainDt = 27, kFCmdDt = 28, kFForces = 29, kFVolt = 33,
              kFRadio = 34, kFloats = 38;
// uint64 rows: the timers' reset times
constexpr int kTMain = 0, kTCmd = 1, kTRadio = 2, kTEst = 3, kTReset = 4, kTUwb = 5, kTimes = 6;
// byte rows
constexpr int kBState = 0, kBReason = 1, kBWarn = 2, kBRunning = 3, kBInit = 4, kBFlags = 5, kBytes = 6;
// uint32 rows
constexpr int kUCycle = 0, kUPacket = 1, kWords = 2;

struct Lp2 { float a1, a2, b0, b1, b2; };
// per type record, device memory
struct OnbType {
  Lp2 acc, batt, temp;
  float c_main, c_cmd;          // LowPassFilterFirstOrder::_coefficient of the two monitors
  float tc_xy, tc_z;            // QuadcopterAttitudeController
  float v_crit, v_warn;
  float period, radio_period;
};

struct OnbArgs {
  // the engine's
  const float *acc;             // raw accelerometer sample [3]
  const float *lpf;             // the rates logic's filter state [12]: rows 9-11 are the filtered gyro
  const float *rates_cmd;       // [4]
  float *motor_cmd;             // [4]
  const uint8_t *type;
  const DevLogic *logic;
  int64_t stride, n;
  // the computer's own slabs, the same stride
  float *f;                     // [kFloats]
  unsigned long long *t;        // [kTimes]
  uint8_t *b;                   // [kBytes]
  uint32_t *u;                  // [kWords]
  unsigned long long *mail_arrival;
  uint8_t *mail_type, *mail_flags;
  const OnbType *types;
  unsigned long long *counters; // [16], or NULL: not counted
};

// LowPassFilterSecondOrder::Apply, LowPassFilterSecondOrder.hpp:51-64
__device__ __forceinline__ float lp2_apply(const Lp2 &k, float in, float &xm0, float &xm1, float &ym0, float &ym1) {
#pragma clang fp contract(off)
  float out = k.b2 * in;
  out = out + (+k.b0 * xm0 + k.b1 * xm1);
  out = out + (-k.a1 * ym0 - k.a2 * ym1);
  xm0 = xm1; xm1 = in;
  ym0 = ym1; ym1 = out;
  return out;
}
// MonitorSimplePeriod::Update, QuadcopterLogic.hpp:394-398 (LowPassFilterFirstOrder::Apply, Timer::AdjustTimeBySeconds)
__device__ __forceinline__ void monitor_update(float c, unsigned long long now, unsigned long long &reset, float &lp) {
#pragma clang fp contract(off)
  const float dt = (float)(now - reset) * 1e-6f;
  if (c <= 0.0f) lp = dt;
  else lp = c * lp + (1 - c) * dt;
  reset += (unsigned long long)(dt * 1e6f);               // (-dt) * float(-1e6): the same product
}
// the gravity correction's axis and angle, KalmanFilter6DOF.cpp:83-103 and :121-141 (the same lines twice)
__device__ __forceinline__ void gravity_axis_angle(const Q4f &att, const V3f &acc, V3f *axis, float *angle) {
#pragma clang fp contract(off)
  V3f e3;
  e3.x = 0.0f; e3.y = 0.0f; e3.z = 1.0f;
  const V3f expAcc = mf_rotate(qf_matrix(qf_inv(att)), e3);
  const float na = sqrtf(vf_dot(acc, acc));
  V3f u;
  u.x = acc.x / na; u.y = acc.y / na; u.z = acc.z / na;
  const float c = vf_dot(expAcc, u);
  V3f ax = vf_cross(u, expAcc);
  const float nr = sqrtf(vf_dot(ax, ax));
  if (nr > 1e-6f) { ax.x = ax.x / nr; ax.y = ax.y / nr; ax.z = ax.z / nr; }
  else { ax.x = 1.0f; ax.y = 0.0f; ax.z = 0.0f; }        // "somewhat arbitrary"
  *axis = ax;
  *angle = guarded_acosf(c);
}
// GetDesiredTorques, GetMotorForces and PropellerSpeedsFromThrust as rates_logic_tick (afe_kernels.hip) states them
__device__ __forceinline__ void motors_from_rates(const DevLogic &G, float thrust_norm, const V3f &wdes, const V3f &w, float F[4], float cmd[4]) {
#pragma clang fp contract(off)
  const float ex = wdes.x - w.x, ey = wdes.y - w.y, ez = wdes.z - w.z;
  const float a0 = ex / G.tc_xy, a1 = ey / G.tc_xy, a2 = ez / G.tc_z;
  const float Iw0 = ((0.0f + G.I[0] * w.x) + G.I[1] * w.y) + G.I[2] * w.z;
  const float Iw1 = ((0.0f + G.I[3] * w.x) + G.I[4] * w.y) + G.I[5] * w.z;
  const float Iw2 = ((0.0f + G.I[6] * w.x) + G.I[7] * w.y) + G.I[8] * w.z;
  const float Ia0 = ((0.0f + G.I[0] * a0) + G.I[1] * a1) + G.I[2] * a2;
  const float Ia1 = ((0.0f + G.I[3] * a0) + G.I[4] * a1) + G.I[5] * a2;
  const float Ia2 = ((0.0f + G.I[6] * a0) + G.I[7] * a1) + G.I[8] * a2;
  const float tx = Ia0 + (w.y * Iw2 - w.z * Iw1);
  const float ty = Ia1 + (w.z * Iw0 - w.x * Iw2);
  const float tz = Ia2 + (w.x * Iw1 - w.y * Iw0);
  const float totF = thrust_norm * G.mass;
  const float desF = totF > G.max_cmd_total ? G.max_cmd_total : totF;
  F[0] = (-tx / G.d - ty / G.d - tz / G.kt + desF) / 4.0f;
  F[1] = (-tx / G.d + ty / G.d + tz / G.kt + desF) / 4.0f;
  F[2] = (+tx / G.d + ty / G.d - tz / G.kt + desF) / 4.0f;
  F[3] = (+tx / G.d - ty / G.d + tz / G.kt + desF) / 4.0f;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (F[i] < G.min_thrust) F[i] = G.min_thrust;
    else if (F[i] > G.max_thrust) F[i] = G.max_thrust;
    cmd[i] = (F[i] <= 0) ? 0.0f : sqrtf(F[i] / (1.0f * G.kf));
  }
}

__global__ void __launch_bounds__(kBlock) afe_onboard_init_kernel(OnbArgs g, unsigned long long now_us) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= g.n) return;
  const int64_t S = g.stride;
  const OnbType &K = g.types[g.type[v]];
  for (int k = 0; k < kFloats; k++) g.f[k * S + v] = 0.0f;
  g.f[kFAtt * S + v] = 1.0f;
  const float v0 = K.v_crit * 1.2f;                        // consts.lowBatteryThreshold * 1.2f, QuadcopterLogic.cpp:139
  for (int k = 0; k < 4; k++) g.f[(kFBattLp + k) * S + v] = v0;
  for (int k = 0; k < 4; k++) g.f[(kFTempLp + k) * S + v] = 25.0f;
  g.f[kFMainDt * S + v] = K.period;
  g.f[kFCmdDt * S + v] = K.radio_period;
  g.f[kFVolt * S + v] = (float)(1.2 * (double)K.v_crit);   // _battVoltage = 1.2 * threshold (double), narrowed at the call, Quadcopter_T.cpp:72, 163
  for (int k = 0; k < kTimes; k++) g.t[k * S + v] = now_us;
  for (int k = 0; k < kBytes; k++) g.b[k * S + v] = 0;
  g.b[kBState * S + v] = 1;                                // FS_IDLE
  for (int k = 0; k < kWords; k++) g.u[k * S + v] = 0;
  g.mail_arrival[v] = 0; g.mail_type[v] = 0; g.mail_flags[v] = 0;
}

__global__ void __launch_bounds__(kBlock) afe_onboard_tick_kernel(OnbArgs g, unsigned long long T) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t S = g.stride;
  int state = -1, reason = -1, warn = 0;
  if (v < g.n) {
    const int ty = g.type[v];
    const OnbType &K = g.types[ty];
    const DevLogic &G = g.logic[ty];
    float *F = g.f + v;
    unsigned long long *Tm = g.t + v;
    uint8_t *B = g.b + v;
    const int state0 = B[kBState * S], reason0 = B[kBReason * S], warn0 = B[kBWarn * S], running0 = B[kBRunning * S], init0 = B[kBInit * S];
    state = state0; reason = reason0; warn = warn0;
    int flags = B[kBFlags * S];
    unsigned long long tRadio = Tm[kTRadio * S];
    // 0
    const unsigned long long arrival = g.mail_arrival[v];
    const bool fresh = arrival != 0 && arrival - 1 <= T;
    int mtype = 0;
    if (fresh) {
      const unsigned long long ta = arrival - 1;
      mtype = g.mail_type[v];
      flags = g.mail_flags[v];
      tRadio = ta;
      unsigned long long tCmd = Tm[kTCmd * S];
      float lpc = F[kFCmdDt * S];
      monitor_update(K.c_cmd, ta, tCmd, lpc);
      Tm[kTCmd * S] = tCmd; Tm[kTRadio * S] = tRadio;
      F[kFCmdDt * S] = lpc;
      B[kBFlags * S] = (uint8_t)flags;
      g.mail_arrival[v] = 0;
    }
    const float cmd_dt = F[kFCmdDt * S];
    // 1
    float b0 = F[(kFBattLp + 0) * S], b1 = F[(kFBattLp + 1) * S], b2 = F[(kFBattLp + 2) * S], b3 = F[(kFBattLp + 3) * S];
    const float vfilt = lp2_apply(K.batt, F[kFVolt * S], b0, b1, b2, b3);
    F[(kFBattLp + 0) * S] = b0; F[(kFBattLp + 1) * S] = b1; F[(kFBattLp + 2) * S] = b2; F[(kFBattLp + 3) * S] = b3;
    // 2
    const float r0 = g.acc[v], r1 = g.acc[S + v], r2 = g.acc[2 * S + v];
    V3f acc;
    {
      const float raw0 = ((0.0f + G.R[0] * r0) + G.R[1] * r1) + G.R[2] * r2;
      const float raw1 = ((0.0f + G.R[3] * r0) + G.R[4] * r1) + G.R[5] * r2;
      const float raw2 = ((0.0f + G.R[6] * r0) + G.R[7] * r1) + G.R[8] * r2;
      float x0 = F[(kFAccLp + 0) * S], x1 = F[(kFAccLp + 3) * S], y0 = F[(kFAccLp + 6) * S], y1 = F[(kFAccLp + 9) * S];
      acc.x = lp2_apply(K.acc, raw0, x0, x1, y0, y1);
      F[(kFAccLp + 0) * S] = x0; F[(kFAccLp + 3) * S] = x1; F[(kFAccLp + 6) * S] = y0; F[(kFAccLp + 9) * S] = y1;
      x0 = F[(kFAccLp + 1) * S]; x1 = F[(kFAccLp + 4) * S]; y0 = F[(kFAccLp + 7) * S]; y1 = F[(kFAccLp + 10) * S];
      acc.y = lp2_apply(K.acc, raw1, x0, x1, y0, y1);
      F[(kFAccLp + 1) * S] = x0; F[(kFAccLp + 4) * S] = x1; F[(kFAccLp + 7) * S] = y0; F[(kFAccLp + 10) * S] = y1;
      x0 = F[(kFAccLp + 2) * S]; x1 = F[(kFAccLp + 5) * S]; y0 = F[(kFAccLp + 8) * S]; y1 = F[(kFAccLp + 11) * S];
      acc.z = lp2_apply(K.acc, raw2, x0, x1, y0, y1);
      F[(kFAccLp + 2) * S] = x0; F[(kFAccLp + 5) * S] = x1; F[(kFAccLp + 8) * S] = y0; F[(kFAccLp + 11) * S] = y1;
    }
    {
      float t0 = F[(kFTempLp + 0) * S], t1 = F[(kFTempLp + 1) * S], t2 = F[(kFTempLp + 2) * S], t3 = F[(kFTempLp + 3) * S];
      (void)lp2_apply(K.temp, 25.0f, t0, t1, t2, t3);     // GetValue() is _debug[0] in the telemetry
      F[(kFTempLp + 0) * S] = t0; F[(kFTempLp + 1) * S] = t1; F[(kFTempLp + 2) * S] = t2; F[(kFTempLp + 3) * S] = t3;
    }
    V3f gyro;
    gyro.x = g.lpf[9 * S + v]; gyro.y = g.lpf[10 * S + v]; gyro.z = g.lpf[11 * S + v];
    // 3
    g.u[kUCycle * S + v] = g.u[kUCycle * S + v] + 1;
    float main_dt = F[kFMainDt * S];
    {
      unsigned long long tMain = Tm[kTMain * S];
      monitor_update(K.c_main, T, tMain, main_dt);
      Tm[kTMain * S] = tMain;
      F[kFMainDt * S] = main_dt;
    }
    // 4
    Q4f att;
    V3f angVel;
    unsigned long long tReset = Tm[kTReset * S];
    if (!init0) {
      att.w = 1.0f; att.x = 0.0f; att.y = 0.0f; att.z = 0.0f;
      angVel.x = 0.0f; angVel.y = 0.0f; angVel.z = 0.0f;
      V3f axis;
      float angle;
      gravity_axis_angle(att, acc, &axis, &angle);
      att = qf_mul(att, qf_from_axis_angle(axis, angle));
      tReset = T;
      Tm[kTReset * S] = T;
      B[kBInit * S] = 1;
    } else {
      att.w = F[(kFAtt + 0) * S]; att.x = F[(kFAtt + 1) * S]; att.y = F[(kFAtt + 2) * S]; att.z = F[(kFAtt + 3) * S];
      const float dt = (float)(T - Tm[kTEst * S]) * 1e-6f;
      angVel = gyro;
      V3f rv;
      rv.x = gyro.x * dt; rv.y = gyro.y * dt; rv.z = gyro.z * dt;
      att = qf_mul(att, qf_from_rotvec(rv));
      V3f axis;
      float angle;
      gravity_axis_angle(att, acc, &axis, &angle);
      const float corr = (dt / 4.0f) * angle;             // TIME_CONST_ATT_CORR
      att = qf_mul(att, qf_from_axis_angle(axis, corr));
    }
    Tm[kTEst * S] = T;
    F[(kFAtt + 0) * S] = att.w; F[(kFAtt + 1) * S] = att.x; F[(kFAtt + 2) * S] = att.y; F[(kFAtt + 3) * S] = att.z;
    F[(kFAngVel + 0) * S] = angVel.x; F[(kFAngVel + 1) * S] = angVel.y; F[(kFAngVel + 2) * S] = angVel.z;
    // 5
    if (fresh && state != 3 && state != 4) {
      if (mtype == 2) { state = 4; if (!reason) reason = 7; }
      else if (mtype == 3) state = 2;
      else if (mtype == 4) state = 5;
      else if (mtype == 5) state = 6;
      else if (mtype == 6) state = 1;
    }
    // 6
    const float since_radio_s = (float)(T - tRadio) * 1e-6f;
    if (vfilt <= K.v_warn) warn |= 0x01;
    if (fabsf(cmd_dt - K.radio_period) > 0.1f * K.radio_period) warn |= 0x02;
    if (since_radio_s > 3 * K.radio_period) warn |= 0x10;
    if (fabsf(main_dt - K.period) > 0.05f * K.period) warn |= 0x08;
    if ((float)(T - tReset) * 1e-6f < 0.02f) warn |= 0x04;
    // 7
    int unsafe = 0;
    if (running0) {
      const float est_z = 0.0f;                            // no UWB: the estimated position stays 0, this cannot fire
      if (est_z < -2.0f && !(flags & 0x02)) unsafe = 1;
      if (T - Tm[kTUwb * S] > 1500000ull && state == 2) unsafe = 2;   // FS_FULLY_AUTONOMOUS is not built: cannot fire
      V3f e3;
      e3.x = 0.0f; e3.y = 0.0f; e3.z = 1.0f;
      if (mf_rotate(qf_matrix(att), e3).z < 0 && !(flags & 0x02)) unsafe = 3;
      if (T - tRadio > 1500000ull) unsafe = 4;
      if (vfilt <= K.v_crit) unsafe = 5;
    }
    const bool critical = !(state == 0 || state == 1 || state == 3 || state == 4);
    if (unsafe && critical) { state = 3; reason = unsafe; }
    // 8
    float force[4] = {0.0f, 0.0f, 0.0f, 0.0f}, cmd[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool write_cmd = true;
    if (state == 6) {
      V3f wdes;
      wdes.x = g.rates_cmd[S + v]; wdes.y = g.rates_cmd[2 * S + v]; wdes.z = g.rates_cmd[3 * S + v];
      float unused[4];
      motors_from_rates(G, g.rates_cmd[v], wdes, angVel, force, unused);
      cmd[0] = g.motor_cmd[v]; cmd[1] = g.motor_cmd[S + v]; cmd[2] = g.motor_cmd[2 * S + v]; cmd[3] = g.motor_cmd[3 * S + v];
      write_cmd = false;
    } else if (state == 5) {
      V3f des;
      des.x = F[(kFRadio + 0) * S]; des.y = F[(kFRadio + 1) * S]; des.z = F[(kFRadio + 2) * S];
      const float yaw_rate = F[(kFRadio + 3) * S];
      if (!(des.z < -9.81f / 2)) {                         // "Magic number!"
        V3f proper;
        proper.x = des.x + 0.0f; proper.y = des.y + 0.0f; proper.z = des.z + 9.81f;
        const float n = sqrtf(vf_dot(proper, proper));
        V3f dir, e3;
        dir.x = proper.x / n; dir.y = proper.y / n; dir.z = proper.z / n;
        e3.x = 0.0f; e3.y = 0.0f; e3.z = 1.0f;
        const float angle = guarded_acosf(vf_dot(dir, e3));
        const V3f ax = vf_cross(e3, dir);
        const float na = sqrtf(vf_dot(ax, ax));
        Q4f desAtt;
        desAtt.w = 1.0f; desAtt.x = 0.0f; desAtt.y = 0.0f; desAtt.z = 0.0f;
        if (!(na < 1e-6f)) {
          const float k = angle / na;
          V3f rv;
          rv.x = ax.x * k; rv.y = ax.y * k; rv.z = ax.z * k;
          desAtt = qf_from_rotvec(rv);
        }
        float y, p, r;
        qf_to_euler_ypr(att, &y, &p, &r);
        const Q4f noYaw = qf_from_euler_ypr(0.0f, p, r);
        V3f wdes = desired_angular_velocity(desAtt, noYaw, K.tc_xy, K.tc_z);
        wdes.z = yaw_rate;
        motors_from_rates(G, n, wdes, angVel, force, cmd);
      }
    }
    if (write_cmd) { g.motor_cmd[v] = cmd[0]; g.motor_cmd[S + v] = cmd[1]; g.motor_cmd[2 * S + v] = cmd[2]; g.motor_cmd[3 * S + v] = cmd[3]; }
    F[(kFForces + 0) * S] = force[0]; F[(kFForces + 1) * S] = force[1]; F[(kFForces + 2) * S] = force[2]; F[(kFForces + 3) * S] = force[3];
    const int running = (cmd[0] > 0 || cmd[1] > 0 || cmd[2] > 0 || cmd[3] > 0) ? 1 : 0;
    // the words that rarely change
    if (state != state0) B[kBState * S] = (uint8_t)state;
    if (reason != reason0) B[kBReason * S] = (uint8_t)reason;
    if (warn != warn0) B[kBWarn * S] = (uint8_t)warn;
    if (running != running0) B[kBRunning * S] = (uint8_t)running;
  }
  // 9
  if (g.counters) {
    const bool lead = (threadIdx.x & 63) == 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const unsigned long long mask = __ballot(k < 7 ? state == k : k < 15 ? reason == k - 7 : warn != 0);
      if (lead && mask) atomicAdd(g.counters + k, (unsigned long long)__popcll(mask));
    }
  }
}

// GetTelemetryDataPackets, QuadcopterLogic.cpp:621-679: out [count][2][30]
__global__ void __launch_bounds__(kBlock) afe_onboard_telemetry_kernel(OnbArgs g, int64_t first, int64_t count, uint8_t *out) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  const int64_t v = first + i, S = g.stride;
  const float *F = g.f + v;
  uint8_t *p1 = out + i * 60, *p2 = p1 + 30;
  const uint32_t counter = g.u[kUPacket * S + v];
  auto put = [](uint8_t *p, int slot, uint16_t code) { p[2 + 2 * slot] = (uint8_t)(code & 0xff); p[3 + 2 * slot] = (uint8_t)(code >> 8); };
  p1[0] = 0; p1[1] = (uint8_t)(counter % 256);
  put(p1, 0, telemetry_code(F[(kFAccLp + 9) * S], -30.0f, 30.0f));
  put(p1, 1, telemetry_code(F[(kFAccLp + 10) * S], -30.0f, 30.0f));
  put(p1, 2, telemetry_code(F[(kFAccLp + 11) * S], -30.0f, 30.0f));
  put(p1, 3, telemetry_code(g.lpf[9 * S + v], -35.0f, 35.0f));
  put(p1, 4, telemetry_code(g.lpf[10 * S + v], -35.0f, 35.0f));
  put(p1, 5, telemetry_code(g.lpf[11 * S + v], -35.0f, 35.0f));
  put(p1, 6, telemetry_code(F[(kFForces + 0) * S], 0.0f, 10.0f));
  put(p1, 7, telemetry_code(F[(kFForces + 1) * S], 0.0f, 10.0f));
  put(p1, 8, telemetry_code(F[(kFForces + 2) * S], 0.0f, 10.0f));
  put(p1, 9, telemetry_code(F[(kFForces + 3) * S], 0.0f, 10.0f));
  put(p1, 10, telemetry_code(0.0f, -30.0f, 30.0f));     // the estimated position: 0 without UWB
  put(p1, 11, telemetry_code(0.0f, -30.0f, 30.0f));
  put(p1, 12, telemetry_code(0.0f, -30.0f, 30.0f));
  put(p1, 13, telemetry_code(F[kFVolt * S], 0.0f, 15.0f));   // voltageRaw
  p2[0] = 1; p2[1] = (uint8_t)(counter % 256);
  put(p2, 0, telemetry_code(0.0f, -30.0f, 30.0f));      // the estimated velocity
  put(p2, 1, telemetry_code(0.0f, -30.0f, 30.0f));
  put(p2, 2, telemetry_code(0.0f, -30.0f, 30.0f));
  const float w = F[(kFAtt + 0) * S];                    // ToVectorPartOfQuaternion: the first component made positive
  const float qx = F[(kFAtt + 1) * S], qy = F[(kFAtt + 2) * S], qz = F[(kFAtt + 3) * S];
  put(p2, 3, telemetry_code(w > 0 ? qx : -qx, -1.0f, 1.0f));
  put(p2, 4, telemetry_code(w > 0 ? qy : -qy, -1.0f, 1.0f));
  put(p2, 5, telemetry_code(w > 0 ? qz : -qz, -1.0f, 1.0f));
  put(p2, 6, telemetry_code(F[(kFTempLp + 3) * S], -100.0f, 100.0f));   // _debug[0]
  put(p2, 7, telemetry_code(0.0f, -100.0f, 100.0f));
  put(p2, 8, telemetry_code(0.0f, -100.0f, 100.0f));
  put(p2, 9, telemetry_code(0.0f, -100.0f, 100.0f));
  put(p2, 10, telemetry_code(0.0f, -100.0f, 100.0f));
  put(p2, 11, telemetry_code(0.0f, -100.0f, 100.0f));
  p2[26] = g.b[kBReason * S + v]; p2[27] = 0;            // memcpy of one byte each; the other byte is 0 here
  p2[28] = g.b[kBWarn * S + v]; p2[29] = 0;
  g.u[kUPacket * S + v] = counter + 1;
  g.b[kBWarn * S + v] = 0;
}

__global__ void __launch_bounds__(kBlock) afe_onboard_stamp_kernel(afe::RadioMailbox m, int64_t first, int64_t count, unsigned long long now_us, int type,
                                                                   const uint8_t *dev_types) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  const int64_t v = first + i;
  if (dev_types) {
    const uint8_t t = dev_types[v];
    if (t == 0) return;
    m.type[v] = t; m.flags[v] = 0;
  } else if (type >= 0) {
    m.type[v] = (uint8_t)type; m.flags[v] = 0;
  }
  m.arrival[v] = now_us + 1;
}

__global__ void __launch_bounds__(kBlock) afe_onboard_math_kernel(int op, int64_t n, const float *x, float *y) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  float s, c;
  fm_sincosf(x[i], &s, &c);
  y[i] = op == 0 ? s : op == 1 ? c : op == 2 ? fm_acosf(x[i]) : op == 3 ? fm_asinf(x[i]) : fm_atan2f(x[i], x[n + i]);
}

size_t up256(size_t x) { return (x + 255) & ~size_t(255); }
dim3 grid_for(int64_t n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }
bool launched() { return hipGetLastError() == hipSuccess; }

bool put_rows(void *dev, size_t esz, int comps, int64_t stride, int64_t first, int64_t count, const void *host) {
  return hipMemcpy2D((char *)dev + (size_t)first * esz, (size_t)stride * esz, host, (size_t)count * esz, (size_t)count * esz, (size_t)comps,
                     hipMemcpyHostToDevice) == hipSuccess;
}
bool get_rows(const void *dev, size_t esz, int comps, int64_t stride, int64_t first, int64_t count, void *host) {
  return hipMemcpy2D(host, (size_t)count * esz, (const char *)dev + (size_t)first * esz, (size_t)stride * esz, (size_t)count * esz, (size_t)comps,
                     hipMemcpyDeviceToHost) == hipSuccess;
}

// LowPassFilterSecondOrder<float, ...>::Initialise, LowPassFilterSecondOrder.hpp:22-49 (as afe_params.cpp expand_logic)
Lp2 lowpass_coefficients(float dt, float wc) {
  const float sqrt2 = float(std::sqrt(2.0));
  Lp2 k;
  k.a1 = (dt * dt * wc * wc - 2 * sqrt2 * dt * wc + 4) / (dt * dt * wc * wc + 2 * sqrt2 * dt * wc + 4);
  k.a2 = 2 * (dt * dt * wc * wc - 4) / (dt * dt * wc * wc + 2 * sqrt2 * dt * wc + 4);
  k.b0 = dt * dt * wc * wc / (dt * dt * wc * wc + 2 * sqrt2 * dt * wc + 4);
  k.b1 = dt * dt * wc * wc / (dt * dt * wc * wc + 2 * sqrt2 * dt * wc + 4);
  k.b2 = 2 * dt * dt * wc * wc / (dt * dt * wc * wc + 2 * sqrt2 * dt * wc + 4);
  return k;
}
// LowPassFilterFirstOrder<float, float>::Initialise, LowPassFilterFirstOrder.hpp:31: exp of a float product -- in C++ the float
// overload, expf (for the products in use, 0.002 x 50 and 0.02 x 1, the double exp narrowed is the same float)
float lowpass1_coefficient(float period, float wc) { return expf(-period * wc); }

bool positive(float x) { return std::isfinite(x) && x > 0; }

}  // namespace

struct afe_onboard {
  afe_engine *engine = nullptr;     // borrowed
  int device = 0;
  int64_t n = 0, stride = 0;
  int n_types = 0;
  float period = 0;                 // the logic period the type table was built for
  std::vector<afe_onboard_config> cfg;
  uint64_t n_ticks = 0, last_tick = 0;
  afe::DevBuf arena;
  OnbArgs args;                     // the computer's part of the kernel arguments
};

namespace {

struct Entry {
  hipStream_t stream;
  OnbArgs g;
  uint64_t n_ticks, now_us;
  float period;
};

std::vector<OnbType> type_table(const afe_onboard *o, float period) {
  std::vector<OnbType> t((size_t)o->n_types);
  for (int k = 0; k < o->n_types; k++) {
    const afe_onboard_config &c = o->cfg[(size_t)k];
    OnbType &x = t[(size_t)k];
    x.acc = lowpass_coefficients(period, c.accel_lowpass_cutoff);
    x.batt = lowpass_coefficients(period, c.batt_lowpass_cutoff);
    x.temp = lowpass_coefficients(period, c.temp_lowpass_cutoff);
    x.c_main = lowpass1_coefficient(period, c.main_loop_monitor_cutoff);
    x.c_cmd = lowpass1_coefficient(c.radio_cmd_period, c.cmd_rate_monitor_cutoff);
    x.tc_xy = c.att_time_const_xy; x.tc_z = c.att_time_const_z;
    x.v_crit = c.low_battery_threshold; x.v_warn = 1.05f * c.low_battery_threshold;
    x.period = period; x.radio_period = c.radio_cmd_period;
  }
  return t;
}

// through the engine's gate; the engine's slabs into the arguments
int enter(afe_onboard *o, Entry *en) {
  afe::EngineAccess acc;
  int rc = afe::engine_enter(o->engine, &acc);
  if (rc != AFE_OK) return rc;
  const afe_device_view &view = acc.view;
  if (view.n_vehicles != o->n || view.stride != o->stride || acc.device != o->device) return AFE_ERR_INVALID_ARG;
  en->stream = acc.stream;
  en->g = o->args;
  rc = afe::engine_logic_filter(o->engine, &en->g.lpf, &en->g.logic, &en->period, &en->n_ticks);
  if (rc != AFE_OK) return rc;
  float *rates = nullptr;
  uint8_t *have = nullptr;
  rc = afe::engine_rates_slabs(o->engine, &rates, &have);
  if (rc != AFE_OK) return rc;
  en->g.rates_cmd = rates;
  en->g.acc = view.acc; en->g.motor_cmd = view.motor_cmd; en->g.type = view.type_index;
  return afe_time_us(o->engine, &en->now_us);
}

int enter_rows(afe_onboard *o, int64_t first, int64_t count) {
  if (!o || first < 0 || count < 0) return AFE_ERR_INVALID_ARG;
  if (first > o->n || count > o->n - first) return AFE_ERR_OUT_OF_RANGE;   // (no sum: it can wrap)
  return AFE_OK;
}
// through the gate, then the stream drained: the copies that follow are synchronous
int drain(afe_onboard *o, Entry *en) {
  const int rc = enter(o, en);
  if (rc != AFE_OK) return rc;
  return hipStreamSynchronize(en->stream) == hipSuccess ? AFE_OK : AFE_ERR_HIP;
}

}  // namespace

extern "C" int afe_onboard_default_config(int quadcopter_type, afe_onboard_config *cfg) {
  if (!cfg) return AFE_ERR_INVALID_ARG;
  afe_follower_config f;
  if (afe_follower_default_config(quadcopter_type, &f) != AFE_OK) return AFE_ERR_INVALID_ARG;   // QuadcopterConstants, as the follower derives them
  afe_onboard_config c;
  std::memset(&c, 0, sizeof(c));
  if (afe_low_battery_threshold_from_type(quadcopter_type, &c.low_battery_threshold) != AFE_OK) return AFE_ERR_INVALID_ARG;
  c.struct_bytes = sizeof(c);
  c.accel_lowpass_cutoff = 100.0f;                        // QuadcopterLogic.cpp:102
  c.batt_lowpass_cutoff = 0.5f * float(2 * M_PI);         // :104
  c.temp_lowpass_cutoff = 0.5f * float(2 * M_PI);         // :105
  c.main_loop_monitor_cutoff = 50.0f;                     // :15
  c.cmd_rate_monitor_cutoff = 1.0f;                       // :14
  c.att_time_const_xy = f.att_time_const_xy; c.att_time_const_z = f.att_time_const_z;
  c.radio_cmd_period = 0.02f;                             // :10
  *cfg = c;
  return AFE_OK;
}

extern "C" int afe_onboard_create(afe_engine *e, const afe_onboard_config *cfg_table, int n_types, afe_onboard **out) {
  if (!e || !cfg_table || !out || n_types <= 0 || n_types > 256) return AFE_ERR_INVALID_ARG;
  for (int k = 0; k < n_types; k++) {
    const afe_onboard_config &c = cfg_table[k];
    if (c.struct_bytes < sizeof(afe_onboard_config)) return AFE_ERR_INVALID_ARG;
    if (!positive(c.accel_lowpass_cutoff) || !positive(c.batt_lowpass_cutoff) || !positive(c.temp_lowpass_cutoff) ||
        !positive(c.main_loop_monitor_cutoff) || !positive(c.cmd_rate_monitor_cutoff) || !positive(c.att_time_const_xy) ||
        !positive(c.att_time_const_z) || !std::isfinite(c.low_battery_threshold) || !positive(c.radio_cmd_period))
      return AFE_ERR_INVALID_ARG;
  }
  afe::EngineAccess acc;
  int rc = afe::engine_enter(e, &acc);
  if (rc != AFE_OK) return rc;
  const float *lpf = nullptr;
  const DevLogic *logic = nullptr;
  float period = 0;
  uint64_t ticks = 0, now_us = 0;
  rc = afe::engine_logic_filter(e, &lpf, &logic, &period, &ticks);
  if (rc != AFE_OK) return rc;
  rc = afe::engine_device_resident(e);
  if (rc != AFE_OK) return rc;
  if (n_types != afe::engine_type_records(e)) return AFE_ERR_INVALID_ARG;   // one config per type record
  rc = afe_time_us(e, &now_us);
  if (rc != AFE_OK) return rc;
  afe_onboard *o = new afe_onboard();
  o->engine = e; o->device = acc.device; o->n = acc.view.n_vehicles; o->stride = acc.view.stride;
  o->n_types = n_types; o->period = period; o->last_tick = ticks;
  o->cfg.assign(cfg_table, cfg_table + n_types);
  const size_t S = (size_t)o->stride;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t p = off; off += up256(bytes); return p; };
  const size_t o_f = take(S * 4 * kFloats), o_t = take(S * 8 * kTimes), o_b = take(S * kBytes), o_u = take(S * 4 * kWords), o_ma = take(S * 8),
               o_mt = take(S), o_mf = take(S), o_types = take(256 * sizeof(OnbType)), o_cnt = take(128);
  if (!o->arena.alloc(off)) { (void)hipGetLastError(); delete o; return AFE_ERR_HIP; }
  unsigned char *A = o->arena.as<unsigned char>();
  std::memset(&o->args, 0, sizeof(o->args));
  OnbArgs &g = o->args;
  g.n = o->n; g.stride = o->stride;
  g.f = (float *)(A + o_f); g.t = (unsigned long long *)(A + o_t); g.b = A + o_b; g.u = (uint32_t *)(A + o_u);
  g.mail_arrival = (unsigned long long *)(A + o_ma); g.mail_type = A + o_mt; g.mail_flags = A + o_mf;
  g.types = (const OnbType *)(A + o_types); g.counters = (unsigned long long *)(A + o_cnt);
  g.type = acc.view.type_index;
  const std::vector<OnbType> table = type_table(o, period);
  const hipStream_t stream = acc.stream;
  rc = hipMemsetAsync(A, 0, off, stream) == hipSuccess ? AFE_OK : AFE_ERR_HIP;      // (the padding beyond n included)
  if (rc == AFE_OK && hipMemcpyAsync(A + o_types, table.data(), table.size() * sizeof(OnbType), hipMemcpyHostToDevice, stream) != hipSuccess) rc = AFE_ERR_HIP;
  if (rc == AFE_OK && hipStreamSynchronize(stream) != hipSuccess) rc = AFE_ERR_HIP;  // (the table is a local)
  if (rc == AFE_OK && o->n > kBlocksPerLaunch * kBlock) rc = AFE_ERR_OUT_OF_RANGE;
  if (rc == AFE_OK && o->n > 0) {
    hipLaunchKernelGGL(afe_onboard_init_kernel, grid_for(o->n), dim3(kBlock), 0, stream, g, (unsigned long long)now_us);
    if (!launched()) rc = AFE_ERR_HIP;
  }
  if (rc == AFE_OK && hipStreamSynchronize(stream) != hipSuccess) rc = AFE_ERR_HIP;
  if (rc == AFE_OK) {
    const afe::RadioMailbox mail = {g.mail_arrival, g.mail_type, g.mail_flags};
    rc = afe::engine_set_mailbox(e, &mail);
  }
  if (rc != AFE_OK) { (void)hipGetLastError(); delete o; return rc; }
  *out = o;
  return AFE_OK;
}

extern "C" int afe_onboard_destroy(afe_onboard *o) {
  if (!o) return AFE_ERR_INVALID_ARG;
  (void)hipSetDevice(o->device);
  (void)hipDeviceSynchronize();
  (void)afe::engine_set_mailbox(o->engine, nullptr);
  delete o;
  return AFE_OK;
}

extern "C" int afe_onboard_info(const afe_onboard *o, int64_t *n_vehicles, uint64_t *n_ticks, uint64_t *last_tick) {
  if (!o) return AFE_ERR_INVALID_ARG;
  if (n_vehicles) *n_vehicles = o->n;
  if (n_ticks) *n_ticks = o->n_ticks;
  if (last_tick) *last_tick = o->n_ticks ? o->last_tick : 0;
  return AFE_OK;
}

extern "C" int afe_onboard_set_battery(afe_onboard *o, int64_t first, int64_t count, const float *volts) {
  const int arc = enter_rows(o, first, count);
  if (arc != AFE_OK) return arc;
  if (!volts) return AFE_ERR_INVALID_ARG;
  if (count == 0) return AFE_OK;
  Entry en;
  const int rc = drain(o, &en);
  if (rc != AFE_OK) return rc;
  return put_rows(o->args.f + (size_t)kFVolt * (size_t)o->stride, 4, 1, o->stride, first, count, volts) ? AFE_OK : AFE_ERR_HIP;
}

extern "C" int afe_onboard_radio(afe_onboard *o, int64_t first, int64_t count, const uint8_t *raw_packets) {
  const int arc = enter_rows(o, first, count);
  if (arc != AFE_OK) return arc;
  if (!raw_packets) return AFE_ERR_INVALID_ARG;
  if (count == 0) return AFE_OK;
  // nothing is applied unless every packet can be: types 2, 5, 6 as afe_set_commands_from_radio, type 4 here
  std::vector<uint8_t> packets(raw_packets, raw_packets + (size_t)count * AFE_RADIO_PACKET_SIZE), types((size_t)count), flags((size_t)count);
  std::vector<afe_radio_message> msg((size_t)count);
  bool any_acc = false;
  for (int64_t k = 0; k < count; k++) {
    afe_radio_message &m = msg[(size_t)k];
    afe_radio_decode(raw_packets + k * AFE_RADIO_PACKET_SIZE, &m);
    types[(size_t)k] = m.type; flags[(size_t)k] = m.flags;
    if (m.type == 4) {
      any_acc = true;                                         // for the engine: the rates command is cleared, as idle does
      if (afe_radio_create_simple_command(6, m.flags, packets.data() + k * AFE_RADIO_PACKET_SIZE) != AFE_OK) return AFE_ERR_INVALID_ARG;
    } else if (m.type != 2 && m.type != 5 && m.type != 6) return AFE_ERR_INVALID_ARG;
  }
  int rc = afe_set_commands_from_radio(o->engine, first, count, packets.data());   // (stamps the mailbox: arrival, and idle for type 4)
  if (rc != AFE_OK) return rc;
  if (!any_acc) return AFE_OK;
  Entry en;
  rc = drain(o, &en);
  if (rc != AFE_OK) return rc;
  const OnbArgs &g = o->args;
  const int64_t S = o->stride;
  std::vector<float> payload((size_t)(4 * count));
  if (!get_rows(g.f + (size_t)kFRadio * (size_t)S, 4, 4, S, first, count, payload.data())) return AFE_ERR_HIP;
  for (int64_t k = 0; k < count; k++)
    if (types[(size_t)k] == 4)
      for (int c = 0; c < 4; c++) payload[(size_t)(c * count + k)] = msg[(size_t)k].floats[c];
  if (!put_rows(g.f + (size_t)kFRadio * (size_t)S, 4, 4, S, first, count, payload.data()) ||
      !put_rows(g.mail_type, 1, 1, S, first, count, types.data()))
    return AFE_ERR_HIP;
  return AFE_OK;
}

extern "C" int afe_onboard_tick(afe_onboard *o, int64_t *counts16) {
  if (!o) return AFE_ERR_INVALID_ARG;
  Entry en;
  int rc = enter(o, &en);
  if (rc != AFE_OK) return rc;
  uint64_t tick_us = 0, steps_after = 0;
  rc = afe::engine_tick_clock(o->engine, &tick_us, &steps_after);
  if (rc != AFE_OK) return rc;
  // every tick exactly once, and behind the step that fired it: the command the step kernel wrote is this tick's
  if (en.n_ticks != o->last_tick + 1 || steps_after != 0) return AFE_ERR_NOT_CONFIGURED;
  OnbArgs &g = en.g;
  if (en.period != o->period) {                               // afe_set_logic_period since: the filters' sampling period follows
    const std::vector<OnbType> table = type_table(o, en.period);
    if (hipMemcpyAsync((void *)g.types, table.data(), table.size() * sizeof(OnbType), hipMemcpyHostToDevice, en.stream) != hipSuccess ||
        hipStreamSynchronize(en.stream) != hipSuccess)
      return AFE_ERR_HIP;
    o->period = en.period;
  }
  if (counts16) {
    if (hipMemsetAsync(g.counters, 0, 128, en.stream) != hipSuccess) return AFE_ERR_HIP;
  } else g.counters = nullptr;
  if (o->n > 0) {
    hipLaunchKernelGGL(afe_onboard_tick_kernel, grid_for(g.n), dim3(kBlock), 0, en.stream, g, (unsigned long long)tick_us);
    if (!launched()) return AFE_ERR_HIP;
  }
  o->last_tick = en.n_ticks;
  o->n_ticks++;
  if (counts16) {
    unsigned long long c[16];
    if (hipMemcpyAsync(c, g.counters, 128, hipMemcpyDeviceToHost, en.stream) != hipSuccess || hipStreamSynchronize(en.stream) != hipSuccess)
      return AFE_ERR_HIP;
    for (int k = 0; k < 16; k++) counts16[k] = (int64_t)c[k];
  }
  return AFE_OK;
}

extern "C" int afe_onboard_get(afe_onboard *o, int64_t first, int64_t count, const afe_onboard_fields *f) {
  const int arc = enter_rows(o, first, count);
  if (arc != AFE_OK) return arc;
  if (!f || f->struct_bytes < sizeof(afe_onboard_fields)) return AFE_ERR_INVALID_ARG;
  if (!f->flight_state && !f->panic_reason && !f->warnings && !f->est_att4 && !f->est_ang_vel3 && !f->acc_filtered3 && !f->batt_filtered &&
      !f->main_loop_dt && !f->cmd_dt && !f->motor_forces4 && !f->cycle_counter && !f->last_radio_us && !f->motors_running)
    return AFE_ERR_INVALID_ARG;
  if (count == 0) return AFE_OK;
  Entry en;
  const int rc = drain(o, &en);
  if (rc != AFE_OK) return rc;
  const OnbArgs &g = o->args;
  const int64_t S = o->stride;
  auto byte_row = [&](int row, uint8_t *host) { return !host || get_rows(g.b + (size_t)row * (size_t)S, 1, 1, S, first, count, host); };
  auto float_rows = [&](int row, int comps, float *host) { return !host || get_rows(g.f + (size_t)row * (size_t)S, 4, comps, S, first, count, host); };
  if (!byte_row(kBState, f->flight_state) || !byte_row(kBReason, f->panic_reason) || !byte_row(kBWarn, f->warnings) ||
      !byte_row(kBRunning, f->motors_running) || !float_rows(kFAtt, 4, f->est_att4) || !float_rows(kFAngVel, 3, f->est_ang_vel3) ||
      !float_rows(kFAccLp + 9, 3, f->acc_filtered3) || !float_rows(kFBattLp + 3, 1, f->batt_filtered) || !float_rows(kFMainDt, 1, f->main_loop_dt) ||
      !float_rows(kFCmdDt, 1, f->cmd_dt) || !float_rows(kFForces, 4, f->motor_forces4) ||
      (f->cycle_counter && !get_rows(g.u + (size_t)kUCycle * (size_t)S, 4, 1, S, first, count, f->cycle_counter)) ||
      (f->last_radio_us && !get_rows(g.t + (size_t)kTRadio * (size_t)S, 8, 1, S, first, count, f->last_radio_us)))
    return AFE_ERR_HIP;
  return AFE_OK;
}

extern "C" int afe_onboard_set_state(afe_onboard *o, int64_t first, int64_t count, const afe_onboard_state *st) {
  const int arc = enter_rows(o, first, count);
  if (arc != AFE_OK) return arc;
  if (!st || st->struct_bytes < sizeof(afe_onboard_state)) return AFE_ERR_INVALID_ARG;
  if (!st->est_att4 && !st->est_ang_vel3 && !st->imu_initialized && !st->lowpass20 && !st->flight_state && !st->motors_running && !st->last_radio_us)
    return AFE_ERR_INVALID_ARG;
  if (st->flight_state)
    for (int64_t k = 0; k < count; k++)
      if (st->flight_state[k] >= AFE_FS_COUNT || st->flight_state[k] == AFE_FS_FULLY_AUTONOMOUS) return AFE_ERR_INVALID_ARG;   // (not built)
  if (count == 0) return AFE_OK;
  Entry en;
  const int rc = drain(o, &en);
  if (rc != AFE_OK) return rc;
  const OnbArgs &g = o->args;
  const int64_t S = o->stride;
  auto byte_row = [&](int row, const uint8_t *host) { return !host || put_rows(g.b + (size_t)row * (size_t)S, 1, 1, S, first, count, host); };
  auto float_rows = [&](int row, int comps, const float *host) { return !host || put_rows(g.f + (size_t)row * (size_t)S, 4, comps, S, first, count, host); };
  if (!float_rows(kFAtt, 4, st->est_att4) || !float_rows(kFAngVel, 3, st->est_ang_vel3) || !float_rows(kFAccLp, 20, st->lowpass20) ||
      !byte_row(kBInit, st->imu_initialized) || !byte_row(kBState, st->flight_state) || !byte_row(kBRunning, st->motors_running) ||
      (st->last_radio_us && !put_rows(g.t + (size_t)kTRadio * (size_t)S, 8, 1, S, first, count, st->last_radio_us)))
    return AFE_ERR_HIP;
  return AFE_OK;
}

extern "C" int afe_onboard_telemetry(afe_onboard *o, int64_t first, int64_t count, uint8_t *packets) {
  const int arc = enter_rows(o, first, count);
  if (arc != AFE_OK) return arc;
  if (!packets) return AFE_ERR_INVALID_ARG;
  if (count == 0) return AFE_OK;
  Entry en;
  const int rc = enter(o, &en);
  if (rc != AFE_OK) return rc;
  const size_t bytes = (size_t)count * 2 * AFE_TELEMETRY_PACKET_SIZE;
  afe::DevBuf out;
  if (!out.alloc(bytes)) { (void)hipGetLastError(); return AFE_ERR_HIP; }
  hipLaunchKernelGGL(afe_onboard_telemetry_kernel, grid_for(count), dim3(kBlock), 0, en.stream, en.g, first, count, out.as<uint8_t>());
  if (!launched()) return AFE_ERR_HIP;
  if (hipMemcpyAsync(packets, out.get(), bytes, hipMemcpyDeviceToHost, en.stream) != hipSuccess || hipStreamSynchronize(en.stream) != hipSuccess)
    return AFE_ERR_HIP;
  return AFE_OK;
}

extern "C" int afe_onboard_selftest_math(int device, int op, int64_t n, const float *x, float *y) {
  if (!x || !y || op < 0 || op > 4 || n < 0) return AFE_ERR_INVALID_ARG;
  if (n == 0) return AFE_OK;
  if (n > kBlocksPerLaunch * kBlock) return AFE_ERR_OUT_OF_RANGE;
  const int prc = afe::pick_gfx950(device, &device);
  if (prc != AFE_OK) return prc;
  const size_t in_bytes = (size_t)n * 4 * (op == 4 ? 2 : 1), out_bytes = (size_t)n * 4;
  afe::DevBuf dx, dy;
  if (!dx.upload(x, in_bytes) || !dy.alloc(out_bytes)) { (void)hipGetLastError(); return AFE_ERR_HIP; }
  hipLaunchKernelGGL(afe_onboard_math_kernel, grid_for(n), dim3(kBlock), 0, nullptr, op, n, dx.as<float>(), dy.as<float>());
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return AFE_ERR_HIP;
  return dy.download(y, out_bytes) ? AFE_OK : AFE_ERR_HIP;
}

// ---- for whoever delivers a command (afe_consumer.h, THE RADIO MAILBOX) ------------------------------------------------------
int afe::onboard_stamp(void *stream, const RadioMailbox &m, int64_t first, int64_t count, uint64_t now_us, int type, const uint8_t *dev_types) {
  if (!m.arrival || count <= 0) return AFE_OK;
  if (count > kBlocksPerLaunch * kBlock) return AFE_ERR_OUT_OF_RANGE;
  hipLaunchKernelGGL(afe_onboard_stamp_kernel, grid_for(count), dim3(kBlock), 0, (hipStream_t)stream, m, first, count, (unsigned long long)now_us, type, dev_types);
  return launched() ? AFE_OK : AFE_ERR_HIP;
}
