// oracle/ref_onboard_probe.cpp -- TEST INFRASTRUCTURE.
// The REFERENCE's own onboard flight computer, compiled from where it lies:
//   Components/Components/Logic/QuadcopterLogic.cpp     (named on the compiler's command line, oracle/Makefile)
//   Components/Components/Logic/KalmanFilter6DOF.cpp    (named there too)
//   Components/Components/Simulation/Quadcopter_T.cpp   (#included below: its member templates must be visible where they
//                                                        are instantiated; it ends in the explicit instantiation for
//                                                        Onboard::QuadcopterLogic, which now links)
//   Components/Components/Simulation/Motor.cpp          (named on the command line)
// driven by Common/Common/Time/ManualTimer.hpp.  -I oracle/eigen_trap and no other Eigen header: storage as in
// oracle/eigen_store, plus the arithmetic members KalmanFilter6DOF.cpp names, each defined as "print which operation,
// abort()".  The path pinned here -- QuadcopterLogic::Run without a UWB range, i.e. KalmanFilter6DOF::Reset, the alignment
// and the complementary branch (KalmanFilter6DOF.cpp:33-147) -- uses element access alone; a path that reached the 9 x 9
// products would end this program with the operation's name on stderr, and the generator requires exit status 0.
// Compiled WITHOUT -fno-math-errno: the reference's `errno = 0; acosf(c); if (errno)` is on the pinned path.
//
// This file's own text is the driver: it reads a call list, makes the reference's calls with the numbers given and writes
// what the reference's members hold afterwards.  Nothing of the logic is restated here.  Private members are read, and
// the ones the script places (tests/onboard_flight.py, afe_onboard_set_state's fields) are written: `#define private
// public`, as in ref_rigid_body_probe.cpp.  The one Eigen operation of the vehicle mode, inertiaMatrix.inverse() at
// Quadcopter_T.cpp:20, is injected as in ref_rigid_body_probe.cpp: the explicit specialisation hands back the request's
// nine numbers.
//
// usage: onboard_probe < request > answer      (binary, little endian; tests/onboard_probe.py)
//   request: int32 magic "ROB1", int32 mode, int32 n, then
//   mode 0, logic: per vehicle  float period, int32 n_ops, then n_ops calls: int32 code and its payload (floats travel as
//     their bit patterns and reach the reference's arguments unchanged)
//       1 CLOCK    uint64 now_us                    ManualTimer::ResetMicroseconds
//       2 INIT     int32 type, id                   new QuadcopterLogic(&clock, period); Initialise(type, id)
//       3 BATTERY  float voltage, current           SetBatteryMeasurement
//       4 GYRO     float x, y, z                    SetIMUMeasurementRateGyro
//       5 ACC      float x, y, z                    SetIMUMeasurementAccelerometer
//       6 TEMP     float t                          SetIMUMeasurementTemperature
//       7 RADIO    int32 type, flags, float f[4]    SetRadioMessage({type, flags, floats = f[0..3], 0 ...})
//       8 RUN                                       Run()                      -> one RUN record
//       9 TELEMETRY                                 GetTelemetryDataPackets    -> 2 x 30 bytes
//      10 PLACE    int32 mask, float att[4], ang_vel[3], int32 imu_initialized, float lowpass[20], int32 state,
//                  uint64 radio_reset_us            bit 0 _kf._att, 1 _kf._angVel, 2 _kf._IMUInitialized, 3 the histories
//                                                   of the accelerometer (xm0, xm1, ym0, ym1: 3 each), battery and
//                                                   temperature (4 each) low-passes, 4 _state, 5 the radio timer's reset time
//      11 MOUNT    float yaw, pitch, roll           _IMU_*, and _R rebuilt by the call Initialise makes (:118-119)
//     RUN record: int32 state, first panic reason, warnings, GetAreMotorsRunning(), cycle counter; uint64 the radio timer's
//       reset time; float attitude[4], angular velocity[3], position[3], velocity[3], accelerometer low-pass[3], gyro
//       low-pass[3], temperature low-pass, filtered battery voltage, lpDt of the main-loop and of the command-rate monitor,
//       motor speeds[4], motor forces[4]
//   mode 1, vehicle: per vehicle  int32 type, dt_us, n_steps; double mass, inertia[9], inverse[9], arm, com[3], min_speed,
//     max_speed, k_thrust, k_torque, tau, J, drag[3], period (Quadcopter_T's constructor arguments).  Noise standard
//     deviations are set to 0.  Per step AdvanceMicroSeconds(dt_us); Run(); after a step in which the logic ran, one line:
//     uint64 master clock; int32 step, cycle counter, battery count, gyro count, accelerometer count, temperature count;
//     float _battMeas.voltageRaw, _imuTemperature.rawMeas, _battMeas.voltageFiltered
//   answer: int32 magic, mode, n, then the records above in call order (mode 1: int32 n_lines in front of each vehicle's)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cassert>
#include <stdint.h>
#include <vector>
#include <memory>
#include <iostream>
#include <random>
#include <fstream>
#include <Eigen/Dense>

static double g_inverse[9];
namespace Eigen {
template <>
Matrix<double, 3, 3> Matrix<double, 3, 3>::inverse() const {
  Matrix<double, 3, 3> m;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) m(i, j) = g_inverse[3 * i + j];
  return m;
}
}  // namespace Eigen

#define private public
#define protected public
#include "Components/Logic/QuadcopterLogic.hpp"
#include "Components/Simulation/Quadcopter_T.hpp"
#undef protected
#undef private
#include "Common/Time/ManualTimer.hpp"
#include "Components/Simulation/Quadcopter_T.cpp"

static const int32_t MAGIC = 0x31424f52;   // "ROB1"
enum { CLOCK = 1, INIT, BATTERY, GYRO, ACC, TEMP, RADIO, RUN, TELEMETRY, PLACE, MOUNT };

template <typename T>
static bool rd(T *v, size_t n) { return fread(v, sizeof(T), n, stdin) == n; }
template <typename T>
static void wr(const T *v, size_t n) { fwrite(v, sizeof(T), n, stdout); }

static void write_run(Onboard::QuadcopterLogic &L) {
  const int32_t ih[5] = {(int32_t) L._state, (int32_t) L._firstPanicReason, (int32_t) L._telWarnings,
                         (int32_t) L.GetAreMotorsRunning(), (int32_t) L._cycleCounter};
  const uint64_t reset = L._timeSinceLastRadioMessage._lastResetTime_usec;
  const Rotationf att = L._kf.GetAttitude();
  const Vec3f w = L._kf.GetAngularVelocity(), p = L._kf.GetPosition(), v = L._kf.GetVelocity();
  const Vec3f a = L._imuAccelerometer.lowPass.GetValue(), g = L._imuRateGyro.lowPass.GetValue();
  float f[31] = {att[0], att[1], att[2], att[3], w.x, w.y, w.z, p.x, p.y, p.z, v.x, v.y, v.z, a.x, a.y, a.z, g.x, g.y, g.z,
                 L._imuTemperature.lowPass.GetValue(), L._battMeas.voltageFiltered, L._monitorMainLoopPeriod.lpDt,
                 L._monitorCmdRate.lpDt};
  for (int k = 0; k < 4; k++) {
    f[23 + k] = L._desMotorSpeeds[k];
    f[27 + k] = L._desMotorForcesForTelemetry[k];
  }
  wr(ih, 5);
  wr(&reset, 1);
  wr(f, 31);
}

static int run_logic(int32_t n) {
  for (int32_t c = 0; c < n; c++) {
    float period;
    int32_t n_ops;
    if (!rd(&period, 1) || !rd(&n_ops, 1) || n_ops < 0) return 2;
    ManualTimer clock;
    std::unique_ptr<Onboard::QuadcopterLogic> L;
    for (int32_t o = 0; o < n_ops; o++) {
      int32_t code;
      if (!rd(&code, 1)) return 2;
      if (code != CLOCK && code != INIT && !L) return 2;
      if (code == CLOCK) {
        uint64_t now;
        if (!rd(&now, 1)) return 2;
        clock.ResetMicroseconds(now);
      } else if (code == INIT) {
        int32_t a[2];
        if (!rd(a, 2)) return 2;
        L.reset(new Onboard::QuadcopterLogic(&clock, period));
        L->Initialise((Onboard::QuadcopterConstants::QuadcopterType) a[0], (uint8_t) a[1]);
      } else if (code == BATTERY) {
        float a[2];
        if (!rd(a, 2)) return 2;
        L->SetBatteryMeasurement(a[0], a[1]);
      } else if (code == GYRO || code == ACC) {
        float a[3];
        if (!rd(a, 3)) return 2;
        if (code == GYRO) L->SetIMUMeasurementRateGyro(a[0], a[1], a[2]);
        else L->SetIMUMeasurementAccelerometer(a[0], a[1], a[2]);
      } else if (code == TEMP) {
        float t;
        if (!rd(&t, 1)) return 2;
        L->SetIMUMeasurementTemperature(t);
      } else if (code == RADIO) {
        int32_t a[2];
        float f[4];
        if (!rd(a, 2) || !rd(f, 4)) return 2;
        RadioTypes::RadioMessageDecoded msg;
        msg.type = (uint8_t) a[0];
        msg.flags = (uint8_t) a[1];
        for (int k = 0; k < RadioTypes::RadioMessageDecoded::NUM_RADIO_FLOAT_FIELDS; k++) msg.floats[k] = k < 4 ? f[k] : 0.0f;
        L->SetRadioMessage(msg);
      } else if (code == RUN) {
        L->Run();
        write_run(*L);
      } else if (code == TELEMETRY) {
        TelemetryPacket::data_packet_t p1, p2;
        memset(&p1, 0, sizeof p1);
        memset(&p2, 0, sizeof p2);
        L->GetTelemetryDataPackets(p1, p2);
        static_assert(sizeof p1 == 30, "a data packet is 30 bytes");
        wr((const uint8_t *) &p1, sizeof p1);
        wr((const uint8_t *) &p2, sizeof p2);
      } else if (code == PLACE) {
        int32_t mask, imu, state;
        float att[4], w[3], lp[20];
        uint64_t reset;
        if (!rd(&mask, 1) || !rd(att, 4) || !rd(w, 3) || !rd(&imu, 1) || !rd(lp, 20) || !rd(&state, 1) || !rd(&reset, 1)) return 2;
        if (mask & 1) L->_kf._att = Rotationf(att[0], att[1], att[2], att[3]);
        if (mask & 2) L->_kf._angVel = Vec3f(w[0], w[1], w[2]);
        if (mask & 4) L->_kf._IMUInitialized = imu != 0;
        if (mask & 8) {
          Vec3f *a[4] = {&L->_imuAccelerometer.lowPass._xm0, &L->_imuAccelerometer.lowPass._xm1, &L->_imuAccelerometer.lowPass._ym0,
                         &L->_imuAccelerometer.lowPass._ym1};
          float *b[4] = {&L->_battVoltageLowPass._xm0, &L->_battVoltageLowPass._xm1, &L->_battVoltageLowPass._ym0, &L->_battVoltageLowPass._ym1};
          float *t[4] = {&L->_imuTemperature.lowPass._xm0, &L->_imuTemperature.lowPass._xm1, &L->_imuTemperature.lowPass._ym0,
                         &L->_imuTemperature.lowPass._ym1};
          for (int k = 0; k < 4; k++) {
            *a[k] = Vec3f(lp[3 * k], lp[3 * k + 1], lp[3 * k + 2]);
            *b[k] = lp[12 + k];
            *t[k] = lp[16 + k];
          }
        }
        if (mask & 16) L->_state = (Onboard::QuadcopterLogic::FlightState) state;
        if (mask & 32) L->_timeSinceLastRadioMessage._lastResetTime_usec = reset;
      } else if (code == MOUNT) {
        float a[3];
        if (!rd(a, 3)) return 2;
        L->_IMU_yaw = a[0];
        L->_IMU_pitch = a[1];
        L->_IMU_roll = a[2];
        L->_R = Rotationf::FromEulerYPR(L->_IMU_yaw, L->_IMU_pitch, L->_IMU_roll).GetRotationMatrix();   // QuadcopterLogic.cpp:118-119
      } else {
        return 2;
      }
    }
  }
  return 0;
}

static int run_vehicle(int32_t n) {
  for (int32_t c = 0; c < n; c++) {
    int32_t h[3];
    double p[33];
    if (!rd(h, 3) || !rd(p, 33) || h[1] < 0 || h[2] < 0) return 2;
    Eigen::Matrix<double, 3, 3> inertia;
    for (int k = 0; k < 9; k++) {
      inertia(k / 3, k % 3) = p[1 + k];
      g_inverse[k] = p[10 + k];
    }
    ManualTimer clock;
    Simulation::Quadcopter_T<Onboard::QuadcopterLogic> q(&clock, p[0], inertia, p[19], Vec3d(p[20], p[21], p[22]), p[23], p[24], p[25],
                                                          p[26], p[27], p[28], Vec3d(p[29], p[30], p[31]), 1,
                                                          (Onboard::QuadcopterConstants::QuadcopterType) h[0], p[32]);
    q._stdDevAccNoise = 0;
    q._stdDevRateGyroNoise = 0;
    std::vector<char> lines;
    int32_t n_lines = 0;
    Onboard::QuadcopterLogic &L = q._logic;
    for (int32_t st = 1; st <= h[2]; st++) {
      const unsigned before = L._cycleCounter;
      clock.AdvanceMicroSeconds((uint64_t) h[1]);
      q.Run();
      if (L._cycleCounter == before) continue;
      const uint64_t now = L._timer._masterTimer->GetMicroSeconds();
      const int32_t ih[6] = {st, (int32_t) L._cycleCounter, (int32_t) L._battMeas.count, (int32_t) L._imuRateGyro.count,
                             (int32_t) L._imuAccelerometer.count, (int32_t) L._imuTemperature.count};
      const float f[3] = {L._battMeas.voltageRaw, L._imuTemperature.rawMeas, L._battMeas.voltageFiltered};
      lines.insert(lines.end(), (const char *) &now, (const char *) &now + sizeof now);
      lines.insert(lines.end(), (const char *) ih, (const char *) ih + sizeof ih);
      lines.insert(lines.end(), (const char *) f, (const char *) f + sizeof f);
      n_lines++;
    }
    wr(&n_lines, 1);
    wr(lines.data(), lines.size());
  }
  return 0;
}

int main() {
  int32_t head[3];
  if (!rd(head, 3) || head[0] != MAGIC || head[2] < 0) return 2;
  wr(head, 3);
  int rc = 2;
  if (head[1] == 0) rc = run_logic(head[2]);
  if (head[1] == 1) rc = run_vehicle(head[2]);
  if (rc) return rc;
  return fflush(stdout) == 0 ? 0 : 1;
}
