// oracle/ref_rigid_body_probe.cpp -- TEST INFRASTRUCTURE.
// The REFERENCE's own rigid-body step, compiled from where it lies:
//   Components/Components/Simulation/Quadcopter_T.cpp   (the constructor and Quadcopter_T::Run, #included below because its
//                                                        member templates must be visible where they are instantiated)
//   Components/Components/Simulation/Motor.cpp          (named on the compiler's command line, oracle/Makefile)
// driven by Common/Common/Time/ManualTimer.hpp.  -I oracle/eigen_store: Eigen::Matrix is storage and constants only, so
// any Eigen arithmetic on this path would not compile.  Quadcopter_T.cpp performs one Eigen operation,
// inertiaMatrix.inverse() in the constructor (:20); eigen_store declares inverse() and defines none.
//
// This file's own text is three things and nothing of the step itself:
//   1. Matrix<double, 3, 3>::inverse(), an explicit specialisation that hands back the nine numbers of the request (the
//      tests give it ora_params_init's; how far those are from the exact inverse is judged apart, tests/
//      test_rigid_body_reference.py).  <double, 3, 3> alone: any other inverse() is a link error.
//   2. ScriptLogic, the logicType Quadcopter_T is instantiated with: it records what Run() hands the onboard logic (the
//      gyro and accelerometer floats) and how often, and replays a table of motor-speed commands, one row per tick.
//      QuadcopterLogic.cpp and KalmanFilter6DOF.cpp are not compiled.
//   3. Probe, a subclass that writes the protected _motorSpeedCommands (the commands before the first tick).
//   4. (closed loop, second request kind) ChainLogic, a logicType that composes the reference's own onboard headers in
//      QuadcopterLogic.cpp's order -- LowPassFilterSecondOrder<float, Vec3f>, QuadcopterAngularVelocityController::
//      GetDesiredTorques, QuadcopterMixer::GetMotorForces / PropellerSpeedsFromThrust, parameters from
//      QuadcopterConstants(type).  Those headers' arithmetic is the reference's; the GLUE between them is this file's own
//      reading of QuadcopterLogic.cpp / KalmanFilter6DOF.cpp (cited line by line at ChainLogic) and stays UNPINNED.
// Motor has no getter for its speed, Quadcopter_T none for its motors: private members are read, nothing is changed
// (as in ref_motion_probe.cpp).
//
// usage: rigid_body_probe < request > answer     (binary, little endian; tests/golden/make_rigid_body_reference.py)
//   request: int32 magic, int32 n_cases, then per case
//     int32  type, dt_us, n_steps, n_checkpoints, n_rows
//     double mass, inertia[9], inverse[9], arm, com[3], min_speed, max_speed, k_thrust, k_torque, tau, J, drag[3], period
//     double pos[3], vel[3], att[4], ang_vel[3], ext_force[3], ext_torque[3]
//     float  cmd0[4]                 the commands before the first tick
//     int32  checkpoint[n_checkpoints]   step numbers, 1-based: recorded after that many steps
//     float  rows[n_rows][4]         ScriptLogic::Run number r leaves row min(r, n_rows - 1)
//   per step: AdvanceMicroSeconds(dt_us); Run()
//   answer: int32 magic, int32 n_cases, then per case uint8 tick[n_steps] (did Run number s call the logic) and per
//     checkpoint  int32 step, int32 ticks, double pos[3], vel[3], att[4], ang_vel[3], motor_speed[4],
//                 float gyro[3], acc[3] (the last sample handed over; 0 before the first), float cmd[4]
//   closed loop: the same with magic "RQC1"; cmd0 is ignored (the reference starts at 0), a row is five floats
//     (step, thrust_norm, wx, wy, wz): the rates command handed to the logic before Run number `step` (1-based), and a
//     checkpoint carries four more floats, the motor forces the mixer left (_desMotorForcesForTelemetry)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
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
#include "Components/Simulation/Quadcopter_T.hpp"
#undef private
#include "Common/Time/ManualTimer.hpp"

static std::vector<float> g_rows;   // [n_rows][ROW], set before a Quadcopter_T is built

// what Quadcopter_T.hpp's inline virtuals name and neither stub uses
class UnusedLogicCalls {
 public:
  void SetBatteryMeasurement(float, float) {}
  void SetIMUMeasurementTemperature(float) {}
  uint8_t GetNextUWBRangingTarget() const { return 0; }
  void SetUWBMeasurement(float, uint8_t, bool) {}
  void GetEstimate(Vec3f &, Vec3f &, Rotationf &, Vec3f &) const {}
  int AddRangingTargetId(uint8_t, Vec3f) { return 0; }
  void SetRadioMessage(RadioTypes::RadioMessageDecoded const) {}
  void GetTelemetryDataPackets(TelemetryPacket::data_packet_t &, TelemetryPacket::data_packet_t &) {}
};

class ScriptLogic : public UnusedLogicCalls {
 public:
  enum { ROW = 4, N_FORCE = 0 };
  ScriptLogic(BaseTimer *const, float) : ticks(0) {
    for (int k = 0; k < 3; k++) gyro[k] = acc[k] = 0;
    for (int k = 0; k < 4; k++) cmd[k] = force[k] = 0;
  }
  void BeforeStep(int) {}
  void Initialise(Onboard::QuadcopterConstants::QuadcopterType, uint8_t) {}
  void SetIMUMeasurementRateGyro(float x, float y, float z) { gyro[0] = x; gyro[1] = y; gyro[2] = z; }
  void SetIMUMeasurementAccelerometer(float x, float y, float z) { acc[0] = x; acc[1] = y; acc[2] = z; }
  void Run() {
    const size_t n_rows = g_rows.size() / 4, r = (size_t) ticks < n_rows ? (size_t) ticks : n_rows - 1;
    for (int k = 0; k < 4; k++) cmd[k] = g_rows[4 * r + k];
    ticks++;
  }
  float GetMotorSpeedCmd(unsigned i) const { return cmd[i]; }
  Vec3f GetAccelerometer() const { return Vec3f(acc[0], acc[1], acc[2]); }
  Vec3f GetRateGyro() const { return Vec3f(gyro[0], gyro[1], gyro[2]); }

  int ticks;
  float gyro[3], acc[3], cmd[4], force[4];
};

// The onboard rates-control chain from the reference's own headers.  Everything marked GLUE is this file's reading of
// the two sources that do not compile here, cited as oracle/agrifly_oracle_logic.c cites them.
class ChainLogic : public UnusedLogicCalls {
 public:
  enum { ROW = 5, N_FORCE = 4 };
  ChainLogic(BaseTimer *const, float onboardLogicPeriod)
      : ticks(0), period_(onboardLogicPeriod), mass_(0), gyro_raw_(0, 0, 0), w_est_(0, 0, 0), w_des_(0, 0, 0),
        thrust_norm_(0), imu_seen_(false), have_cmd_(false) {
    for (int k = 0; k < 3; k++) gyro[k] = acc[k] = 0;
    for (int k = 0; k < 4; k++) cmd[k] = force[k] = 0;       // QuadcopterLogic.cpp:24-27
  }
  void Initialise(Onboard::QuadcopterConstants::QuadcopterType type, uint8_t) {
    Onboard::QuadcopterConstants consts(type);                // GLUE: QuadcopterLogic.cpp:111-150, the lines of this chain
    mass_ = consts.mass;                                      // :113
    mount_ = Rotationf::FromEulerYPR(consts.IMU_yaw, consts.IMU_pitch, consts.IMU_roll).GetRotationMatrix();   // :115-119
    gyro_lpf_.Initialise(period_, 200.0f, gyro_raw_);    // :103, :133-134
    rate_ctrl_.SetParameters(consts.angVelControl_timeConst_xy, consts.angVelControl_timeConst_z, consts.inertiaMatrix);   // :144-146
    mixer_.SetParameters(consts.armLength, consts.propellerThrustFromSpeedSqr, consts.propellerTorqueFromThrust,
                         consts.prop0SpinDir, consts.maxThrustPerPropeller, consts.minThrustPerPropeller,
                         consts.maxCmdTotalThrust);           // :124-127, :147-150
  }
  void SetIMUMeasurementRateGyro(float x, float y, float z) {  // QuadcopterLogic.hpp:40-45; _gyroCalibrationBias = 0 (ResetGyroCalibration, QuadcopterLogic.cpp:93)
    gyro[0] = x; gyro[1] = y; gyro[2] = z;
    gyro_raw_ = mount_ * Vec3f(x, y, z);
    gyro_lpf_.Apply(gyro_raw_ - Vec3f(0, 0, 0));
  }
  void SetIMUMeasurementAccelerometer(float x, float y, float z) { acc[0] = x; acc[1] = y; acc[2] = z; }
  // GLUE: SetRadioMessage + ParseIncomingCommunications for an externalRatesCmd (QuadcopterLogic.cpp:275-303)
  void BeforeStep(int st) {
    for (size_t r = 0; r < g_rows.size() / ROW; r++) {
      const float *row = &g_rows[ROW * r];
      if ((int) row[0] != st) continue;
      have_cmd_ = true;
      thrust_norm_ = row[1];
      w_des_ = Vec3f(row[2], row[3], row[4]);
    }
  }
  void Run() {
    ticks++;
    // GLUE: UpdateEstimator -> KalmanFilter6DOF::Predict (KalmanFilter6DOF.cpp:70-147): the first call initialises only
    // (:71-108); afterwards, without UWB, w_est_ = measGyro (:114-115), measGyro being the low-pass value (QuadcopterLogic.cpp:224)
    if (!imu_seen_) imu_seen_ = true;
    else w_est_ = gyro_lpf_.GetValue();
    if (!have_cmd_) {                                      // GLUE: FS_IDLE, QuadcopterLogic.cpp:207-218
      for (int k = 0; k < 4; k++) cmd[k] = force[k] = 0;
      return;
    }
    // RunControllerExternalRatesControl, QuadcopterLogic.cpp:528-541
    const Vec3f torque = rate_ctrl_.GetDesiredTorques(w_des_, w_est_);
    mixer_.GetMotorForces(thrust_norm_ * mass_, torque, force);
    mixer_.PropellerSpeedsFromThrust(force, cmd);
  }
  float GetMotorSpeedCmd(unsigned i) const { return cmd[i]; }
  Vec3f GetAccelerometer() const { return Vec3f(acc[0], acc[1], acc[2]); }
  Vec3f GetRateGyro() const { return gyro_lpf_.GetValue(); }

  int ticks;
  float gyro[3], acc[3], cmd[4], force[4];

 private:
  const float period_;
  float mass_;
  Matrix<float, 3, 3> mount_;
  Vec3f gyro_raw_, w_est_, w_des_;
  float thrust_norm_;
  bool imu_seen_, have_cmd_;
  LowPassFilterSecondOrder<float, Vec3f> gyro_lpf_;
  Onboard::QuadcopterAngularVelocityController rate_ctrl_;
  Onboard::QuadcopterMixer mixer_;
};

#include "Components/Simulation/Quadcopter_T.cpp"

template <class Logic>
class Probe : public Simulation::Quadcopter_T<Logic> {
 public:
  typedef Simulation::Quadcopter_T<Logic> Base;
  using Base::Base;
  void SetCommands(const float c[4]) {
    for (int k = 0; k < 4; k++) this->_motorSpeedCommands[k] = c[k];
  }
  Logic &TheLogic() { return this->_logic; }
  float Command(int k) const { return this->_motorSpeedCommands[k]; }
  double MotorSpeed(int k) const { return this->_motors[k]._speed; }
};

static const int32_t MAGIC = 0x31425152, MAGIC_CHAIN = 0x31435152;   // "RQB1", "RQC1"

template <typename T>
static bool rd(T *v, size_t n) { return fread(v, sizeof(T), n, stdin) == n; }
template <typename T>
static void wr(const T *v, size_t n) { fwrite(v, sizeof(T), n, stdout); }

template <class Logic>
static int run_cases(int32_t n_cases) {
  for (int32_t c = 0; c < n_cases; c++) {
    int32_t h[5];
    double p[33], s[19];
    float cmd0[4];
    if (!rd(h, 5) || !rd(p, 33) || !rd(s, 19) || !rd(cmd0, 4)) return 2;
    const int32_t type = h[0], dt_us = h[1], n_steps = h[2], n_check = h[3], n_rows = h[4];
    if (dt_us < 0 || n_steps < 1 || n_check < 1 || n_rows < 1) return 2;
    std::vector<int32_t> check(n_check);
    g_rows.assign((size_t) Logic::ROW * n_rows, 0.0f);
    if (!rd(check.data(), check.size()) || !rd(g_rows.data(), g_rows.size())) return 2;

    Eigen::Matrix<double, 3, 3> inertia;
    for (int k = 0; k < 9; k++) {
      inertia(k / 3, k % 3) = p[1 + k];
      g_inverse[k] = p[10 + k];
    }
    ManualTimer clock;
    Probe<Logic> q(&clock, p[0], inertia, p[19], Vec3d(p[20], p[21], p[22]), p[23], p[24], p[25], p[26], p[27], p[28],
                   Vec3d(p[29], p[30], p[31]), 1, (Onboard::QuadcopterConstants::QuadcopterType) type, p[32]);
    const double *x = s;
    q.SetPosition(Vec3d(x[0], x[1], x[2]));
    q.SetVelocity(Vec3d(x[3], x[4], x[5]));
    q.SetAttitude(Rotationd(x[6], x[7], x[8], x[9]));
    q.SetAngularVelocity(Vec3d(x[10], x[11], x[12]));
    q.SetExternalForce(Vec3d(x[13], x[14], x[15]));
    q.SetExternalTorque(Vec3d(x[16], x[17], x[18]));
    if (Logic::N_FORCE == 0) q.SetCommands(cmd0);

    std::vector<uint8_t> tick(n_steps);
    std::vector<char> rec;
    Logic &L = q.TheLogic();
    for (int32_t st = 1; st <= n_steps; st++) {
      const int before = L.ticks;
      L.BeforeStep(st);
      clock.AdvanceMicroSeconds((uint64_t) dt_us);
      q.Run();
      tick[st - 1] = (uint8_t) (L.ticks - before);
      for (int32_t k = 0; k < n_check; k++) {
        if (check[k] != st) continue;
        const Vec3d pos = q.GetPosition(), vel = q.GetVelocity(), av = q.GetAngularVelocity();
        const Rotationd att = q.GetAttitude();
        const int32_t ih[2] = {st, L.ticks};
        const double d[17] = {pos.x, pos.y, pos.z, vel.x, vel.y, vel.z, att[0], att[1], att[2], att[3], av.x, av.y, av.z,
                              q.MotorSpeed(0), q.MotorSpeed(1), q.MotorSpeed(2), q.MotorSpeed(3)};
        const float f[14] = {L.gyro[0], L.gyro[1], L.gyro[2], L.acc[0], L.acc[1], L.acc[2],
                             q.Command(0), q.Command(1), q.Command(2), q.Command(3), L.force[0], L.force[1], L.force[2], L.force[3]};
        rec.insert(rec.end(), (const char *) ih, (const char *) ih + sizeof ih);
        rec.insert(rec.end(), (const char *) d, (const char *) d + sizeof d);
        rec.insert(rec.end(), (const char *) f, (const char *) f + sizeof(float) * (10 + Logic::N_FORCE));
      }
    }
    wr(tick.data(), tick.size());
    wr(rec.data(), rec.size());
  }
  return 0;
}

int main() {
  int32_t head[2];
  if (!rd(head, 2) || (head[0] != MAGIC && head[0] != MAGIC_CHAIN)) return 2;
  wr(head, 2);
  const int rc = head[0] == MAGIC ? run_cases<ScriptLogic>(head[1]) : run_cases<ChainLogic>(head[1]);
  if (rc) return rc;
  return fflush(stdout) == 0 ? 0 : 1;
}
