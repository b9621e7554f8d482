// tests/cpp/test_fleet.cpp -- agrifly::Fleet<logicType> with more than one vehicle, and the on-device rates logic judged
// against the checker's host logic flown through that Fleet.  Compares on its own and prints ONE JSON object;
// tests/test_gpu_fleet.py runs it once per case and asserts.  Linked against the engine library and the CPU checker
// (oracle/libagrifly_oracle.so): test infrastructure, never the product path.
//
//   test_fleet record <f32|f64>          C1: a recording logicType in a 130-vehicle fleet of the four shipped types
//   test_fleet single                    C1: the single-vehicle Quadcopter_T through the reference's 15-argument call
//   test_fleet equal <f32|f64> <N> <mixed|oneK> <default|persistent> <dt_us> <period>
//                                        C2: engine A = Fleet<OraLogic> (host logic), engine B = the device logic;
//                                        every field of every vehicle after every step, bit for bit
//   test_fleet arena <f32|f64> <N>       C3: the same comparison either side of the Fleet's arena switch (16 384)
//   test_fleet script <N> <mixed|oneK> <dt_us> <period>
//                                        no GPU: C2's script flown by the checker alone (ora_step_batch + ora_logic_tick,
//                                        what oracle_py.ClosedLoopBatch does), for its branch tallies
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "agrifly/Quadcopter_T.hpp"
#include "../../oracle/agrifly_oracle.h"
#include "../../oracle/agrifly_oracle_logic.h"

namespace {

uint32_t bits(float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; }
uint64_t bits(double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; }

void must(afe_engine *e, int rc, const char *what) {
  if (rc == AFE_OK) return;
  std::fprintf(stderr, "test_fleet: %s failed: %s (%s)\n", what, afe_status_string(rc), e ? afe_last_error(e) : "");
  std::exit(3);
}

// the members of the logicType concept no test here uses (Quadcopter_T.cpp:163-199, Quadcopter_T.hpp:53-83)
struct UnusedCalls {
  void Initialise(int, uint8_t) {}
  void GetEstimate(Vec3f &, Vec3f &, Rotationf &, Vec3f &) const {}
  int AddRangingTargetId(uint8_t, Vec3f) { return 0; }
  template <class M> void SetRadioMessage(M const) {}
  template <class P> void GetTelemetryDataPackets(P &, P &) {}
  uint8_t GetNextUWBRangingTarget() const { return 0; }
  void SetUWBMeasurement(float, uint8_t, bool) {}
};

// ---- C1: a logicType that records what it is handed and answers with commands unique to (vehicle, motor, tick) -----
struct RecLogic : UnusedCalls {
  int index, runs, order_ok, stage, type;
  float batt_v, batt_i, temp, gyro[3], acc[3];
  RecLogic(BaseTimer *, float) : index(-1), runs(0), order_ok(1), stage(0), type(-1), batt_v(-1), batt_i(0), temp(0) {
    for (int k = 0; k < 3; k++) gyro[k] = acc[k] = 0;
  }
  void Initialise(int t, uint8_t) { type = t; }
  Vec3f GetAccelerometer() const { return Vec3f(acc[0], acc[1], acc[2]); }
  Vec3f GetRateGyro() const { return Vec3f(gyro[0], gyro[1], gyro[2]); }
  // Quadcopter_T.cpp:163-189, in this order at every tick
  void SetBatteryMeasurement(float v, float i) { order_ok &= (stage == 0); stage = 1; batt_v = v; batt_i = i; }
  void SetIMUMeasurementRateGyro(float x, float y, float z) { order_ok &= (stage == 1); stage = 2; gyro[0] = x; gyro[1] = y; gyro[2] = z; }
  void SetIMUMeasurementAccelerometer(float x, float y, float z) { order_ok &= (stage == 2); stage = 3; acc[0] = x; acc[1] = y; acc[2] = z; }
  void SetIMUMeasurementTemperature(float t) { order_ok &= (stage == 3); stage = 4; temp = t; }
  void Run() { order_ok &= (stage == 4); stage = 5; runs++; }
  float GetMotorSpeedCmd(unsigned m) {
    order_ok &= (stage == 5 + (int)m);                     // motors 0, 1, 2, 3 after Run()
    stage = (m == 3) ? 0 : stage + 1;
    return Command(index, (int)m, runs);
  }
  // exact in float, distinct for every (vehicle < 256, motor, tick <= 15), below every shipped type's motorMaxSpeed
  static float Command(int i, int m, int tick) { return 100.0f + float(4 * i + m) + float(tick) / 16.0f; }
};

const int SHIPPED[4] = {1, 2, 4, 5};

// a fixed shuffle of 0..n-1 (LCG-driven Fisher-Yates): type k % n_types lands on a scattered index
std::vector<uint8_t> shuffled_types(int64_t n, int n_types) {
  std::vector<uint8_t> t((size_t)n);
  for (int64_t i = 0; i < n; i++) t[(size_t)i] = (uint8_t)(i % n_types);
  uint64_t s = 0x9E3779B97F4A7C15ull;
  for (int64_t i = n - 1; i > 0; i--) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    const int64_t j = (int64_t)((s >> 33) % (uint64_t)(i + 1));
    std::swap(t[(size_t)i], t[(size_t)j]);
  }
  return t;
}

struct Fail {   // mismatch bookkeeping: a count per check and the first one in full
  std::vector<std::pair<std::string, long> > counts;
  std::string first;
  void add(const char *check, const std::string &detail) {
    for (size_t k = 0; k < counts.size(); k++)
      if (counts[k].first == check) { counts[k].second++; goto done; }
    counts.push_back(std::make_pair(std::string(check), 1L));
  done:
    if (first.empty()) first = std::string(check) + ": " + detail;
  }
  void declare(const char *check) { counts.push_back(std::make_pair(std::string(check), 0L)); }
  long total() const { long t = 0; for (size_t k = 0; k < counts.size(); k++) t += counts[k].second; return t; }
  void print() const {
    std::printf("\"mismatches\": {");
    for (size_t k = 0; k < counts.size(); k++) std::printf("%s\"%s\": %ld", k ? ", " : "", counts[k].first.c_str(), counts[k].second);
    std::printf("}, \"total_mismatches\": %ld, \"first_mismatch\": \"%s\"", total(), first.c_str());
  }
};

std::string fmt(const char *f, ...) __attribute__((format(printf, 1, 2)));
std::string fmt(const char *f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  std::vsnprintf(buf, sizeof(buf), f, ap);
  va_end(ap);
  return buf;
}

int run_record(int precision) {
  const int64_t N = 130;
  const uint64_t dt_us = 1000;
  const double period = 1.0 / 500.0;
  std::vector<afe_vehicle_params> table(4);
  std::vector<float> volts(4), thr(4);
  for (int k = 0; k < 4; k++) {
    must(0, afe_params_from_type(SHIPPED[k], &table[k]), "afe_params_from_type");
    must(0, afe_low_battery_threshold_from_type(SHIPPED[k], &thr[k]), "afe_low_battery_threshold_from_type");
    volts[k] = agrifly::BatteryVoltage(thr[k]);
  }
  const std::vector<uint8_t> types = shuffled_types(N, 4);
  ManualTimer timer;
  agrifly::Fleet<RecLogic> fleet(&timer, N, table, types, period, precision, -1, volts);
  afe_engine *e = fleet.engine();
  must(e, afe_set_imu_noise(e, 1, 0.1, 0.2, AFE_SEED_DECORRELATED), "afe_set_imu_noise");
  for (int64_t i = 0; i < N; i++) fleet.logic(i).index = (int)i;

  Fail f;
  const char *checks[] = {"call_order", "battery", "current", "temperature", "runs", "gyro", "acc", "cmd_slots", "rotor_speed",
                          "noise_distinct", "accessor_get", "accessor_neighbour", "type_mix"};
  for (size_t k = 0; k < sizeof(checks) / sizeof(*checks); k++) f.declare(checks[k]);
  { int seen[4] = {0, 0, 0, 0}; bool mixed64 = false;
    for (int64_t i = 0; i < N; i++) { seen[types[(size_t)i]]++; if (i < 64 && types[(size_t)i] != types[0]) mixed64 = true; }
    for (int k = 0; k < 4; k++) if (seen[k] < 10) f.add("type_mix", fmt("type entry %d has %d vehicles", k, seen[k]));
    if (!mixed64) f.add("type_mix", "the first 64 vehicles share one type"); }

  std::vector<float> gyro((size_t)(3 * N)), acc((size_t)(3 * N)), cmd((size_t)(4 * N));
  std::vector<double> w((size_t)(4 * N));
  int ticks = 0, steps = 0;
  bool tick_last_step = false;
  for (int s = 0; s < 14; s++) {
    timer.AdvanceMicroSeconds(dt_us);
    const uint64_t before = fleet.ticks();
    fleet.Run();
    steps++;
    const bool tick = fleet.ticks() != before;
    must(e, afe_get_state(e, 0, N, 0, 0, 0, 0, w.data()), "afe_get_state");
    // rotor speeds after this step: the commands in force BEFORE it (zero time constant: speed = command).  The commands of
    // a tick act from the next step on (Quadcopter_T.cpp:187-189).
    for (int64_t i = 0; i < N; i++)
      for (int m = 0; m < 4; m++) {
        const double want = ticks == 0 ? 0.0 : (double)RecLogic::Command((int)i, m, ticks);
        if (bits(w[(size_t)(m * N + i)]) != bits(want))
          f.add("rotor_speed", fmt("step %d vehicle %lld motor %d: rotor speed %.9g, the command in force was %.9g%s", s, (long long)i, m,
                                   w[(size_t)(m * N + i)], want, tick_last_step ? " (set at the previous step's tick)" : ""));
      }
    tick_last_step = tick;
    if (!tick) continue;
    ticks++;
    must(e, afe_get_imu(e, 0, N, gyro.data(), acc.data()), "afe_get_imu");
    must(e, afe_get_motor_cmds(e, 0, N, cmd.data()), "afe_get_motor_cmds");
    for (int64_t i = 0; i < N; i++) {
      const RecLogic &L = fleet.logic(i);
      if (!L.order_ok) f.add("call_order", fmt("tick %d vehicle %lld", ticks, (long long)i));
      if (L.runs != ticks) f.add("runs", fmt("tick %d vehicle %lld ran %d times", ticks, (long long)i, L.runs));
      const float want_v = 1.2f * thr[types[(size_t)i]];
      if (bits(L.batt_v) != bits(want_v))
        f.add("battery", fmt("tick %d vehicle %lld (type %d): handed %.9g V, 1.2f x threshold is %.9g V", ticks, (long long)i,
                             SHIPPED[types[(size_t)i]], L.batt_v, want_v));
      if (bits(L.batt_i) != bits(-1.0f)) f.add("current", fmt("tick %d vehicle %lld: %.9g A", ticks, (long long)i, L.batt_i));
      if (bits(L.temp) != bits(25.0f)) f.add("temperature", fmt("tick %d vehicle %lld: %.9g", ticks, (long long)i, L.temp));
      for (int k = 0; k < 3; k++) {
        if (bits(L.gyro[k]) != bits(gyro[(size_t)(k * N + i)]))
          f.add("gyro", fmt("tick %d vehicle %lld axis %d: logic was handed %.9g, afe_get_imu gives %.9g", ticks, (long long)i, k, L.gyro[k], gyro[(size_t)(k * N + i)]));
        if (bits(L.acc[k]) != bits(acc[(size_t)(k * N + i)]))
          f.add("acc", fmt("tick %d vehicle %lld axis %d: logic was handed %.9g, afe_get_imu gives %.9g", ticks, (long long)i, k, L.acc[k], acc[(size_t)(k * N + i)]));
      }
      for (int m = 0; m < 4; m++)
        if (bits(cmd[(size_t)(m * N + i)]) != bits(RecLogic::Command((int)i, m, ticks)))
          f.add("cmd_slots", fmt("tick %d vehicle %lld motor %d: slot holds %.9g, the logic returned %.9g", ticks, (long long)i, m,
                                 cmd[(size_t)(m * N + i)], RecLogic::Command((int)i, m, ticks)));
      // decorrelated noise: no two vehicles see the same sample
      for (int64_t j = 0; j < i; j++)
        if (bits(gyro[(size_t)i]) == bits(gyro[(size_t)j]) && bits(gyro[(size_t)(N + i)]) == bits(gyro[(size_t)(N + j)]))
          f.add("noise_distinct", fmt("tick %d vehicles %lld and %lld were handed the same gyro sample", ticks, (long long)j, (long long)i));
    }
  }

  // per-index accessors: vehicle i and no neighbour
  const int64_t probe[4] = {0, 63, 64, 129};
  std::vector<double> p0((size_t)(3 * N)), v0((size_t)(3 * N)), q0((size_t)(4 * N)), w0((size_t)(3 * N)), m0((size_t)(4 * N)), x0((size_t)(3 * N));
  std::vector<double> p1(p0), v1(v0), q1(q0), w1(w0), m1(m0), x1(x0);
  for (int c = 0; c < 4; c++) {
    const int64_t i = probe[c];
    must(e, afe_get_state(e, 0, N, p0.data(), v0.data(), q0.data(), w0.data(), m0.data()), "afe_get_state");
    must(e, afe_get_external_force(e, 0, N, x0.data()), "afe_get_external_force");
    // dyadic values: exact in float, so the AFE_F32 engine gives them back bit for bit
    const Vec3d P(1.5 + c, -2.25 - c, 0.75 + 2 * c), V(0.5 + c, 1.25, -3.0 - c), W(0.125 + c, -0.25, 0.375), Fx(0.5, -0.25 - c, 1.0);
    const Rotationd Q(0.5, 0.5, -0.5, 0.5);
    fleet.SetPosition(i, P); fleet.SetVelocity(i, V); fleet.SetAttitude(i, Q); fleet.SetAngularVelocity(i, W);
    fleet.SetExternalForce(i, Fx);
    const Vec3d gp = fleet.GetPosition(i), gv = fleet.GetVelocity(i), gw = fleet.GetAngularVelocity(i);
    const Rotationd gq = fleet.GetAttitude(i);
    for (int k = 0; k < 3; k++)
      if (bits(gp[k]) != bits(P[k]) || bits(gv[k]) != bits(V[k]) || bits(gw[k]) != bits(W[k]))
        f.add("accessor_get", fmt("vehicle %lld axis %d: Get* after Set* gives pos %.17g vel %.17g rate %.17g", (long long)i, k, gp[k], gv[k], gw[k]));
    for (unsigned k = 0; k < 4; k++)
      if (bits(gq[k]) != bits(Q[k])) f.add("accessor_get", fmt("vehicle %lld attitude[%u] = %.17g", (long long)i, k, gq[k]));
    for (unsigned m = 0; m < 4; m++)
      if (bits(fleet.GetMotorSpeed(i, m)) != bits(m0[(size_t)(m * N + i)]))
        f.add("accessor_get", fmt("vehicle %lld GetMotorSpeed(%u) = %.17g, the slab holds %.17g", (long long)i, m, fleet.GetMotorSpeed(i, m), m0[(size_t)(m * N + i)]));
    must(e, afe_get_state(e, 0, N, p1.data(), v1.data(), q1.data(), w1.data(), m1.data()), "afe_get_state");
    must(e, afe_get_external_force(e, 0, N, x1.data()), "afe_get_external_force");
    for (int64_t j = 0; j < N; j++) {
      bool same = true, set = true;
      for (int k = 0; k < 3; k++) {
        same &= bits(p0[(size_t)(k * N + j)]) == bits(p1[(size_t)(k * N + j)]) && bits(v0[(size_t)(k * N + j)]) == bits(v1[(size_t)(k * N + j)]) &&
                bits(w0[(size_t)(k * N + j)]) == bits(w1[(size_t)(k * N + j)]) && bits(x0[(size_t)(k * N + j)]) == bits(x1[(size_t)(k * N + j)]);
        set &= bits(p1[(size_t)(k * N + j)]) == bits(P[k]) && bits(v1[(size_t)(k * N + j)]) == bits(V[k]) && bits(w1[(size_t)(k * N + j)]) == bits(W[k]) &&
               bits(x1[(size_t)(k * N + j)]) == bits(Fx[k]);
      }
      for (int k = 0; k < 4; k++) {
        same &= bits(q0[(size_t)(k * N + j)]) == bits(q1[(size_t)(k * N + j)]) && bits(m0[(size_t)(k * N + j)]) == bits(m1[(size_t)(k * N + j)]);
        set &= bits(q1[(size_t)(k * N + j)]) == bits(Q[(unsigned)k]) && bits(m0[(size_t)(k * N + j)]) == bits(m1[(size_t)(k * N + j)]);
      }
      if (j == i && !set) f.add("accessor_get", fmt("vehicle %lld: the slabs do not hold what Set*(%lld) wrote", (long long)j, (long long)i));
      if (j != i && !same) f.add("accessor_neighbour", fmt("Set*(%lld) changed vehicle %lld", (long long)i, (long long)j));
    }
  }
  std::printf("{\"case\": \"record\", \"precision\": %d, \"vehicles\": %lld, \"steps\": %d, \"ticks\": %d, ", precision, (long long)N, steps, ticks);
  f.print();
  std::printf("}\n");
  return 0;
}

// The single-vehicle drop-in through the reference's own fifteen-argument call (Simulator/Rappids_Simulator/main.cpp:
// 211-218): what voltage does its logic see?  And with the trailing overrides given.
float single_voltage(int type, int how) {
  afe_vehicle_params c;
  must(0, afe_params_from_type(type, &c), "afe_params_from_type");
  agrifly::Matrix33 I;
  for (int k = 0; k < 9; k++) I.m[k] = c.inertia[k];
  ManualTimer timer;
  const Vec3d zero(0, 0, 0), drag(c.lin_drag_coeff_b[0], c.lin_drag_coeff_b[1], c.lin_drag_coeff_b[2]);
  agrifly::Quadcopter_T<RecLogic> *quad;
  if (how == 0)        // the reference's call, nothing appended
    quad = new agrifly::Quadcopter_T<RecLogic>(&timer, c.mass, I, c.arm_length, zero, c.motor_min_speed, c.motor_max_speed,
                                               c.prop_thrust_from_speed_sqr, c.prop_torque_from_speed_sqr, c.motor_time_const,
                                               c.motor_inertia, drag, 1, type, 1.0 / 500.0);
  else if (how == 1)   // an explicit threshold wins
    quad = new agrifly::Quadcopter_T<RecLogic>(&timer, c.mass, I, c.arm_length, zero, c.motor_min_speed, c.motor_max_speed,
                                               c.prop_thrust_from_speed_sqr, c.prop_torque_from_speed_sqr, c.motor_time_const,
                                               c.motor_inertia, drag, 1, type, 1.0 / 500.0, AFE_F32, 5.0f);
  else                 // an explicit 0 is an explicit 0
    quad = new agrifly::Quadcopter_T<RecLogic>(&timer, c.mass, I, c.arm_length, zero, c.motor_min_speed, c.motor_max_speed,
                                               c.prop_thrust_from_speed_sqr, c.prop_torque_from_speed_sqr, c.motor_time_const,
                                               c.motor_inertia, drag, 1, type, 1.0 / 500.0, AFE_F32, 0.0f);
  for (int s = 0; s < 4 && quad->Logic().runs == 0; s++) { timer.AdvanceMicroSeconds(1000); quad->Run(); }
  const float v = quad->Logic().runs > 0 && quad->Logic().type == type ? quad->Logic().batt_v : -2.0f;
  delete quad;
  return v;
}

int run_single() {
  Fail f;
  f.declare("battery_from_type"); f.declare("override");
  std::printf("{\"case\": \"single\", \"handed_volts\": {");
  for (int k = 0; k < 4; k++) {
    const float thr[4] = {3.0f, 3.0f, 9.0f, 6.0f};                 // QuadcopterConstants.hpp:83, 117, 180, 220
    const float v = single_voltage(SHIPPED[k], 0), want = 1.2f * thr[k];
    std::printf("%s\"%d\": %.9g", k ? ", " : "", SHIPPED[k], v);
    if (bits(v) != bits(want))
      f.add("battery_from_type", fmt("type %d through the 15-argument call: the logic was handed %.9g V, 1.2f x %g V is %.9g V", SHIPPED[k], v, thr[k], want));
  }
  const float a = single_voltage(5, 1), b = single_voltage(5, 2);
  if (bits(a) != bits(1.2f * 5.0f)) f.add("override", fmt("explicit threshold 5 V on type 5: handed %.9g V", a));
  if (bits(b) != bits(0.0f)) f.add("override", fmt("explicit threshold 0 V on type 5: handed %.9g V", b));
  std::printf("}, \"override_5V\": %.9g, \"override_0V\": %.9g, ", a, b);
  f.print();
  std::printf("}\n");
  return 0;
}

// ---- C2 / C3: the checker's rates logic as a host logicType --------------------------------------------------------
struct OraLogic : UnusedCalls {
  const ora_logic_params *P;
  ora_logic_branches *tally;
  ora_logic_state S;
  float gyro[3], acc[3];
  OraLogic(BaseTimer *, float) : P(0), tally(0) { std::memset(&S, 0, sizeof(S)); for (int k = 0; k < 3; k++) gyro[k] = acc[k] = 0; }
  void setup(const ora_logic_params *p, ora_logic_branches *t) { P = p; tally = t; ora_logic_init(P, &S); }
  Vec3f GetAccelerometer() const { return Vec3f(acc[0], acc[1], acc[2]); }
  Vec3f GetRateGyro() const { return Vec3f(gyro[0], gyro[1], gyro[2]); }
  void SetBatteryMeasurement(float, float) {}
  void SetIMUMeasurementRateGyro(float x, float y, float z) { gyro[0] = x; gyro[1] = y; gyro[2] = z; }
  void SetIMUMeasurementAccelerometer(float x, float y, float z) { acc[0] = x; acc[1] = y; acc[2] = z; }
  void SetIMUMeasurementTemperature(float) {}
  void Run() { ora_logic_count_branches(tally); ora_logic_tick(P, &S, gyro); ora_logic_count_branches(0); }
  float GetMotorSpeedCmd(unsigned m) const { return S.motor_speed_cmd[m]; }
};

// The six-entry type table: the four shipped types, a tilted IMU mount, a full inertia tensor with a rotor lag.
struct Types {
  std::vector<afe_vehicle_params> vehicle;
  std::vector<afe_rates_logic_params> device_logic;
  std::vector<ora_logic_params> host_logic;
  std::vector<std::string> name;
};
Types make_types(float onboard_period) {
  Types T;
  T.vehicle.resize(6); T.device_logic.resize(6); T.host_logic.resize(6);
  const int base[6] = {1, 2, 4, 5, 5, 2};
  const char *names[6] = {"type1", "type2", "type4", "type5", "tilted_mount", "full_inertia"};
  for (int k = 0; k < 6; k++) {
    must(0, afe_params_from_type(base[k], &T.vehicle[k]), "afe_params_from_type");
    must(0, afe_rates_logic_params_from_type(base[k], &T.device_logic[k]), "afe_rates_logic_params_from_type");
    if (ora_logic_params_from_type(&T.host_logic[k], base[k], onboard_period) != 0) std::exit(3);
    T.name.push_back(names[k]);
  }
  // 4: the IMU is mounted tilted about all three axes -- in the vehicle (the sample the step synthesises is rotated by the
  // inverse mount, Quadcopter_T.cpp:78-80, 166, 175) and in the logic (which rotates it back, QuadcopterLogic.hpp:43)
  const float yaw = 0.4f, pitch = -0.3f, roll = 0.55f;
  T.vehicle[4].imu_yaw = yaw; T.vehicle[4].imu_pitch = pitch; T.vehicle[4].imu_roll = roll;
  T.device_logic[4].imu_yaw = yaw; T.device_logic[4].imu_pitch = pitch; T.device_logic[4].imu_roll = roll;
  ora_logic_set_imu_mount(&T.host_logic[4], yaw, pitch, roll);
  // 5: a full symmetric inertia tensor in the vehicle and in the logic's record, and rotors that lag
  const float I[9] = {30e-6f, 4e-6f, -3e-6f, 4e-6f, 34e-6f, 5e-6f, -3e-6f, 5e-6f, 60e-6f};
  for (int k = 0; k < 9; k++) { T.vehicle[5].inertia[k] = I[k]; T.device_logic[5].inertia[k] = I[k]; T.host_logic[5].inertia[k] = I[k]; }
  T.vehicle[5].motor_time_const = 0.015;
  return T;
}

// The script, in steps.  Commands are (thrust_norm [m/s^2], body rates [rad/s]) for a vehicle range.
struct Command { int step; int64_t first, end; float thrust, w[3]; };
std::vector<Command> make_script(int64_t n, int n_steps) {
  std::vector<Command> c;
  const int64_t sub_end = n < 101 ? n : 101;
  const Command a = {30, 0, n, 9.5f, {0.3f, -0.2f, 0.1f}};                 // all vehicles, the linear range
  const Command b = {70, 17, sub_end, 12.0f, {-1.0f, 0.8f, -0.5f}};        // the sub-range [17, 101) only
  c.push_back(a); c.push_back(b);
  // thrust beyond every type's total-thrust cap; rate steps of alternating sign every 8 steps, large enough to put single
  // propellers above maxThrustPerPropeller and below 0 whatever the vehicle does in between
  for (int s = 110, k = 0; s < n_steps; s += 8, k++) {
    const float sg = (k & 1) ? -1.0f : 1.0f;
    const Command x = {s, 0, n, 100.0f, {sg * 200.0f, sg * -150.0f, sg * 60.0f}};
    c.push_back(x);
  }
  return c;
}
const int N_STEPS = 200, NAN_STEP = 90;

void parse_types(const char *arg, int64_t n, const Types &all, Types &used, std::vector<uint8_t> &index) {
  if (!std::strcmp(arg, "mixed")) { used = all; index = shuffled_types(n, 6); return; }
  if (!std::strncmp(arg, "one", 3) && arg[3] >= '0' && arg[3] <= '5' && !arg[4]) {
    const int k = arg[3] - '0';
    used.vehicle.assign(1, all.vehicle[(size_t)k]); used.device_logic.assign(1, all.device_logic[(size_t)k]);
    used.host_logic.assign(1, all.host_logic[(size_t)k]); used.name.assign(1, all.name[(size_t)k]);
    index.assign((size_t)n, 0);
    return;
  }
  std::fprintf(stderr, "test_fleet: types must be mixed or one0..one5\n");
  std::exit(2);
}

void print_tallies(const Types &T, const std::vector<ora_logic_branches> &tally) {
  std::printf("\"tallies\": {");
  for (size_t k = 0; k < T.name.size(); k++)
    std::printf("%s\"%s\": {\"ticks\": %llu, \"idle\": %llu, \"first_imu\": %llu, \"cap\": %llu, \"lower\": %llu, \"upper\": %llu, "
                "\"f_le0\": %llu, \"f_le0_reachable\": %d}", k ? ", " : "", T.name[k].c_str(), tally[k].ticks, tally[k].idle, tally[k].first_imu,
                tally[k].cap, tally[k].lower, tally[k].upper, tally[k].f_le0, T.host_logic[k].min_thrust <= 0.0f ? 1 : 0);
  std::printf("}");
}

struct Snapshot {
  std::vector<float> cmd, gyro, acc;
  std::vector<double> pos, vel, att, w, rotor;
  explicit Snapshot(int64_t n) : cmd((size_t)(4 * n)), gyro((size_t)(3 * n)), acc((size_t)(3 * n)), pos((size_t)(3 * n)), vel((size_t)(3 * n)),
                                 att((size_t)(4 * n)), w((size_t)(3 * n)), rotor((size_t)(4 * n)) {}
  void read(afe_engine *e, int64_t n) {
    must(e, afe_get_motor_cmds(e, 0, n, cmd.data()), "afe_get_motor_cmds");
    must(e, afe_get_state(e, 0, n, pos.data(), vel.data(), att.data(), w.data(), rotor.data()), "afe_get_state");
    must(e, afe_get_imu(e, 0, n, gyro.data(), acc.data()), "afe_get_imu");
  }
};

// value-wise with NaN equal to NaN, and non-finite in the same slots
template <class T> bool same_value(T a, T b) { return (a != a && b != b) || (a == b && std::isfinite(a) == std::isfinite(b)); }

// A against B over every field of every vehicle.  `loose` (or -1) is the one vehicle compared value-wise.
template <class T>
void compare_field(const char *field, const std::vector<T> &a, const std::vector<T> &b, int comps, int64_t n, int64_t loose, int step, Fail &f,
                   long &loose_nonfinite, const int64_t *named, int n_named) {
  for (int k = 0; k < comps; k++)
    for (int64_t i = 0; i < n; i++) {
      const T x = a[(size_t)(k * n + i)], y = b[(size_t)(k * n + i)];
      bool ok;
      if (i == loose) { ok = same_value(x, y); loose_nonfinite += !std::isfinite(x); }
      else ok = bits(x) == bits(y);
      if (ok) continue;
      std::string who;
      for (int q = 0; q < n_named; q++) if (named[q] == i) who = fmt(" [NAMED VEHICLE %lld]", (long long)i);
      f.add(field, fmt("step %d vehicle %lld%s %s[%d]: host logic engine %.17g (%#llx), device logic engine %.17g (%#llx)", step, (long long)i,
                       who.c_str(), field, k, (double)x, (unsigned long long)bits(x), (double)y, (unsigned long long)bits(y)));
    }
}

int run_equal(const char *label, int precision, int64_t N, const char *types_arg, const char *mode, uint64_t dt_us, double period, bool arena) {
  const Types all = make_types(float(period));
  Types T;
  std::vector<uint8_t> index;
  parse_types(types_arg, N, all, T, index);
  const int n_steps = arena ? 8 : N_STEPS;
  const int64_t nanv = arena ? -1 : (N > 77 ? 77 : N / 2 + 8);
  const int64_t named[3] = {0, 16383, 16384};

  ManualTimer timer;
  agrifly::Fleet<OraLogic> A(&timer, N, T.vehicle, index, period, precision);
  std::vector<ora_logic_branches> tally(T.name.size());
  std::memset(tally.data(), 0, sizeof(ora_logic_branches) * tally.size());
  for (int64_t i = 0; i < N; i++) A.logic(i).setup(&T.host_logic[index[(size_t)i]], &tally[index[(size_t)i]]);
  // B: the creation call the Fleet chose for this N (Quadcopter_T.hpp, Fleet::init)
  afe_engine *B = 0;
  if (N <= 16384) must(0, afe_create_host_visible(&B, N, precision, -1, 0), "afe_create_host_visible");
  else must(0, afe_create(&B, N, precision, -1, 0), "afe_create");
  must(B, afe_set_type_table(B, T.vehicle.data(), (int)T.vehicle.size()), "afe_set_type_table");
  must(B, afe_set_vehicle_types(B, 0, N, index.data()), "afe_set_vehicle_types");
  must(B, afe_set_logic_period(B, period), "afe_set_logic_period");
  must(B, afe_set_rates_logic(B, T.device_logic.data(), (int)T.device_logic.size()), "afe_set_rates_logic");
  if (!std::strcmp(mode, "persistent")) must(B, afe_set_step_mode(B, AFE_STEP_PERSISTENT), "afe_set_step_mode");
  else if (std::strcmp(mode, "default")) { std::fprintf(stderr, "test_fleet: mode must be default or persistent\n"); return 2; }
  afe_engine *engines[2] = {A.engine(), B};
  // the same state and noise policy on both: a spread of attitudes, rates and velocities, decorrelated IMU noise
  std::vector<double> pos((size_t)(3 * N)), vel((size_t)(3 * N)), att((size_t)(4 * N)), w((size_t)(3 * N));
  for (int64_t i = 0; i < N; i++) {
    const double u = (double)(i % 97) / 97.0, v = (double)(i % 31) / 31.0;
    pos[(size_t)i] = 0.5 * (double)(i % 13); pos[(size_t)(N + i)] = -0.25 * (double)(i % 7); pos[(size_t)(2 * N + i)] = 1.0 + u;
    vel[(size_t)i] = u - 0.5; vel[(size_t)(N + i)] = 0.5 - v; vel[(size_t)(2 * N + i)] = 0.25 * (u - v);
    const Rotationd q = Rotationd::FromEulerYPR(0.6 * (u - 0.5), 0.3 * (v - 0.5), 0.4 * (u + v - 1.0));
    for (unsigned k = 0; k < 4; k++) att[(size_t)((int64_t)k * N + i)] = q[k];
    w[(size_t)i] = 0.8 * (v - 0.5); w[(size_t)(N + i)] = 0.6 * (u - 0.5); w[(size_t)(2 * N + i)] = 0.3 * (u - v);
  }
  for (int k = 0; k < 2; k++) {
    must(engines[k], afe_set_state(engines[k], 0, N, pos.data(), vel.data(), att.data(), w.data(), 0), "afe_set_state");
    must(engines[k], afe_set_imu_noise(engines[k], 1, 0.1, 0.2, AFE_SEED_DECORRELATED), "afe_set_imu_noise");
  }

  Fail f;
  const char *fields[] = {"motor_cmds", "pos", "vel", "att", "ang_vel", "rotor_speed", "gyro", "acc", "logic_ticks"};
  for (size_t k = 0; k < sizeof(fields) / sizeof(*fields); k++) f.declare(fields[k]);
  std::vector<Command> script = make_script(N, n_steps);
  if (arena) {   // three logic ticks; the command is in force from the start so that the later ticks do real work
    script.clear();
    const Command c = {0, 0, N, 9.5f, {0.3f, -0.2f, 0.1f}};
    script.push_back(c);
  }
  Snapshot sa(N), sb(N);
  long loose_nonfinite = 0;
  int persistent_seen = 0, steps_done = 0;
  uint64_t ticks_a = 0, ticks_b = 0;
  int nonzero = 0, distinct = 0;
  std::vector<float> thrust, w3;
  for (int s = 0; s < n_steps; s++) {
    for (size_t c = 0; c < script.size(); c++) {
      if (script[c].step != s) continue;
      const Command &cmd = script[c];
      const int64_t cnt = cmd.end - cmd.first;
      for (int64_t i = cmd.first; i < cmd.end; i++) ora_logic_set_rates_cmd(&A.logic(i).S, cmd.thrust, cmd.w);
      thrust.assign((size_t)cnt, cmd.thrust);
      w3.resize((size_t)(3 * cnt));
      for (int k = 0; k < 3; k++) for (int64_t i = 0; i < cnt; i++) w3[(size_t)(k * cnt + i)] = cmd.w[k];
      must(B, afe_set_rates_commands(B, cmd.first, cnt, thrust.data(), w3.data()), "afe_set_rates_commands");
    }
    if (s == NAN_STEP && nanv >= 0) {   // one vehicle's body rate goes non-finite, through both engines
      const double nan = std::numeric_limits<double>::quiet_NaN();
      A.SetAngularVelocity(nanv, Vec3d(nan, 0.5, -0.25));
      const double wn[3] = {nan, 0.5, -0.25};
      must(B, afe_set_state(B, nanv, 1, 0, 0, 0, wn, 0), "afe_set_state");
    }
    timer.AdvanceMicroSeconds(dt_us);
    A.Run();
    must(B, afe_step(B, dt_us, 1), "afe_step");
    int running = 0;
    must(B, afe_persistent_running(B, &running), "afe_persistent_running");
    persistent_seen += running;
    steps_done++;
    sa.read(A.engine(), N); sb.read(B, N);
    const int64_t loose = (s >= NAN_STEP) ? nanv : -1;
    compare_field("motor_cmds", sa.cmd, sb.cmd, 4, N, loose, s, f, loose_nonfinite, named, 3);
    compare_field("pos", sa.pos, sb.pos, 3, N, loose, s, f, loose_nonfinite, named, 3);
    compare_field("vel", sa.vel, sb.vel, 3, N, loose, s, f, loose_nonfinite, named, 3);
    compare_field("att", sa.att, sb.att, 4, N, loose, s, f, loose_nonfinite, named, 3);
    compare_field("ang_vel", sa.w, sb.w, 3, N, loose, s, f, loose_nonfinite, named, 3);
    compare_field("rotor_speed", sa.rotor, sb.rotor, 4, N, loose, s, f, loose_nonfinite, named, 3);
    compare_field("gyro", sa.gyro, sb.gyro, 3, N, loose, s, f, loose_nonfinite, named, 3);
    compare_field("acc", sa.acc, sb.acc, 3, N, loose, s, f, loose_nonfinite, named, 3);
    must(A.engine(), afe_logic_ticks(A.engine(), &ticks_a), "afe_logic_ticks");
    must(B, afe_logic_ticks(B, &ticks_b), "afe_logic_ticks");
    if (ticks_a != ticks_b) f.add("logic_ticks", fmt("step %d: %llu against %llu", s, (unsigned long long)ticks_a, (unsigned long long)ticks_b));
    // did the run do anything?  In the linear range (before the NaN and the saturating commands) a vehicle's commands are
    // not all zero and differ from its neighbour's: every vehicle sees noise of its own
    if (s == (arena ? n_steps - 1 : NAN_STEP - 1))
      for (int64_t i = 0; i < N; i++) {
        bool nz = false, df = false;
        for (int m = 0; m < 4; m++) {
          nz |= sa.cmd[(size_t)(m * N + i)] != 0.0f;
          if (i) df |= bits(sa.cmd[(size_t)(m * N + i)]) != bits(sa.cmd[(size_t)(m * N + i - 1)]);
        }
        nonzero += nz; distinct += df;
      }
  }
  int rp = -1, ad = -1;
  must(B, afe_step_kernel_info(B, &rp, &ad), "afe_step_kernel_info");
  std::printf("{\"case\": \"%s\", \"precision\": %d, \"vehicles\": %lld, \"types\": \"%s\", \"mode\": \"%s\", \"dt_us\": %llu, \"period\": %.17g, "
              "\"steps\": %d, \"logic_ticks\": %llu, \"nonfinite_vehicle\": %lld, \"nonfinite_slots_seen\": %ld, \"resident_grid_steps\": %d, "
              "\"record_path\": %d, \"vehicles_with_nonzero_cmd\": %d, \"neighbours_with_distinct_cmd\": %d, ",
              label, precision, (long long)N, types_arg, mode, (unsigned long long)dt_us, period, steps_done, (unsigned long long)ticks_a,
              (long long)nanv, loose_nonfinite, persistent_seen, rp, nonzero, distinct);
  print_tallies(T, tally);
  std::printf(", ");
  f.print();
  std::printf("}\n");
  afe_destroy(B);
  return 0;
}

// No GPU: the script flown by the checker alone, for the branch tallies it reaches.
int run_script(int64_t N, const char *types_arg, uint64_t dt_us, double period) {
  const Types all = make_types(float(period));
  Types T;
  std::vector<uint8_t> index;
  parse_types(types_arg, N, all, T, index);
  std::vector<ora_params> table(T.vehicle.size());
  for (size_t k = 0; k < table.size(); k++) {
    const afe_vehicle_params &v = T.vehicle[k];
    ora_params_init(&table[k], v.mass, v.inertia, v.arm_length, v.com_error, v.motor_min_speed, v.motor_max_speed, v.prop_thrust_from_speed_sqr,
                    v.prop_torque_from_speed_sqr, v.motor_time_const, v.motor_inertia, v.lin_drag_coeff_b, v.imu_yaw, v.imu_pitch, v.imu_roll);
  }
  std::vector<double> pos((size_t)(3 * N), 0.0), vel((size_t)(3 * N), 0.0), att((size_t)(4 * N), 0.0), w((size_t)(3 * N), 0.0), rotor((size_t)(4 * N), 0.0);
  std::vector<double> xf((size_t)(3 * N), 0.0), xt((size_t)(3 * N), 0.0);
  std::vector<float> cmd((size_t)(4 * N), 0.0f), gyro((size_t)(3 * N), 0.0f), acc((size_t)(3 * N), 0.0f);
  std::vector<uint32_t> rng((size_t)N);
  std::vector<ora_logic_state> S((size_t)N);
  std::vector<ora_logic_branches> tally(T.name.size());
  std::memset(tally.data(), 0, sizeof(ora_logic_branches) * tally.size());
  for (int64_t i = 0; i < N; i++) {
    att[(size_t)i] = 1.0;
    rng[(size_t)i] = (uint32_t)(1 + i);   // AFE_SEED_DECORRELATED
    pos[(size_t)(2 * N + i)] = 1.0;
    w[(size_t)i] = 0.8 * ((double)(i % 31) / 31.0 - 0.5);
    ora_logic_init(&T.host_logic[index[(size_t)i]], &S[(size_t)i]);
  }
  ora_clock clock;
  ora_clock_init(&clock, period);
  const std::vector<Command> script = make_script(N, N_STEPS);
  uint64_t ticks = 0;
  for (int s = 0; s < N_STEPS; s++) {
    for (size_t c = 0; c < script.size(); c++)
      if (script[c].step == s)
        for (int64_t i = script[c].first; i < script[c].end; i++) ora_logic_set_rates_cmd(&S[(size_t)i], script[c].thrust, script[c].w);
    ora_clock_advance(&clock, dt_us);
    int tick = 0;
    const double dt = ora_clock_run(&clock, &tick);
    const uint8_t t8 = (uint8_t)tick;
    ora_step_batch(N, 1, table.data(), index.data(), pos.data(), vel.data(), att.data(), w.data(), rotor.data(), rng.data(), cmd.data(), xf.data(),
                   xt.data(), dt, &t8, gyro.data(), acc.data());
    if (!tick) continue;
    ticks++;
    for (int64_t i = 0; i < N; i++) {
      const float g[3] = {gyro[(size_t)i], gyro[(size_t)(N + i)], gyro[(size_t)(2 * N + i)]};
      ora_logic_count_branches(&tally[index[(size_t)i]]);
      ora_logic_tick(&T.host_logic[index[(size_t)i]], &S[(size_t)i], g);
      for (int m = 0; m < 4; m++) cmd[(size_t)(m * N + i)] = S[(size_t)i].motor_speed_cmd[m];
    }
    ora_logic_count_branches(0);
  }
  std::printf("{\"case\": \"script\", \"vehicles\": %lld, \"types\": \"%s\", \"dt_us\": %llu, \"period\": %.17g, \"steps\": %d, \"logic_ticks\": %llu, ",
              (long long)N, types_arg, (unsigned long long)dt_us, period, N_STEPS, (unsigned long long)ticks);
  print_tallies(T, tally);
  std::printf("}\n");
  return 0;
}

int precision_of(const char *a) {
  if (!std::strcmp(a, "f64")) return AFE_F64;
  if (!std::strcmp(a, "f32")) return AFE_F32;
  std::fprintf(stderr, "test_fleet: precision must be f32 or f64\n");
  std::exit(2);
}

}  // namespace

int main(int argc, char **argv) {
  const std::string cmd = argc > 1 ? argv[1] : "";
  if (cmd == "record" && argc == 3) return run_record(precision_of(argv[2]));
  if (cmd == "single" && argc == 2) return run_single();
  if (cmd == "equal" && argc == 8)
    return run_equal("equal", precision_of(argv[2]), atoll(argv[3]), argv[4], argv[5], (uint64_t)atoll(argv[6]), atof(argv[7]), false);
  if (cmd == "arena" && argc == 4) return run_equal("arena", precision_of(argv[2]), atoll(argv[3]), "one3", "default", 1000, 1.0 / 500.0, true);
  if (cmd == "script" && argc == 6) return run_script(atoll(argv[2]), argv[3], (uint64_t)atoll(argv[4]), atof(argv[5]));
  std::fprintf(stderr, "usage: test_fleet record <f32|f64> | single | equal <f32|f64> <N> <mixed|oneK> <default|persistent> <dt_us> <period> | "
                       "arena <f32|f64> <N> | script <N> <mixed|oneK> <dt_us> <period>\n");
  return 2;
}
