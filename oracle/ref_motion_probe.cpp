// oracle/ref_motion_probe.cpp -- TEST INFRASTRUCTURE.
// Known answers from the REFERENCE's own rotation math and rotor model, compiled from where they lie:
//   Common/Common/Math/Rotation.hpp   (Rotation<double>, and Rotation<float> for the IMU mount)
//   Components/Components/Simulation/Motor.{hpp,cpp}, driven by Common/Common/Time/ManualTimer.hpp
// Rotation.hpp includes Matrix.hpp, which includes <Eigen/Dense>: the Makefile puts oracle/eigen_decl first on the
// include path, a header that only DECLARES Eigen::Matrix.  Any Eigen arithmetic on a path printed here would not compile.
//
// usage: motion_probe < cases   (one case per line, numbers as C99 hex floats or decimals; one JSON object per line out)
//   R rx ry rz                    Rotation<double>::FromRotationVector(Vec3d(r))
//   P a0 a1 a2 a3 wx wy wz dt     att * FromRotationVector(angVel * dt), Quadcopter_T.cpp:142 (angVel * dt in double)
//   M a0 a1 a2 a3 b0 b1 b2 b3     a * b (quaternion product, Rotation.hpp:124-131)
//   V q0 q1 q2 q3 x y z           q * v and q.Inverse() * v
//   E y p r                       Rotation<double>::FromEulerYPR
//   Y q0 q1 q2 q3                 ToEulerYPR, GetRotationMatrix(Real[9])
//   F y p r                       Rotation<float>::FromEulerYPR(y, p, r).Inverse().GetRotationMatrix(R[9]) (Quadcopter_T.cpp:78-80)
//   S cw min max kf ktau tau J px py pz ax ay az n  then n pairs "dt_us cmd"
//                                 a Simulation::Motor (cw: 1 PROP_CLOCKWISE, 0 counter-clockwise) on a ManualTimer:
//                                 per pair AdvanceMicroSeconds(dt_us), SetSpeedCommand(cmd), Run(); prints the state after
//                                 every Run() (a Run() under 1 us is Motor.cpp:41-43's early return and changes nothing)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <stdint.h>
#include "Common/Math/Rotation.hpp"
#include "Common/Time/ManualTimer.hpp"
#include "Common/Time/Timer.hpp"
#include "Components/Simulation/SimulationObject.hpp"
// Motor has no getter for its speed: its private members are read directly (nothing else of the class is changed)
#define private public
#include "Components/Simulation/Motor.hpp"
#undef private
#include "Components/Simulation/Motor.cpp"

static bool rd(double *v, int n) {
  char tok[128];
  for (int i = 0; i < n; i++) {
    if (scanf("%127s", tok) != 1) return false;
    v[i] = strtod(tok, 0);
  }
  return true;
}

static void pr(const char *key, const double *v, int n, const char *tail) {
  printf("\"%s\": [", key);
  for (int i = 0; i < n; i++) printf("%s%.17g", i ? ", " : "", v[i]);
  printf("]%s", tail);
}

int main() {
  char op[8];
  while (scanf("%7s", op) == 1) {
    double a[16];
    if (!strcmp(op, "R")) {
      if (!rd(a, 3)) return 2;
      const Rotationd q = Rotationd::FromRotationVector(Vec3d(a[0], a[1], a[2]));
      const double o[4] = {q[0], q[1], q[2], q[3]};
      printf("{\"op\": \"R\", "); pr("q", o, 4, "}\n");
    } else if (!strcmp(op, "P")) {
      if (!rd(a, 8)) return 2;
      const Rotationd att(a[0], a[1], a[2], a[3]);
      const Vec3d angVel(a[4], a[5], a[6]);
      const double dt = a[7];
      const Rotationd dq = Rotationd::FromRotationVector(angVel * dt);
      const Rotationd q = att * dq;
      const double d[4] = {dq[0], dq[1], dq[2], dq[3]}, o[4] = {q[0], q[1], q[2], q[3]};
      printf("{\"op\": \"P\", "); pr("dq", d, 4, ", "); pr("q", o, 4, "}\n");
    } else if (!strcmp(op, "M")) {
      if (!rd(a, 8)) return 2;
      const Rotationd q = Rotationd(a[0], a[1], a[2], a[3]) * Rotationd(a[4], a[5], a[6], a[7]);
      const double o[4] = {q[0], q[1], q[2], q[3]};
      printf("{\"op\": \"M\", "); pr("q", o, 4, "}\n");
    } else if (!strcmp(op, "V")) {
      if (!rd(a, 7)) return 2;
      const Rotationd q(a[0], a[1], a[2], a[3]);
      const Vec3d v(a[4], a[5], a[6]);
      const Vec3d f = q * v, b = q.Inverse() * v;
      const double fo[3] = {f.x, f.y, f.z}, bo[3] = {b.x, b.y, b.z};
      printf("{\"op\": \"V\", "); pr("fwd", fo, 3, ", "); pr("inv", bo, 3, "}\n");
    } else if (!strcmp(op, "E")) {
      if (!rd(a, 3)) return 2;
      const Rotationd q = Rotationd::FromEulerYPR(a[0], a[1], a[2]);
      const double o[4] = {q[0], q[1], q[2], q[3]};
      printf("{\"op\": \"E\", "); pr("q", o, 4, "}\n");
    } else if (!strcmp(op, "Y")) {
      if (!rd(a, 4)) return 2;
      const Rotationd q(a[0], a[1], a[2], a[3]);
      double ypr[3], R[9];
      q.ToEulerYPR(ypr[0], ypr[1], ypr[2]);
      q.GetRotationMatrix(R);
      printf("{\"op\": \"Y\", "); pr("ypr", ypr, 3, ", "); pr("R", R, 9, "}\n");
    } else if (!strcmp(op, "F")) {
      if (!rd(a, 3)) return 2;
      float Rf[9];
      Rotationf::FromEulerYPR((float) a[0], (float) a[1], (float) a[2]).Inverse().GetRotationMatrix(Rf);
      double R[9];
      for (int k = 0; k < 9; k++) R[k] = Rf[k];
      printf("{\"op\": \"F\", "); pr("R", R, 9, "}\n");
    } else if (!strcmp(op, "S")) {
      if (!rd(a, 14)) return 2;
      ManualTimer clock;
      Simulation::Motor m(&clock, Vec3d(a[7], a[8], a[9]), Vec3d(a[10], a[11], a[12]),
                          a[0] != 0 ? Simulation::Motor::PROP_CLOCKWISE : Simulation::Motor::PROP_COUNTERCLOCKWISE,
                          a[1], a[2], a[3], a[4], a[5], a[6]);
      const int n = (int) a[13];
      printf("{\"op\": \"S\", \"steps\": [");
      for (int k = 0; k < n; k++) {
        double s[2];
        if (!rd(s, 2)) return 2;
        clock.AdvanceMicroSeconds((uint64_t) s[0]);
        m.SetSpeedCommand(s[1]);
        m.Run();
        const Vec3d f = m.GetForce(), t = m.GetTorque(), L = m.GetAngularMomentum();
        const double sp[1] = {m._speed}, fo[3] = {f.x, f.y, f.z}, to[3] = {t.x, t.y, t.z}, lo[3] = {L.x, L.y, L.z};
        const double pw[1] = {m.GetPowerConsumption()};
        printf("%s{", k ? ", " : "");
        pr("speed", sp, 1, ", "); pr("thrust", fo, 3, ", "); pr("torque", to, 3, ", ");
        pr("ang_mom", lo, 3, ", "); pr("power", pw, 1, "}");
      }
      printf("]}\n");
    } else {
      fprintf(stderr, "motion_probe: unknown case '%s'\n", op);
      return 2;
    }
  }
  return 0;
}
