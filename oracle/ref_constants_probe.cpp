// oracle/ref_constants_probe.cpp -- TEST INFRASTRUCTURE.
// The REFERENCE's own type constants, read from where they lie:
//   Components/Components/Logic/QuadcopterConstants.hpp   (#included below; -I oracle/eigen_store: the inertia matrix is
//                                                          storage only, as for ref_rigid_body_probe.cpp)
// This file's own text constructs Onboard::QuadcopterConstants(t) for t = 0..5 and prints its public data members, and
// calls GetVehicleTypeFromID for ids 0..31.  Nothing is computed here.
//
// usage: constants_probe > answer      (text; tests/golden/make_vehicle_constants.py)
//   "F <type> <name> <ieee-754 bits, hex> <decimal>"   a float member
//   "I <type> <name> <value>"                          an int / enum / bool member
//   "D <id> <type>"                                    GetVehicleTypeFromID(id)
// A member that the constructor leaves unset for a type is NOT printed for it (reading it would be reading an
// indeterminate value): linDragCoeffB* in the default branch (:237-266), ESCspeedToPWMConsts where the type sets the
// CF table only, CFspeedToPWMConsts where it sets the ESC pair only.
#include <cstdio>
#include <cstring>
#include <cmath>
#include <stdint.h>

#include "Components/Logic/QuadcopterConstants.hpp"

typedef Onboard::QuadcopterConstants QC;

static void F(int t, const char *name, float v) {
  uint32_t b;
  std::memcpy(&b, &v, 4);
  std::printf("F %d %s %08x %.9g\n", t, name, (unsigned)b, (double)v);
}
static void I(int t, const char *name, int v) { std::printf("I %d %s %d\n", t, name, v); }

int main() {
  for (int t = 0; t < 6; t++) {
    QC c((QC::QuadcopterType)t);
    F(t, "mass", c.mass);
    F(t, "inertia_xx", c.inertia_xx);
    F(t, "inertia_zz", c.inertia_zz);
    F(t, "armLength", c.armLength);
    F(t, "propellerThrustFromSpeedSqr", c.propellerThrustFromSpeedSqr);
    F(t, "propellerTorqueFromThrust", c.propellerTorqueFromThrust);
    F(t, "maxThrustPerPropeller", c.maxThrustPerPropeller);
    F(t, "minThrustPerPropeller", c.minThrustPerPropeller);
    F(t, "maxCmdTotalThrust", c.maxCmdTotalThrust);
    I(t, "prop0SpinDir", c.prop0SpinDir);
    if (t >= 1 && t <= 5) {   // the default branch sets no drag
      F(t, "linDragCoeffBx", c.linDragCoeffBx);
      F(t, "linDragCoeffBy", c.linDragCoeffBy);
      F(t, "linDragCoeffBz", c.linDragCoeffBz);
    }
    F(t, "motorTimeConst", c.motorTimeConst);
    F(t, "motorInertia", c.motorInertia);
    F(t, "motorMinSpeed", c.motorMinSpeed);
    F(t, "motorMaxSpeed", c.motorMaxSpeed);
    I(t, "motorType", (int)c.motorType);
    if (t <= 3) {             // INVALID, CF_STANDARD, CF_BIGMOTORSPROPS, CF_FEEDTHROUGH set the CF table
      char name[32];
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 2; j++) {
          std::snprintf(name, sizeof(name), "CFspeedToPWMConsts_%d_%d", i, j);
          F(t, name, c.CFspeedToPWMConsts[i][j]);
        }
    }
    if (t == 0 || t >= 4) {   // INVALID, CF_LARGEQUAD, CF_MINIQUAD set the ESC pair
      F(t, "ESCspeedToPWMConsts_0", c.ESCspeedToPWMConsts[0]);
      F(t, "ESCspeedToPWMConsts_1", c.ESCspeedToPWMConsts[1]);
    }
    F(t, "posControl_natFreq", c.posControl_natFreq);
    F(t, "posControl_damping", c.posControl_damping);
    F(t, "angVelControl_timeConst_xy", c.angVelControl_timeConst_xy);
    F(t, "attControl_timeConst_xy", c.attControl_timeConst_xy);
    F(t, "angVelControl_timeConst_z", c.angVelControl_timeConst_z);
    F(t, "attControl_timeConst_z", c.attControl_timeConst_z);
    F(t, "IMU_yaw", c.IMU_yaw);
    F(t, "IMU_pitch", c.IMU_pitch);
    F(t, "IMU_roll", c.IMU_roll);
    F(t, "lowBatteryThreshold", c.lowBatteryThreshold);
    I(t, "valid", c.valid ? 1 : 0);
    char name[32];
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        std::snprintf(name, sizeof(name), "inertiaMatrix_%d_%d", i, j);
        F(t, name, c.inertiaMatrix(i, j));
      }
  }
  for (unsigned id = 0; id < 32; id++) std::printf("D %u %d\n", id, (int)QC::GetVehicleTypeFromID(id));
  return 0;
}
