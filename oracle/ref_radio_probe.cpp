// oracle/ref_radio_probe.cpp -- TEST INFRASTRUCTURE.
// Known answers from the REFERENCE's own radio codec, compiled from where it lies:
//   Common/Common/DataTypes/RadioTypes.hpp   (all five message kinds, encodeToRadioByte, decodeFromRadioBytes)
// The header includes Vec3.hpp and through it Matrix.hpp and <Eigen/Dense>, but does no Eigen arithmetic: it uses Vec3f
// element access alone.  The Makefile puts oracle/eigen_decl first on the include path, a header that only DECLARES
// Eigen::Matrix, so anything Eigen on a path printed here would not compile.
//
// usage: radio_probe < cases   (one case per line; floats as their IEEE-754 bit patterns in hex, so NaN and -0 travel)
//   R flags thrust wx wy wz                     CreateRatesCommand
//   P flags px py pz vx vy vz ax ay az          CreatePositionCommand
//   A flags ax ay az yawRate                    CreateAccelerationCommand
//   K flags | I flags                           CreateKillCommand | CreateIdleCommand
//   D b0 .. b22                                 decode 23 arbitrary bytes (hex)
// The reference's Create* functions leave the bytes they do not write alone: the buffer is zeroed first (as
// ref_telemetry_probe.cpp does).  One JSON object per line out: the 23 bytes as hex, and RadioMessageDecoded(raw)'s type,
// flags and the floats that kind of message carries (bit patterns; ten, but nine for a position and four for an
// acceleration command).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdint.h>
#include "Common/DataTypes/RadioTypes.hpp"

typedef RadioTypes::RadioMessageDecoded Msg;

static bool rd_float(float *v, int n) {
  for (int i = 0; i < n; i++) {
    unsigned bits;
    if (scanf("%x", &bits) != 1) return false;
    uint32_t b = bits;
    memcpy(&v[i], &b, 4);
  }
  return true;
}

int main() {
  char op[8];
  while (scanf("%7s", op) == 1) {
    uint8_t raw[Msg::RAW_PACKET_SIZE];
    memset(raw, 0, sizeof raw);
    unsigned flags = 0;
    float f[9];
    if (op[0] == 'D') {
      for (int i = 0; i < (int) Msg::RAW_PACKET_SIZE; i++) {
        unsigned b;
        if (scanf("%x", &b) != 1) return 2;
        raw[i] = (uint8_t) b;
      }
    } else if (scanf("%x", &flags) != 1) {
      return 2;
    } else if (op[0] == 'R') {
      if (!rd_float(f, 4)) return 2;
      Msg::CreateRatesCommand((uint8_t) flags, f[0], Vec3f(f[1], f[2], f[3]), raw);
    } else if (op[0] == 'P') {
      if (!rd_float(f, 9)) return 2;
      Msg::CreatePositionCommand((uint8_t) flags, Vec3f(f[0], f[1], f[2]), Vec3f(f[3], f[4], f[5]), Vec3f(f[6], f[7], f[8]), raw);
    } else if (op[0] == 'A') {
      if (!rd_float(f, 4)) return 2;
      Msg::CreateAccelerationCommand((uint8_t) flags, Vec3f(f[0], f[1], f[2]), f[3], raw);
    } else if (op[0] == 'K') {
      Msg::CreateKillCommand((uint8_t) flags, raw);
    } else if (op[0] == 'I') {
      Msg::CreateIdleCommand((uint8_t) flags, raw);
    } else {
      fprintf(stderr, "radio_probe: unknown case '%s'\n", op);
      return 2;
    }
    const Msg m(raw);
    printf("{\"raw\": \"");
    for (int i = 0; i < (int) Msg::RAW_PACKET_SIZE; i++) printf("%02x", raw[i]);
    printf("\", \"type\": %u, \"flags\": %u, \"floats\": [", m.type, m.flags);
    // the constructor leaves the fields its message kind does not carry uninitialised (:195-230): they are not printed
    const int n_set = m.type == RadioTypes::positionCommand ? 9 : m.type == RadioTypes::externalAccelerationCmd ? 4
                      : (int) Msg::NUM_RADIO_FLOAT_FIELDS;
    for (int i = 0; i < n_set; i++) {
      uint32_t b;
      memcpy(&b, &m.floats[i], 4);
      printf("%s%u", i ? ", " : "", b);
    }
    printf("]}\n");
  }
  return 0;
}
