// oracle/ref_gps_probe.cpp -- TEST INFRASTRUCTURE.
// The REFERENCE's own GPS + IMU estimator, compiled from where it lies:
//   Components/Components/Offboard/GPSIMUStateEstimator.cpp   (named on the compiler's command line, oracle/Makefile)
// driven by Common/Common/Time/ManualTimer.hpp as its master clock.  -I oracle/eigen_dense and no other Eigen header: the
// recording dense stand-in, whose head says what may and what may not be concluded from the numbers printed here.
// Compiled WITHOUT -fno-math-errno: the reference's `errno = 0; acosf(c); if (errno)` (:77-98) is on the path.
//
// This file's own text is the driver: it reads a call list, makes the reference's calls with the numbers given and writes
// what the reference's members hold afterwards, with the stand-in's tape of that call.  Nothing of the estimator is
// restated here.  Private members are read and written (`#define private public`, as in the sibling probes): _cov,
// _lastMeasUpdateAttCorrection, _initialized, _numResets, the mean and both timers' reset stamps.
//
// usage: gps_probe < request > answer      (text; every double travels as a C99 hex float, so bit for bit, "nan" / "inf"
//                                           for those; tests/gps_probe.py)
//   request, one record a line:
//     C us                                   ManualTimer::ResetMicroseconds(us)
//     N id                                   new GPSIMUStateEstimator(&clock, id) under that id (the constructor's Reset)
//     L id initialized numResets tPredict_us tUpdate_us pos[3] vel[3] att[4] angVel[3] corr[3] cov[81]
//                                            members written directly (the teacher-forced recording)
//     W id pos[3] vel[3] att[4] angVel[3] corr[3] cov[81]
//                                            those members written and _initialized set; the counters and timers stay (the
//                                            script's set_state)
//     P id acc[3] gyro[3]                    Predict
//     U id pos[3]                            UpdateWithMeasurement
//     R id                                   Reset
//   answer: behind N, P, U and R one block
//     S id initialized numResets tPredict_us tUpdate_us pos[3] vel[3] att[4] angVel[3] corr[3] lastMeasAtt[4] cov[81]
//     B branch      recognised from the state before and after: constructed, reset, first_predict, predict,
//                   measure_before_predict, singular (every member the restart sets holds exactly what :230-235 sets, and
//                   _lastGoodMeasUpdate was not reset) or update
//     T kind r k c  then operands and result on one line each (A, B, O), for every tape entry of the call, in order
//     E
#include <cerrno>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <iostream>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <stdint.h>
#include <string>
#include <vector>
#include <Eigen/Dense>

#define private public
#define protected public
#include "Components/Offboard/GPSIMUStateEstimator.hpp"
#undef protected
#undef private
#include "Common/Time/ManualTimer.hpp"

typedef Offboard::GPSIMUStateEstimator Est;

static void put(const double *v, size_t n) {
  for (size_t k = 0; k < n; k++) printf(" %a", v[k]);
}

static void write_state(int id, Est &e) {
  printf("S %d %d %u %" PRIu64 " %" PRIu64, id, (int) e._initialized, e._numResets, e._estimateTimer._lastResetTime_usec,
         e._lastGoodMeasUpdate._lastResetTime_usec);
  const double m[20] = {e._pos.x, e._pos.y, e._pos.z, e._vel.x, e._vel.y, e._vel.z, e._att[0], e._att[1], e._att[2], e._att[3],
                        e._angVel.x, e._angVel.y, e._angVel.z, e._lastMeasUpdateAttCorrection.x, e._lastMeasUpdateAttCorrection.y,
                        e._lastMeasUpdateAttCorrection.z, e._lastMeasAtt[0], e._lastMeasAtt[1], e._lastMeasAtt[2], e._lastMeasAtt[3]};
  put(m, 20);
  for (int i = 0; i < 9; i++)
    for (int j = 0; j < 9; j++) printf(" %a", e._cov(i, j));
  printf("\n");
}

static void write_tape() {
  std::vector<Eigen::TapeEntry> &t = Eigen::tape();
  for (size_t n = 0; n < t.size(); n++) {
    printf("T %d %d %d %d\nA", t[n].kind, t[n].r, t[n].k, t[n].c);
    put(t[n].a.data(), t[n].a.size());
    printf("\nB");
    put(t[n].b.data(), t[n].b.size());
    printf("\nO");
    put(t[n].out.data(), t[n].out.size());
    printf("\n");
  }
  t.clear();
  printf("E\n");
}

// every member the restart of :230-235 sets holds exactly what it sets
static bool restarted_at(Est &e, const double z[3]) {
  const double want[13] = {z[0], z[1], z[2], 0, 0, 0, 1, 0, 0, 0, 0, 0, 0};
  const double got[13] = {e._pos.x, e._pos.y, e._pos.z, e._vel.x, e._vel.y, e._vel.z, e._att[0], e._att[1], e._att[2], e._att[3],
                          e._angVel.x, e._angVel.y, e._angVel.z};
  for (int k = 0; k < 13; k++)
    if (!(want[k] == got[k] || (std::isnan(want[k]) && std::isnan(got[k])))) return false;
  for (int i = 0; i < 9; i++)
    for (int j = 0; j < 9; j++)
      if (i != j && !(e._cov(i, j) == 0.0)) return false;
  return true;
}

int main() {
  ManualTimer clock;
  std::map<int, std::unique_ptr<Est> > fleet;
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string op, tok;
    in >> op;
    std::vector<double> a;
    if (op == "C") {
      uint64_t us;
      if (!(in >> us)) return 2;
      clock.ResetMicroseconds(us);
      continue;
    }
    int id;
    if (!(in >> id)) return 2;
    uint64_t head[4] = {0, 0, 0, 0};
    if (op == "L")
      for (int k = 0; k < 4; k++)
        if (!(in >> head[k])) return 2;
    while (in >> tok) a.push_back(strtod(tok.c_str(), NULL));     // strtod reads hex floats, "nan" and "inf"
    Eigen::tape().clear();
    if (op == "N") {
      if (a.size() != 0) return 2;
      fleet[id].reset(new Est(&clock, (unsigned) id));
      write_state(id, *fleet[id]);
      printf("B constructed\n");
      write_tape();
      continue;
    }
    if (!fleet.count(id)) return 2;
    Est &e = *fleet[id];
    if (op == "L" || op == "W") {
      if (a.size() != 16 + 81) return 2;
      e._initialized = op == "W" || head[0] != 0;
      if (op == "L") {
        e._numResets = (unsigned) head[1];
        e._estimateTimer._lastResetTime_usec = head[2];
        e._lastGoodMeasUpdate._lastResetTime_usec = head[3];
      }
      e._pos = Vec3d(a[0], a[1], a[2]);
      e._vel = Vec3d(a[3], a[4], a[5]);
      e._att = Rotationd(a[6], a[7], a[8], a[9]);
      e._angVel = Vec3d(a[10], a[11], a[12]);
      e._lastMeasUpdateAttCorrection = Vec3d(a[13], a[14], a[15]);
      for (int k = 0; k < 81; k++) e._cov(k / 9, k % 9) = a[16 + k];
      continue;
    }
    const bool was_initialized = e._initialized;
    const uint64_t was_update = e._lastGoodMeasUpdate._lastResetTime_usec;
    const char *branch = NULL;
    if (op == "P") {
      if (a.size() != 6) return 2;
      e.Predict(Vec3d(a[0], a[1], a[2]), Vec3d(a[3], a[4], a[5]));
      branch = was_initialized ? "predict" : "first_predict";
    } else if (op == "U") {
      if (a.size() != 3) return 2;
      e.UpdateWithMeasurement(Vec3d(a[0], a[1], a[2]));
      if (!was_initialized) branch = "measure_before_predict";
      else branch = restarted_at(e, a.data()) && e._lastGoodMeasUpdate._lastResetTime_usec == was_update ? "singular" : "update";
    } else if (op == "R") {
      if (a.size() != 0) return 2;
      e.Reset();
      branch = "reset";
    } else {
      return 2;
    }
    write_state(id, e);
    printf("B %s\n", branch);
    write_tape();
  }
  return fflush(stdout) == 0 ? 0 : 1;
}
