// afe_estimator_ring.h -- the host side of the estimator's command ring (afe_estimator.hip): activation times, the slot
// count and the two refusals.  Internal to the library, host only, header only, free of HIP, so that a plain program can
// exercise it (tests/test_estimator_cpu.py compiles one under the address and undefined-behaviour sanitizers).
//
// THE RING.  PredictionPipe (PredictionPipe.hpp:25-68) is a deque per vehicle; every vehicle is announced to in the same
// call, so the activation times are one list for the whole ensemble and message k lives in slot k % slots.  The ring
// replaces ClearExpiredMessages: a message that a newer one has superseded at a vehicle's validAt is never looked at again
// (Active scans newest first and nothing asks before validAt), so dropping it late or never is unobservable.  What IS
// observable is losing a message some vehicle still needs.  THE RULE:
//
//   need    the earliest time a vehicle's validAt can stand at.  A vehicle that propagates in measure call c ends at T_c;
//           one that is reset in call c (ten rejections) initialises in call c + 1 WITHOUT moving its validAt and propagates
//           from T_c in call c + 2.  So after measure call c: need = T_(c-1), the time of the call BEFORE the last one; and a
//           host reset at time R (creation is one, R = 0) holds need down to R until two measure calls have passed.
//   announce (activation time `from`) is refused with AFE_ERR_OUT_OF_RANGE
//           (a) unless from is strictly later than the newest message's (two equal times give the reference a step of 0 s
//               that it repeats for ever), and
//           (b) when the ring is full, unless the successor of the message it would overwrite was active a full tick (1 us)
//               before need:  from[successor] <= need - 1e-6.
//   slots   (delay_us + 2 * max_measure_gap_us) / period_us + 3: with announces one period apart and measure calls at most
//           max_measure_gap_us apart, (b) never refuses.  More than 16 is refused at create.
#pragma once
#include <stdint.h>

namespace afe {

constexpr int kEstimatorMaxSlots = 16;
constexpr double kEstimatorTick = 1e-6;

// 0: refused (period 0, or more than 16 slots)
inline int estimator_ring_slots(uint64_t delay_us, uint64_t period_us, uint64_t max_gap_us) {
  if (period_us == 0) return 0;
  if (max_gap_us > (uint64_t(1) << 40) || delay_us > (uint64_t(1) << 40)) return 0;
  const uint64_t k = (delay_us + 2 * max_gap_us) / period_us + 3;
  return k > (uint64_t)kEstimatorMaxSlots ? 0 : (int)k;
}

struct EstimatorRing {
  int slots = 0;
  uint64_t seq = 0;                       // messages announced so far; message k lives in slot k % slots
  double from[kEstimatorMaxSlots] = {};   // activation time [s] of the message in each slot
  // what `need` is made of (all in us since creation)
  uint64_t t_last = 0, t_prev = 0;        // the last measure call and the one before it
  bool reset_pending = true;              // creation is a reset at 0
  uint64_t reset_floor = 0;
  int calls_since_reset = 0;

  uint64_t need_us() const { return reset_pending && reset_floor < t_prev ? reset_floor : t_prev; }
  void measured(uint64_t t_us) {
    t_prev = t_last;
    t_last = t_us;
    if (reset_pending && ++calls_since_reset >= 2) reset_pending = false;
  }
  void was_reset(uint64_t t_us) {
    if (!reset_pending) reset_floor = t_us;    // (an older pending reset keeps its earlier floor)
    reset_pending = true;
    calls_since_reset = 0;
  }
  // true: the message may be announced
  bool accepts(double from_s) const {
    if (seq > 0 && !(from_s > from[(seq - 1) % (uint64_t)slots])) return false;
    if (seq >= (uint64_t)slots) {
      const double successor = from[(seq - (uint64_t)slots + 1) % (uint64_t)slots];
      if (!(successor <= (double)need_us() * 1e-6 - kEstimatorTick)) return false;
    }
    return true;
  }
  int write_slot() const { return (int)(seq % (uint64_t)slots); }
  void push(double from_s) { from[write_slot()] = from_s; seq++; }
  int n_messages() const { return seq < (uint64_t)slots ? (int)seq : slots; }
  int newest_slot() const { return (int)((seq + (uint64_t)slots - 1) % (uint64_t)slots); }
};

}  // namespace afe
