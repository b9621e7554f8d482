// afe_estimator.h -- what the trajectory follower (afe_follower.hip) needs of an attached estimator (afe_estimator.hip).
// Internal to the library, host only.
#pragma once
#include <stdint.h>

#include "../../include/agrifly_engine.h"

namespace afe {

// The prediction buffer looks like the slabs of an fp64 engine standing at the origin: planar doubles with the engine's
// stride, position 3, velocity 3, attitude 4 (and body rates 3 behind them), anchors that are all +0.
struct EstimatorLink {
  const double *pos, *vel, *att, *zero_anchor_xy;
};

// AFE_ERR_INVALID_ARG unless the estimator borrows this very engine; nothing else is touched
int estimator_check_engine(const afe_estimator *est, const afe_engine *e);
// the prediction stamped at now_us (AFE_ERR_NOT_CONFIGURED if there is none) -- the caller has passed the engine's gate
int estimator_link(afe_estimator *est, uint64_t now_us, EstimatorLink *out);
// SetPredictedValues for a kernel that writes the message itself: the ring's refusals (afe_estimator_ring.h), then
// *slot = where the 6 planar doubles (acc 3, angVel 3, the engine's stride) go.  Nothing is recorded until
// estimator_announce_commit, which the caller makes once its launch went out.
int estimator_announce_begin(afe_estimator *est, uint64_t now_us, double **slot, double *from_s);
void estimator_announce_commit(afe_estimator *est, double from_s);

}  // namespace afe
