// afe_gps_estimator.h -- what the trajectory follower (afe_follower.hip) and the flight stage machine (afe_stages.hip) need of an attached GPS + IMU estimator
// (afe_gps_estimator.hip).  Internal to the library, host only.
#pragma once
#include <stdint.h>

#include "../../include/agrifly_engine.h"
#include "afe_estimator.h"

namespace afe {

// AFE_ERR_INVALID_ARG unless the estimator borrows this very engine; nothing else is touched
int gps_estimator_check_engine(const afe_gps_estimator *g, const afe_engine *e);
// GetCurrentEstimate() (GPSIMUStateEstimator.cpp:56-64), no prediction ahead: the estimate rows themselves, which look like
// an fp64 engine's slabs with anchors of +0.  AFE_ERR_NOT_CONFIGURED unless the estimator's last _imu consumed the sample
// of logic tick n_ticks (the engine's count now) -- the caller has passed the engine's gate.
int gps_estimator_link(afe_gps_estimator *g, uint64_t n_ticks, EstimatorLink *out);
// _lastGoodMeasUpdate for the stage machine's safety net (GetTimeSinceLastGoodMeasurement, GPSIMUStateEstimator.hpp:94-96): the
// row of last-good-update times, one uint64 per vehicle in device memory, and the afe_time_us they are relative to
int gps_estimator_last_update(afe_gps_estimator *g, const unsigned long long **t_update_us, uint64_t *origin_us);

}  // namespace afe
