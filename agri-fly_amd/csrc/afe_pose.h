// afe_pose.h -- vehicle -> camera pose on the device: the one statement of the arithmetic behind afe_camera_pose_kernel
// (afe_render.hip) and the path audit of afe_clearance_plans_engine (afe_clearance.hip).  IEEE double, contraction off, the
// order below is the contract: tests/path_checker.py camera_pose and the camera's CPU checker restate it independently,
// and every image and every record is compared with them bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace afe {

// Origin o[3] and row-major camera-to-world matrix R[9] of vehicle v.  pos / att: the engine's slabs (or an upload shaped
// like them), planar, `stride` elements between components, elem_size 4 or 8; anchor_xy: x and y are relative to it
// (afe_device_view::pos_anchor_xy), NULL: absolute; mount[4]: the camera's attitude in the body frame.
__device__ __forceinline__ void camera_pose(const void *pos, const void *att, const double *anchor_xy, int64_t stride, int elem_size,
                                            const double *mount, int64_t v, double *o, double *R) {
#pragma clang fp contract(off)
  double p[3], q[4];
  if (elem_size == 8) {
    const double *P = (const double *)pos, *Q = (const double *)att;
    for (int k = 0; k < 3; k++) p[k] = P[k * stride + v];
    for (int k = 0; k < 4; k++) q[k] = Q[k * stride + v];
  } else {
    const float *P = (const float *)pos, *Q = (const float *)att;
    for (int k = 0; k < 3; k++) p[k] = (double)P[k * stride + v];
    for (int k = 0; k < 4; k++) q[k] = (double)Q[k * stride + v];
  }
  if (anchor_xy) { p[0] = anchor_xy[v] + p[0]; p[1] = anchor_xy[stride + v] + p[1]; }
  const double *m = mount;
  // att * mount, Rotation.hpp:124-131
  const double c0 = m[0] * q[0] - m[1] * q[1] - m[2] * q[2] - m[3] * q[3];
  const double c1 = m[1] * q[0] + m[0] * q[1] + m[3] * q[2] - m[2] * q[3];
  const double c2 = m[2] * q[0] - m[3] * q[1] + m[0] * q[2] + m[1] * q[3];
  const double c3 = m[3] * q[0] + m[2] * q[1] - m[1] * q[2] + m[0] * q[3];
  const double r0 = c0 * c0, r1 = c1 * c1, r2 = c2 * c2, r3 = c3 * c3;
  o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
  // Rotation.hpp:196-220
  R[0] = r0 + r1 - r2 - r3;
  R[1] = 2 * c1 * c2 - 2 * c0 * c3;
  R[2] = 2 * c1 * c3 + 2 * c0 * c2;
  R[3] = 2 * c1 * c2 + 2 * c0 * c3;
  R[4] = r0 - r1 + r2 - r3;
  R[5] = 2 * c2 * c3 - 2 * c0 * c1;
  R[6] = 2 * c1 * c3 - 2 * c0 * c2;
  R[7] = 2 * c2 * c3 + 2 * c0 * c1;
  R[8] = r0 - r1 - r2 + r3;
}

}  // namespace afe
