// afe_offboard_math.h -- the device functions the offboard consumers share: the trajectory follower (afe_follower.hip) and the
// flight stage machine (afe_stages.hip).  Internal to the library, device code, header only.  Everything here is part of both
// definitions (the ORDER of the operations is the contract, see afe_follower.hip): contraction is off in every function, + - * /
// sqrt and the conversions are correctly rounded, and the device library's own functions are reached through the fm_ / dm_
// helpers alone, which the self-tests of both consumers call as well.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace afe_offboard {

// ---- the device library's functions, through the helpers both the kernels and the self-tests call --------------------
// sine and cosine of one angle are asked for together wherever a controller needs them: the helper is the pair, so
// that a merged call cannot give the kernel other bits than the self-test
__device__ __forceinline__ void fm_sincosf(float x, float *s, float *c) { *s = sinf(x); *c = cosf(x); }
__device__ __forceinline__ float fm_asinf(float x) { return asinf(x); }
__device__ __forceinline__ float fm_acosf(float x) { return acosf(x); }
__device__ __forceinline__ double fm_acos(double x) { return acos(x); }
__device__ __forceinline__ float fm_atan2f(float y, float x) { return atan2f(y, x); }
__device__ __forceinline__ void dm_sincos(double x, double *s, double *c) { *s = sin(x); *c = cos(x); }

// ---- double ----------------------------------------------------------------------------------------------------------
struct V3 { double x, y, z; };
struct Q4 { double w, x, y, z; };
struct M9 { double m[9]; };

__device__ __forceinline__ Q4 q_mul(const Q4 &a, const Q4 &b) {          // Rotation.hpp:124-131, this = a, r1 = b
#pragma clang fp contract(off)
  Q4 c;
  c.w = b.w * a.w - b.x * a.x - b.y * a.y - b.z * a.z;
  c.x = b.x * a.w + b.w * a.x + b.z * a.y - b.y * a.z;
  c.y = b.y * a.w - b.z * a.x + b.w * a.y + b.x * a.z;
  c.z = b.z * a.w + b.y * a.x - b.x * a.y + b.w * a.z;
  return c;
}
__device__ __forceinline__ Q4 q_inv(const Q4 &q) { Q4 r; r.w = q.w; r.x = -q.x; r.y = -q.y; r.z = -q.z; return r; }
__device__ __forceinline__ M9 q_matrix(const Q4 &q) {                    // Rotation.hpp:196-220
#pragma clang fp contract(off)
  const double r0 = q.w * q.w, r1 = q.x * q.x, r2 = q.y * q.y, r3 = q.z * q.z;
  M9 R;
  R.m[0] = r0 + r1 - r2 - r3;
  R.m[1] = 2 * q.x * q.y - 2 * q.w * q.z;
  R.m[2] = 2 * q.x * q.z + 2 * q.w * q.y;
  R.m[3] = 2 * q.x * q.y + 2 * q.w * q.z;
  R.m[4] = r0 - r1 + r2 - r3;
  R.m[5] = 2 * q.y * q.z - 2 * q.w * q.x;
  R.m[6] = 2 * q.x * q.z - 2 * q.w * q.y;
  R.m[7] = 2 * q.y * q.z + 2 * q.w * q.x;
  R.m[8] = r0 - r1 - r2 + r3;
  return R;
}
__device__ __forceinline__ V3 m_rotate(const M9 &R, const V3 &v) {       // Rotation.hpp:236-245
#pragma clang fp contract(off)
  V3 o;
  o.x = R.m[0] * v.x + R.m[1] * v.y + R.m[2] * v.z;
  o.y = R.m[3] * v.x + R.m[4] * v.y + R.m[5] * v.z;
  o.z = R.m[6] * v.x + R.m[7] * v.y + R.m[8] * v.z;
  return o;
}
__device__ __forceinline__ double v_dot(const V3 &a, const V3 &b) {
#pragma clang fp contract(off)
  return a.x * b.x + a.y * b.y + a.z * b.z;
}
__device__ __forceinline__ V3 v_cross(const V3 &a, const V3 &b) {        // Vec3.hpp:106-109
#pragma clang fp contract(off)
  V3 o;
  o.x = a.y * b.z - a.z * b.y;
  o.y = a.z * b.x - a.x * b.z;
  o.z = a.x * b.y - a.y * b.x;
  return o;
}

// ---- float -------------------------------------------------------------------------------------------------------------
struct V3f { float x, y, z; };
struct Q4f { float w, x, y, z; };
struct M9f { float m[9]; };

__device__ __forceinline__ Q4f qf_mul(const Q4f &a, const Q4f &b) {
#pragma clang fp contract(off)
  Q4f c;
  c.w = b.w * a.w - b.x * a.x - b.y * a.y - b.z * a.z;
  c.x = b.x * a.w + b.w * a.x + b.z * a.y - b.y * a.z;
  c.y = b.y * a.w - b.z * a.x + b.w * a.y + b.x * a.z;
  c.z = b.z * a.w + b.y * a.x - b.x * a.y + b.w * a.z;
  return c;
}
__device__ __forceinline__ Q4f qf_inv(const Q4f &q) { Q4f r; r.w = q.w; r.x = -q.x; r.y = -q.y; r.z = -q.z; return r; }
__device__ __forceinline__ M9f qf_matrix(const Q4f &q) {
#pragma clang fp contract(off)
  const float r0 = q.w * q.w, r1 = q.x * q.x, r2 = q.y * q.y, r3 = q.z * q.z;
  M9f R;
  R.m[0] = r0 + r1 - r2 - r3;
  R.m[1] = 2 * q.x * q.y - 2 * q.w * q.z;
  R.m[2] = 2 * q.x * q.z + 2 * q.w * q.y;
  R.m[3] = 2 * q.x * q.y + 2 * q.w * q.z;
  R.m[4] = r0 - r1 + r2 - r3;
  R.m[5] = 2 * q.y * q.z - 2 * q.w * q.x;
  R.m[6] = 2 * q.x * q.z - 2 * q.w * q.y;
  R.m[7] = 2 * q.y * q.z + 2 * q.w * q.x;
  R.m[8] = r0 - r1 - r2 + r3;
  return R;
}
__device__ __forceinline__ V3f mf_rotate(const M9f &R, const V3f &v) {
#pragma clang fp contract(off)
  V3f o;
  o.x = R.m[0] * v.x + R.m[1] * v.y + R.m[2] * v.z;
  o.y = R.m[3] * v.x + R.m[4] * v.y + R.m[5] * v.z;
  o.z = R.m[6] * v.x + R.m[7] * v.y + R.m[8] * v.z;
  return o;
}
__device__ __forceinline__ float vf_dot(const V3f &a, const V3f &b) {
#pragma clang fp contract(off)
  return a.x * b.x + a.y * b.y + a.z * b.z;
}
__device__ __forceinline__ V3f vf_cross(const V3f &a, const V3f &b) {
#pragma clang fp contract(off)
  V3f o;
  o.x = a.y * b.z - a.z * b.y;
  o.y = a.z * b.x - a.x * b.z;
  o.z = a.x * b.y - a.y * b.x;
  return o;
}
// Rotation.hpp:84-97
__device__ __forceinline__ Q4f qf_from_rotvec(const V3f &r) {
#pragma clang fp contract(off)
  Q4f q;
  q.w = 1.0f; q.x = 0.0f; q.y = 0.0f; q.z = 0.0f;
  const float theta = sqrtf(vf_dot(r, r));
  if (theta < 4.84813681e-6f) return q;
  const float ux = r.x / theta, uy = r.y / theta, uz = r.z / theta;
  float s, c;
  fm_sincosf(theta * 0.5f, &s, &c);
  q.w = c; q.x = s * ux; q.y = s * uy; q.z = s * uz;
  return q;
}
// Rotation.hpp:144-161 (the norm held at 1 for asinf)
__device__ __forceinline__ V3f qf_to_rotvec(const Q4f &q) {
#pragma clang fp contract(off)
  V3f n;
  if (q.w > 0.0f) { n.x = q.x; n.y = q.y; n.z = q.z; }
  else { n.x = -q.x; n.y = -q.y; n.z = -q.z; }
  const float norm = sqrtf(vf_dot(n, n));
  const float angle = fm_asinf(norm < 1.0f ? norm : 1.0f) * 2.0f;
  V3f o;
  o.x = 0.0f; o.y = 0.0f; o.z = 0.0f;
  if (angle < 4.84813681e-6f) return o;
  const float k = angle / norm;
  o.x = n.x * k; o.y = n.y * k; o.z = n.z * k;
  return o;
}
__device__ __forceinline__ float tilt_angle(float c) {
  return c >= 1.0f ? 0.0f : c <= -1.0f ? 3.14159274f : fm_acosf(c);      // float(M_PI)
}
// `errno = 0; angle = acosf(c); if (errno) angle = c < 0 ? float(M_PI) : 0` (KalmanFilter6DOF.cpp:95-103, QuadcopterLogic.cpp:490-499):
// glibc sets EDOM for |c| > 1 alone -- a NaN argument sets nothing and passes through
__device__ __forceinline__ float guarded_acosf(float c) {
  if (c > 1.0f) return 0.0f;
  if (c < -1.0f) return 3.14159274f;                                       // float(M_PI)
  return fm_acosf(c);
}
// Rotation::FromAxisAngle, Rotation.hpp:92-97 (a unit vector is the caller's business)
__device__ __forceinline__ Q4f qf_from_axis_angle(const V3f &u, float angle) {
#pragma clang fp contract(off)
  float s, c;
  fm_sincosf(angle * 0.5f, &s, &c);
  Q4f q;
  q.w = c; q.x = s * u.x; q.y = s * u.y; q.z = s * u.z;
  return q;
}
// Rotation::FromEulerYPR, Rotation.hpp:99-110
__device__ __forceinline__ Q4f qf_from_euler_ypr(float y, float p, float r) {
#pragma clang fp contract(off)
  float sy, cy, sp, cp, sr, cr;
  fm_sincosf(0.5f * y, &sy, &cy);
  fm_sincosf(0.5f * p, &sp, &cp);
  fm_sincosf(0.5f * r, &sr, &cr);
  Q4f q;
  q.w = cy * cp * cr + sy * sp * sr;
  q.x = cy * cp * sr - sy * sp * cr;
  q.y = cy * sp * cr + sy * cp * sr;
  q.z = sy * cp * cr - cy * sp * sr;
  return q;
}
// Rotation::ToEulerYPR, Rotation.hpp:163-169
__device__ __forceinline__ void qf_to_euler_ypr(const Q4f &q, float *y, float *p, float *r) {
#pragma clang fp contract(off)
  *y = fm_atan2f(2.0f * q.x * q.y + 2.0f * q.w * q.z, q.x * q.x + q.w * q.w - q.z * q.z - q.y * q.y);
  *p = -fm_asinf(2.0f * q.x * q.z - 2.0f * q.w * q.y);
  *r = fm_atan2f(2.0f * q.y * q.z + 2.0f * q.w * q.x, q.z * q.z - q.y * q.y - q.x * q.x + q.w * q.w);
}
// EncodeOnesRange(MapToOnesRange(x, a, b)), TelemetryPacket.hpp:38-60: outside [-1, 1] is code 0; the float sum is truncated to
// 16 bits; a NaN (no comparison holds, the conversion is undefined in the reference) is code 0 here
__device__ __forceinline__ uint16_t telemetry_code(float x, float a, float b) {
#pragma clang fp contract(off)
  const float t = ((x - a) / (b - a)) * 2 - 1;
  if (t != t || t < -1 || t > 1) return 0;
  return (uint16_t)(int)(32768 + 32767 * t);
}
// encodeToRadioByte + decodeFromRadioBytes, RadioTypes.hpp:73-116, two bytes, limit 35
__device__ __forceinline__ float radio_quantise35(float v) {
#pragma clang fp contract(off)
  const float limit = 35.0f;
  int out;
  if (v > -limit && v < limit) out = int(v * 32768 / limit + 0.5f) + 32768;
  else if (v > -limit) out = 65535;
  else out = 0;
  out &= 0xffff;                                                         // two bytes on the wire
  return limit * (out - 32768) / 32768.0f;
}

// The attitude whose z axis is the unit vector `dir` (QuadcopterController.cpp:48-66 and :103-122, the same lines twice):
// identity when |e3 x dir| < 1e-6f, else FromRotationVector((e3 x dir) * (angle / n))
__device__ __forceinline__ Q4f tilt_attitude(const V3f &dir) {
#pragma clang fp contract(off)
  V3f e3;
  e3.x = 0.0f; e3.y = 0.0f; e3.z = 1.0f;
  const float angle = tilt_angle(vf_dot(dir, e3));
  const V3f ax = vf_cross(e3, dir);
  const float n = sqrtf(vf_dot(ax, ax));
  Q4f att;
  att.w = 1.0f; att.x = 0.0f; att.y = 0.0f; att.z = 0.0f;
  if (!(n < 1e-6f)) {
    const float k = angle / n;
    V3f rv3;
    rv3.x = k * ax.x; rv3.y = k * ax.y; rv3.z = k * ax.z;
    att = qf_from_rotvec(rv3);
  }
  return att;
}
// GetDesiredAngularVelocity, QuadcopterAttitudeController.hpp:35-68
__device__ __forceinline__ V3f desired_angular_velocity(const Q4f &desAtt, const Q4f &qf, float tc_xy, float tc_z) {
#pragma clang fp contract(off)
  V3f e3;
  e3.x = 0.0f; e3.y = 0.0f; e3.z = 1.0f;
  const Q4f err = qf_mul(qf_inv(desAtt), qf);
  const V3f rot = qf_to_rotvec(err);
  const V3f zb = mf_rotate(qf_matrix(qf_inv(err)), e3);
  V3f rax = vf_cross(zb, e3);
  const float an = tilt_angle(vf_dot(zb, e3));
  const float rn = sqrtf(vf_dot(rax, rax));
  if (rn < 1e-12f) { rax.x = 0.0f; rax.y = 0.0f; rax.z = 0.0f; }
  else { rax.x = rax.x / rn; rax.y = rax.y / rn; rax.z = rax.z / rn; }
  const float k3 = 1.0f / tc_z, k12 = 1.0f / tc_xy;
  const float nk3 = -k3, kr = (k12 - k3) * an;
  V3f we;
  we.x = nk3 * rot.x - kr * rax.x;
  we.y = nk3 * rot.y - kr * rax.y;
  we.z = nk3 * rot.z - kr * rax.z;
  return we;
}

// STATE READ: X = anchor_x + (double)px, Y = anchor_y + (double)py, Z = (double)pz (as afe_get_state forms them); velocity and
// attitude widened to double.  Nothing is normalised.  A: any argument block with pos, vel, att, anchor_xy and stride.
template <typename T, typename A>
__device__ __forceinline__ void load_state(const A &g, int64_t v, V3 &p, V3 &vel, Q4 &q) {
#pragma clang fp contract(off)
  const int64_t S = g.stride;
  const T *P = (const T *)g.pos, *V = (const T *)g.vel, *Q = (const T *)g.att;
  p.x = g.anchor_xy[v] + (double)P[v]; p.y = g.anchor_xy[S + v] + (double)P[S + v]; p.z = (double)P[2 * S + v];
  vel.x = (double)V[v]; vel.y = (double)V[S + v]; vel.z = (double)V[2 * S + v];
  q.w = (double)Q[v]; q.x = (double)Q[S + v]; q.y = (double)Q[2 * S + v]; q.z = (double)Q[3 * S + v];
}

}  // namespace afe_offboard
