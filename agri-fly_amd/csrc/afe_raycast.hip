// afe_raycast.hip -- what one arbitrary ray hits first in the clearance map's mesh, and how far away: explicit rays, line of
// sight between two points, and range sensors (time-of-flight beams) mounted on every vehicle of an engine.  The C ABI is in
// include/agrifly_engine.h ("range beams").  The map, its tree and its records are afe_clearance.hip's (afe_clearance_map.h).
//
// THE DEFINITION (tests/raycast_checker.py restates it in numpy float64, operation for operation; kernel and checker must
// give the same bits, so the ORDER of the operations below is part of the contract).  Everything is IEEE double with
// contraction off; only + - * /, fabs, fmax and comparisons appear.
//
//   dot(u, v)   = u.x*v.x + u.y*v.y + u.z*v.z                                          (left to right)
//   cross(u, v) = (u.y*v.z - u.z*v.y,  u.z*v.x - u.x*v.z,  u.x*v.y - u.y*v.x)
//   |u|_1       = (|u.x| + |u.y|) + |u.z|
//
//   ONE RAY (origin o, direction d, neither normalised) against ONE TRIANGLE: the depth camera's closed, watertight rule
//   (afe_render.hip and its CPU checker's ray_triangle), operation for operation.
//        v0 = (double)first vertex,  e1 = (double)v1 - v0,  e2 = (double)v2 - v0      (the a, ab, ac the map stores)
//        p = cross(d, e2);  det = dot(e1, p);  tv = o - v0
//        en = fmax(|e1|_1, |e2|_1);  dn = |d|_1
//        eps = (dn * (2^-48 * en)) * (|tv|_1 + en);  cut = fmax(1, 32768 * en)
//        miss unless |det| > eps * cut
//        s = det > 0 ? 1 : -1
//        nu = dot(tv, p) * s;   miss if nu < -eps
//        q = cross(tv, e1);  nv = dot(d, q) * s;   miss if nv < -eps
//        miss if (|det| - nu) - nv < -eps
//        t = dot(e2, q) * (1 / det);   a hit iff t > 0 and t < +inf   (an overflowed t is the camera's "nothing" as well)
//   The map's `degenerate` flag is not consulted: a collinear triangle fails the det test by the rule itself.
//
//   WINNER over the triangles: only hits with t <= t_max count (t_max = +inf: no limit); the smallest t wins; among
//   bitwise-equal t the lowest index in the order given to afe_clearance_map_create (a ray along a shared edge ties all
//   the time).  The answer is (t, tri); no hit: (+inf, -1).  A ray with a non-finite component in o or d: the same, without
//   a walk.  d = 0 hits nothing by the rule (eps = 0, det = 0).
//
//   LINE OF SIGHT from p0 to p1:  d = p1 - p0 per axis;  blocked = 1 iff the first-hit query with o = p0, t_max = 1 has a
//   hit, else 0.  A non-finite end gives 0.
//
//   RANGE SENSOR: a mount quaternion and n_beams beams {off[3], dir[3], t_max, frame}, 1 <= n_beams <= 32.  The vehicle's
//   origin o_v and matrix R are afe::camera_pose's (afe_pose.h), unchanged: anchors added in double, fp32 or fp64 slabs.
//        frame 0 (sensor frame):  w.x = o_v.x + ((R0*off.x + R1*off.y) + R2*off.z),  rows 1 and 2 for y and z
//                                 d.x = (R0*dir.x + R1*dir.y) + R2*dir.z,            likewise
//        frame 1 (world frame):   w = o_v + off per axis,  d = dir
//   then the first-hit query with the beam's t_max.  t is the ray PARAMETER: metres when |dir|_2 = 1 and the quaternions
//   are unit; R is not normalised, as in the camera's contract.
//
// THE WALK.  One ray per lane, 256-thread blocks, clr_walk's shape: the explicit stack in LDS as [level][lane]
// (32 x 256 x 4 B = 32 KB per block, a lane only ever touches its own column), a node record as two dwordx4 per child, a
// triangle's first 32 bytes (box, index) decide whether its double-precision part is fetched, the triangles kept out of the
// tree first, brute force (a downward beam gets its bound from the ground before it walks), then the tree, the child with the
// smaller entry parameter first.  A lane whose ray misses the root's box, or is non-finite, never enters the loop.
//
// NO OUTPUT BIT DEPENDS ON THE BOXES.  The map's boxes are the exact float32 bounds of the triangles, but the rule accepts
// rays that pass up to 2^-12 m OUTSIDE a triangle (the camera checker's comment: 6 en eps / |det| < 6 / 32768), and the computed t is
// not the exact one.  What a skipped box could have held:
//   (1) t's error.  t = N / det with |det| > eps * cut = 2^-48 dn en (|tv|_1 + en) max(1, 2^15 en).  N = dot(e2, q) and det
//       carry at most 16 roundings each on terms bounded by en^2 |tv|_1 and dn en^2: |dN| <= 2^-49 en^2 |tv|_1,
//       |d det| <= 2^-49 dn en^2.  So |dN / det| <= (en / max(1, 2^15 en)) / (2 dn) <= 2^-16 / dn, and
//       |d det / det| <= 2^-16 / (|tv|_1 + en).  The exact hit lies within delta = 6 en / cut <= min(6 en, 2^-12) of the
//       triangle, so |t| dn = |t d|_1 <= |tv|_1 + en + 3 delta <= 19 (|tv|_1 + en), and |t| |d det / det| <= 19 * 2^-16 / dn.
//       With the reciprocal's and the product's own roundings  |t_computed - t_exact| < 2^-11 / dn,  which moves the point
//       o + t d by less than 2^-11 m along every axis (|d_k| <= dn).
//   (2) So for every accepted (t, triangle) the EXACT point o + t d, t the computed parameter, lies in the triangle's box
//       grown by 2^-12 + 2^-11 < 2^-10 m per axis -- and therefore in every node box above it grown likewise.
//   (3) THE MARGIN.  The slab test runs in double against boxes grown per axis k by
//           m_k = 2^-9 + 2^-40 * (max(|scene_lo_k|, |scene_hi_k|) + |o_k|)
//       folded into the ray once:  a_k = ((double)lo_k - (o_k + m_k)) * (1 / d_k),  b_k = ((double)hi_k - (o_k - m_k)) * (1 / d_k).
//       The two numerators carry two roundings at the scale of the coordinates, at most 2^-51 (|box_k| + |o_k| + m_k) -- far
//       below m_k - 2^-10 -- so the computed numerators lie strictly OUTSIDE those of the 2^-10 box of (2), whichever way
//       they round.  The reciprocal and the product add a relative 3 * 2^-53.  Hence, with near_k = min(a_k, b_k),
//       far_k = max(a_k, b_k), enter = max(near_x, near_y, near_z, 0), exit = min(far_x, far_y, far_z), every t of (2)
//       satisfies   enter <= t (1 + 2^-51)   and   exit >= t (1 - 2^-51).
//   (4) THE SLACK.  A box (node or triangle) is skipped only if   enter * (1 - 2^-40) > exit   or   enter * (1 - 2^-40) > best,
//       best = the smallest t accepted so far (initially t_max).  By (3) the first cannot happen to a box that holds an
//       accepted point, and the second only if t > best strictly: a skipped triangle could neither win nor TIE, so the
//       lowest index among equal t is never lost.  A relative slack suffices because t > 0 bounds its own error (unlike
//       the distance queries, where best can be 0); 2^-40 is two thousand times the 2^-51 of (3).
//   (5) d_k = +-0:  1 / d_k = +-inf.  A numerator of either sign gives a = -+inf: the axis drops out (near = -inf, far = +inf)
//       when o_k lies inside the grown slab, and makes enter = +inf or exit = -inf (skip, correctly: the ray never reaches
//       the slab) when it lies outside.  A numerator of exactly 0 gives 0 * inf = NaN: then near_k = -inf, far_k = +inf
//       (visit).  Every comparison is written so that a NaN reads "visit".
// Visiting more never changes a bit: every visited triangle runs the full rule, and the winner is order-independent
// (smallest t, then lowest index).  The any-hit instantiation (line of sight) stops at the first accepted triangle: "has
// a hit with t <= 1" does not depend on which.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "afe_clearance_map.h"
#include "afe_consumer.h"
#include "afe_pose.h"

namespace {

using afe::DevBuf;
using afe::EngineAccess;
using afe::StreamTimer;
using namespace afe::clr;   // the map's records and constants

constexpr int kMaxBeams = 32;
enum RaySource { kExplicit = 0, kSegment = 1, kEngine = 2 };

struct RayArgs {
  // the map (ClrArgs' tree part)
  const CNode *nodes;
  const CTri *tris;
  uint32_t root_ref, big_first, n_big;
  float root_lo[3], root_hi[3];
  double scene_lo[3], scene_hi[3];
  int64_t base, count;        // this launch answers rays [base, base + count) of `total`
  int64_t total;              // explicit: planar stride of a / b; engine: n_beams * n_vehicles_in_range
  // kExplicit: a = origin, b = dir, t_max [total] or NULL.  kSegment: a = p0, b = p1 (d = b - a, t_max = 1).
  const double *a, *b, *t_max;
  // kEngine: ray i is beam i / n_veh of vehicle first + i % n_veh (beam-major: neighbouring lanes read neighbouring slab elements)
  const void *pos, *att;
  const double *anchor_xy;
  int64_t stride, first, n_veh;
  int elem_size;
  double mount[4];
  const afe_range_beam *beams;   // device table
  // outputs, indexed by the ray (any may be NULL)
  double *t_out;
  int32_t *tri_out;
  uint8_t *blocked_out;
  unsigned long long *stats;     // counting build: [0] nodes visited, [1] triangle box tests, [2] fp64 ray/triangle tests
};

struct Ray {
  double ox, oy, oz, dx, dy, dz, dn;
  double ix, iy, iz;                  // 1 / d
  double lx, ly, lz, hx, hy, hz;      // o + m, o - m: what the boxes' lower and upper faces are measured from
};

struct RBest {
  double t;
  int32_t idx;
};

__device__ __forceinline__ double ray_dot(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
  return ax * bx + ay * by + az * bz;
}

// the definition (file header), one triangle against one ray; updates the winner
__device__ __forceinline__ void ray_eval(const CTri *T, int32_t index, const Ray &r, RBest &b) {
#pragma clang fp contract(off)
  const double v0x = T->a[0], v0y = T->a[1], v0z = T->a[2];
  const double e1x = T->ab[0], e1y = T->ab[1], e1z = T->ab[2];
  const double e2x = T->ac[0], e2y = T->ac[1], e2z = T->ac[2];
  const double px = r.dy * e2z - r.dz * e2y, py = r.dz * e2x - r.dx * e2z, pz = r.dx * e2y - r.dy * e2x;
  const double det = ray_dot(e1x, e1y, e1z, px, py, pz);
  const double tvx = r.ox - v0x, tvy = r.oy - v0y, tvz = r.oz - v0z;
  const double en = fmax(fabs(e1x) + fabs(e1y) + fabs(e1z), fabs(e2x) + fabs(e2y) + fabs(e2z));
  const double k1 = 0x1p-48 * en, cut = fmax(1.0, 32768.0 * en);
  const double tn = fabs(tvx) + fabs(tvy) + fabs(tvz);
  const double eps = (r.dn * k1) * (tn + en);
  if (!(fabs(det) > eps * cut)) return;
  const double s = det > 0.0 ? 1.0 : -1.0;
  const double nu = ray_dot(tvx, tvy, tvz, px, py, pz) * s;
  if (nu < -eps) return;
  const double qx = tvy * e1z - tvz * e1y, qy = tvz * e1x - tvx * e1z, qz = tvx * e1y - tvy * e1x;
  const double nv = ray_dot(r.dx, r.dy, r.dz, qx, qy, qz) * s;
  if (nv < -eps) return;
  if ((fabs(det) - nu) - nv < -eps) return;
  const double inv = 1.0 / det;
  const double t = ray_dot(e2x, e2y, e2z, qx, qy, qz) * inv;
  if (t > 0.0 && t < std::numeric_limits<double>::infinity() && (t < b.t || (t == b.t && index < b.idx))) {
    b.t = t;
    b.idx = index;
  }
}

// one axis of the slab test against the grown box (file header (3), (5)): near and far parameter; NaN reads "no constraint"
__device__ __forceinline__ void ray_axis(float lo, float hi, double from_lo, double from_hi, double inv, double &near, double &far) {
#pragma clang fp contract(off)
  const double a = ((double)lo - from_lo) * inv, b = ((double)hi - from_hi) * inv;
  const bool ordered = (a == a) && (b == b);
  near = ordered ? (a < b ? a : b) : -std::numeric_limits<double>::infinity();
  far = ordered ? (a < b ? b : a) : std::numeric_limits<double>::infinity();
}

// entry parameter of the ray into the grown box, already times (1 - 2^-40); `exit` its exit parameter
__device__ __forceinline__ double ray_box(float lox, float loy, float loz, float hix, float hiy, float hiz, const Ray &r, double &exit) {
#pragma clang fp contract(off)
  double nx, ny, nz, fx, fy, fz;
  ray_axis(lox, hix, r.lx, r.hx, r.ix, nx, fx);
  ray_axis(loy, hiy, r.ly, r.hy, r.iy, ny, fy);
  ray_axis(loz, hiz, r.lz, r.hz, r.iz, nz, fz);
  double enter = 0.0;
  enter = nx > enter ? nx : enter;
  enter = ny > enter ? ny : enter;
  enter = nz > enter ? nz : enter;
  exit = fx;
  exit = fy < exit ? fy : exit;
  exit = fz < exit ? fz : exit;
  return enter * (1.0 - 0x1p-40);
}

// "may only err towards visiting": false for NaN
__device__ __forceinline__ bool ray_skip(double enter, double exit, double best) { return enter > exit || enter > best; }

// box of the triangle first (32 B), the double-precision part only if the ray could meet the grown box at or before the bound
template <bool COUNT>
__device__ __forceinline__ void ray_test(const CTri *T, const Ray &r, RBest &b, unsigned &n_box, unsigned &n_eval) {
  const float4 *head = reinterpret_cast<const float4 *>(T);
  const float4 h0 = head[0], h1 = head[1];        // lo.xyz hi.x | hi.yz index degenerate
  if (COUNT) n_box++;
  double exit;
  const double enter = ray_box(h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, r, exit);
  if (ray_skip(enter, exit, b.t)) return;
  if (COUNT) n_eval++;
  ray_eval(T, __float_as_int(h1.z), r, b);
}

// The walk for one finite ray, starting from the bound in b.  ANY: returns at the first accepted triangle.
template <bool ANY, bool COUNT>
__device__ __forceinline__ void ray_walk(const RayArgs &g, const Ray &r, RBest &b, uint32_t (*stack)[kBlock], int col, unsigned &n_nodes,
                                         unsigned &n_box, unsigned &n_eval) {
  for (uint32_t k = 0; k < g.n_big; k++) {
    ray_test<COUNT>(g.tris + g.big_first + k, r, b, n_box, n_eval);
    if (ANY && b.idx != 0x7fffffff) return;
  }
  uint32_t cur = g.root_ref;
  if (cur != kNone) {
    double exit;
    const double enter = ray_box(g.root_lo[0], g.root_lo[1], g.root_lo[2], g.root_hi[0], g.root_hi[1], g.root_hi[2], r, exit);
    if (ray_skip(enter, exit, b.t)) cur = kNone;
  }
  int sp = 0;
  while (cur != kNone) {                 // bounded: every node is entered at most once
    if (cur & kLeafBit) {
      const uint32_t first = cur & kFirstMask, cnt = (cur >> 28) & 7u;
      for (uint32_t k = 0; k < cnt; k++) ray_test<COUNT>(g.tris + first + k, r, b, n_box, n_eval);
      if (ANY && b.idx != 0x7fffffff) return;
      cur = kNone;
    } else {
      if (COUNT) n_nodes++;
      const float4 *rec = reinterpret_cast<const float4 *>(g.nodes + cur);
      const float4 lo0 = rec[0], hi0 = rec[1], lo1 = rec[2], hi1 = rec[3];
      double exit0, exit1;
      const double enter0 = ray_box(lo0.x, lo0.y, lo0.z, hi0.x, hi0.y, hi0.z, r, exit0);
      const double enter1 = ray_box(lo1.x, lo1.y, lo1.z, hi1.x, hi1.y, hi1.z, r, exit1);
      const bool go0 = !ray_skip(enter0, exit0, b.t), go1 = !ray_skip(enter1, exit1, b.t);
      const uint32_t ref0 = (uint32_t)__float_as_int(lo0.w), ref1 = (uint32_t)__float_as_int(lo1.w);
      if (go0 && go1) {
        const bool near0 = enter0 <= enter1;
        if (sp < kStack) stack[sp++][col] = near0 ? ref1 : ref0;    // (the builder keeps the depth below kStack)
        cur = near0 ? ref0 : ref1;
        continue;
      }
      cur = go0 ? ref0 : (go1 ? ref1 : kNone);
      if (cur != kNone) continue;
    }
    if (sp > 0) cur = stack[--sp][col];
  }
}

template <int SRC, bool ANY, bool COUNT>
__global__ void __launch_bounds__(kBlock) afe_raycast_kernel(RayArgs g) {
#pragma clang fp contract(off)
  __shared__ uint32_t stack[kStack][kBlock];
  const int lane = threadIdx.x;
  const int64_t j = (int64_t)blockIdx.x * kBlock + lane;
  const bool valid = j < g.count;
  const int64_t i = g.base + j;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  Ray r;
  r.ox = nan; r.oy = nan; r.oz = nan; r.dx = nan; r.dy = nan; r.dz = nan;
  double t_max = inf;
  if (valid) {
    if (SRC == kExplicit) {
      r.ox = g.a[i]; r.oy = g.a[g.total + i]; r.oz = g.a[2 * g.total + i];
      r.dx = g.b[i]; r.dy = g.b[g.total + i]; r.dz = g.b[2 * g.total + i];
      if (g.t_max) t_max = g.t_max[i];
    } else if (SRC == kSegment) {
      r.ox = g.a[i]; r.oy = g.a[g.total + i]; r.oz = g.a[2 * g.total + i];
      r.dx = g.b[i] - r.ox; r.dy = g.b[g.total + i] - r.oy; r.dz = g.b[2 * g.total + i] - r.oz;
      t_max = 1.0;
    } else {
      const int64_t beam = i / g.n_veh, v = g.first + (i - beam * g.n_veh);
      double o[3], R[9];
      afe::camera_pose(g.pos, g.att, g.anchor_xy, g.stride, g.elem_size, g.mount, v, o, R);
      const afe_range_beam *B = g.beams + beam;
      const double fx = B->off[0], fy = B->off[1], fz = B->off[2];
      const double ex = B->dir[0], ey = B->dir[1], ez = B->dir[2];
      t_max = B->t_max;
      if (B->frame == 0) {
        r.ox = o[0] + ((R[0] * fx + R[1] * fy) + R[2] * fz);
        r.oy = o[1] + ((R[3] * fx + R[4] * fy) + R[5] * fz);
        r.oz = o[2] + ((R[6] * fx + R[7] * fy) + R[8] * fz);
        r.dx = (R[0] * ex + R[1] * ey) + R[2] * ez;
        r.dy = (R[3] * ex + R[4] * ey) + R[5] * ez;
        r.dz = (R[6] * ex + R[7] * ey) + R[8] * ez;
      } else {
        r.ox = o[0] + fx; r.oy = o[1] + fy; r.oz = o[2] + fz;
        r.dx = ex; r.dy = ey; r.dz = ez;
      }
    }
  }
  RBest b;
  b.t = t_max; b.idx = 0x7fffffff;
  unsigned n_nodes = 0, n_box = 0, n_eval = 0;
  if (valid && __builtin_isfinite(r.ox) && __builtin_isfinite(r.oy) && __builtin_isfinite(r.oz) && __builtin_isfinite(r.dx) &&
      __builtin_isfinite(r.dy) && __builtin_isfinite(r.dz)) {
    r.dn = fabs(r.dx) + fabs(r.dy) + fabs(r.dz);
    r.ix = 1.0 / r.dx; r.iy = 1.0 / r.dy; r.iz = 1.0 / r.dz;
    const double mx = 0x1p-9 + 0x1p-40 * (fmax(fabs(g.scene_lo[0]), fabs(g.scene_hi[0])) + fabs(r.ox));
    const double my = 0x1p-9 + 0x1p-40 * (fmax(fabs(g.scene_lo[1]), fabs(g.scene_hi[1])) + fabs(r.oy));
    const double mz = 0x1p-9 + 0x1p-40 * (fmax(fabs(g.scene_lo[2]), fabs(g.scene_hi[2])) + fabs(r.oz));
    r.lx = r.ox + mx; r.ly = r.oy + my; r.lz = r.oz + mz;
    r.hx = r.ox - mx; r.hy = r.oy - my; r.hz = r.oz - mz;
    ray_walk<ANY, COUNT>(g, r, b, stack, lane, n_nodes, n_box, n_eval);
  }
  const bool found = b.idx != 0x7fffffff;
  if (valid) {
    if (g.t_out) g.t_out[i] = found ? b.t : inf;
    if (g.tri_out) g.tri_out[i] = found ? b.idx : -1;
    if (g.blocked_out) g.blocked_out[i] = found ? 1 : 0;
  }
  if (COUNT && valid) {
    atomicAdd(g.stats + 0, (unsigned long long)n_nodes);
    atomicAdd(g.stats + 1, (unsigned long long)n_box);
    atomicAdd(g.stats + 2, (unsigned long long)n_eval);
  }
}

// g.total rays on `stream`, in runs below 2^31 threads
template <int SRC, bool ANY, bool COUNT>
int launch_rays(RayArgs g, int64_t n_rays, hipStream_t stream, float *kernel_ms) {
  StreamTimer timer(stream, kernel_ms != nullptr);
  if (!timer.ok()) return AFE_ERR_HIP;
  int rc = AFE_OK;
  for (int64_t done = 0; done < n_rays && rc == AFE_OK; done += kPointsPerLaunch) {
    const int64_t n = std::min(n_rays - done, kPointsPerLaunch);
    g.base = done;
    g.count = n;
    hipLaunchKernelGGL((afe_raycast_kernel<SRC, ANY, COUNT>), dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, g);
    rc = hipGetLastError() == hipSuccess ? AFE_OK : AFE_ERR_HIP;
  }
  return timer.finish(rc, kernel_ms);
}

RayArgs map_args(const afe_clearance_map *m) {
  RayArgs g;
  std::memset(&g, 0, sizeof(g));
  const ClrArgs &c = m->base;
  g.nodes = c.nodes; g.tris = c.tris;
  g.root_ref = c.root_ref; g.big_first = c.big_first; g.n_big = c.n_big;
  for (int k = 0; k < 3; k++) {
    g.root_lo[k] = c.root_lo[k]; g.root_hi[k] = c.root_hi[k];
    g.scene_lo[k] = c.scene_lo[k]; g.scene_hi[k] = c.scene_hi[k];
  }
  return g;
}

bool t_max_ok(double t_max) { return t_max >= 0.0; }   // false for NaN and negatives; +inf passes

int cast_rays(afe_clearance_map *m, int64_t n_rays, const double *origin, const double *dir, const double *t_max, double *t_out, int32_t *tri_out,
              float *kernel_ms, uint64_t *stats) {
  if (hipSetDevice(m->device) != hipSuccess) return AFE_ERR_HIP;
  const size_t n = (size_t)n_rays;
  DevBuf d_o, d_d, d_tmax, d_t, d_tri, d_stats;
  if (!d_o.upload(origin, n * 24) || !d_d.upload(dir, n * 24) || (t_max && !d_tmax.upload(t_max, n * 8)) || !d_t.alloc(n * 8) || !d_tri.alloc(n * 4) ||
      (stats && !d_stats.alloc(24))) {
    (void)hipGetLastError();
    return AFE_ERR_HIP;
  }
  if (stats && hipMemset(d_stats.get(), 0, 24) != hipSuccess) return AFE_ERR_HIP;
  RayArgs g = map_args(m);
  g.total = n_rays;
  g.a = d_o.as<double>(); g.b = d_d.as<double>(); g.t_max = d_tmax.as<double>();
  g.t_out = d_t.as<double>(); g.tri_out = d_tri.as<int32_t>();
  g.stats = (unsigned long long *)d_stats.get();
  float ms = 0;
  const int rc = stats ? launch_rays<kExplicit, false, true>(g, n_rays, nullptr, &ms) : launch_rays<kExplicit, false, false>(g, n_rays, nullptr, &ms);
  if (rc != AFE_OK) return rc;
  if (kernel_ms) *kernel_ms = ms;
  if ((t_out && !d_t.download(t_out, n * 8)) || (tri_out && !d_tri.download(tri_out, n * 4))) return AFE_ERR_HIP;
  if (stats) {
    unsigned long long host[3];
    if (!d_stats.download(host, 24)) return AFE_ERR_HIP;
    for (int k = 0; k < 3; k++) stats[k] = host[k];
    stats[3] = (uint64_t)n_rays;
  }
  return AFE_OK;
}

bool t_max_array_bad(const double *t_max, int64_t n) {
  if (!t_max) return false;
  for (int64_t i = 0; i < n; i++) if (!t_max_ok(t_max[i])) return true;
  return false;
}

}  // namespace

extern "C" int afe_raycast(afe_clearance_map *m, int64_t n, const double *origin, const double *dir, const double *t_max, double *t_out,
                           int32_t *tri_out, float *kernel_ms) {
  if (!m || n < 0 || !origin || !dir || !t_out || !tri_out) return AFE_ERR_INVALID_ARG;
  if (n > kMaxPoints || t_max_array_bad(t_max, n)) return AFE_ERR_OUT_OF_RANGE;
  if (n == 0) return AFE_OK;
  return cast_rays(m, n, origin, dir, t_max, t_out, tri_out, kernel_ms, nullptr);
}

extern "C" int afe_raycast_stats(afe_clearance_map *m, int64_t n, const double *origin, const double *dir, const double *t_max, double *t_out,
                                 int32_t *tri_out, uint64_t stats[4], float *kernel_ms) {
  if (!m || n <= 0 || !origin || !dir || !stats) return AFE_ERR_INVALID_ARG;
  if (n > kMaxPoints || t_max_array_bad(t_max, n)) return AFE_ERR_OUT_OF_RANGE;
  return cast_rays(m, n, origin, dir, t_max, t_out, tri_out, kernel_ms, stats);
}

extern "C" int afe_line_of_sight(afe_clearance_map *m, int64_t n, const double *p0, const double *p1, uint8_t *blocked, float *kernel_ms) {
  if (!m || n < 0 || !p0 || !p1 || !blocked) return AFE_ERR_INVALID_ARG;
  if (n > kMaxPoints) return AFE_ERR_OUT_OF_RANGE;
  if (n == 0) return AFE_OK;
  if (hipSetDevice(m->device) != hipSuccess) return AFE_ERR_HIP;
  const size_t count = (size_t)n;
  DevBuf d_p0, d_p1, d_out;
  if (!d_p0.upload(p0, count * 24) || !d_p1.upload(p1, count * 24) || !d_out.alloc(count)) {
    (void)hipGetLastError();
    return AFE_ERR_HIP;
  }
  RayArgs g = map_args(m);
  g.total = n;
  g.a = d_p0.as<double>(); g.b = d_p1.as<double>();
  g.blocked_out = d_out.as<uint8_t>();
  float ms = 0;
  const int rc = launch_rays<kSegment, true, false>(g, n, nullptr, &ms);
  if (rc != AFE_OK) return rc;
  if (kernel_ms) *kernel_ms = ms;
  return d_out.download(blocked, count) ? AFE_OK : AFE_ERR_HIP;
}

// ---------------------------------------------------------------------------------------
// the range sensor
// ---------------------------------------------------------------------------------------
struct afe_range_sensor {
  afe_engine *engine = nullptr;        // borrowed
  afe_clearance_map *map = nullptr;    // borrowed
  int n_beams = 0;
  int64_t n = 0;
  int device = 0;
  double mount[4] = {1.0, 0.0, 0.0, 0.0};
  DevBuf beams;                        // afe_range_beam[n_beams]
};

extern "C" int afe_range_sensor_create(afe_engine *e, afe_clearance_map *m, const double mount[4], const afe_range_beam *beams, int n_beams,
                                       afe_range_sensor **out) {
  if (!e || !m || !beams || !out) return AFE_ERR_INVALID_ARG;
  if (mount) for (int k = 0; k < 4; k++) if (!std::isfinite(mount[k])) return AFE_ERR_INVALID_ARG;
  if (n_beams < 1 || n_beams > kMaxBeams) return AFE_ERR_OUT_OF_RANGE;
  for (int b = 0; b < n_beams; b++)
    for (int k = 0; k < 3; k++) if (!std::isfinite(beams[b].off[k]) || !std::isfinite(beams[b].dir[k])) return AFE_ERR_INVALID_ARG;
  for (int b = 0; b < n_beams; b++) if (!t_max_ok(beams[b].t_max) || (beams[b].frame != 0 && beams[b].frame != 1)) return AFE_ERR_OUT_OF_RANGE;
  EngineAccess acc;
  const int rc = afe::engine_enter(e, &acc);
  if (rc != AFE_OK) return rc;
  if (acc.device != m->device) return AFE_ERR_INVALID_ARG;
  afe_range_sensor *s = new afe_range_sensor();
  s->engine = e; s->map = m; s->n_beams = n_beams; s->n = acc.view.n_vehicles; s->device = acc.device;
  if (mount) for (int k = 0; k < 4; k++) s->mount[k] = mount[k];
  if (!s->beams.upload(beams, (size_t)n_beams * sizeof(afe_range_beam))) {
    (void)hipGetLastError();
    delete s;
    return AFE_ERR_HIP;
  }
  *out = s;
  return AFE_OK;
}

extern "C" int afe_range_sensor_update(afe_range_sensor *s, int64_t first, int64_t count, void *t_out, void *tri_out, int out_is_device,
                                       float *kernel_ms) {
  if (!s || first < 0 || count < 0) return AFE_ERR_INVALID_ARG;
  if (count > 0 && !t_out) return AFE_ERR_INVALID_ARG;
  if (afe::engine_range_bad(s->engine, first, count)) return AFE_ERR_OUT_OF_RANGE;
  if (count == 0) return AFE_OK;          // a valid range of nothing: answered before the engine is touched
  EngineAccess acc;
  int rc = afe::engine_enter(s->engine, &acc);     // (ends a resident grid, as the camera does)
  if (rc != AFE_OK) return rc;
  if (acc.device != s->device || acc.view.n_vehicles != s->n) return AFE_ERR_INVALID_ARG;
  const afe_device_view &view = acc.view;
  const hipStream_t stream = acc.stream;
  const int64_t n_rays = (int64_t)s->n_beams * count;
  const size_t n = (size_t)n_rays;
  DevBuf d_t, d_tri;
  RayArgs g = map_args(s->map);
  g.total = n_rays;
  g.pos = view.pos; g.att = view.att; g.anchor_xy = view.pos_anchor_xy; g.stride = view.stride; g.first = first; g.n_veh = count;
  g.elem_size = view.state_elem_size;
  for (int k = 0; k < 4; k++) g.mount[k] = s->mount[k];
  g.beams = s->beams.as<afe_range_beam>();
  if (out_is_device) {
    g.t_out = (double *)t_out; g.tri_out = (int32_t *)tri_out;
  } else {
    if (!d_t.alloc(n * 8) || (tri_out && !d_tri.alloc(n * 4))) { (void)hipGetLastError(); return AFE_ERR_HIP; }
    g.t_out = d_t.as<double>(); g.tri_out = d_tri.as<int32_t>();
  }
  float ms = 0;
  rc = launch_rays<kEngine, false, false>(g, n_rays, stream, kernel_ms ? &ms : nullptr);
  // (host outputs: the buffers above must outlive the work in flight, also where a step below fails)
  if (rc == AFE_OK && !out_is_device &&
      (hipMemcpyAsync(t_out, g.t_out, n * 8, hipMemcpyDeviceToHost, stream) != hipSuccess ||
       (tri_out && hipMemcpyAsync(tri_out, g.tri_out, n * 4, hipMemcpyDeviceToHost, stream) != hipSuccess)))
    rc = AFE_ERR_HIP;
  if (!out_is_device && hipStreamSynchronize(stream) != hipSuccess) rc = AFE_ERR_HIP;
  if (rc == AFE_OK && kernel_ms) *kernel_ms = ms;
  return rc;
}

extern "C" int afe_range_sensor_info(const afe_range_sensor *s, int *n_beams, int64_t *n_vehicles) {
  if (!s) return AFE_ERR_INVALID_ARG;
  if (n_beams) *n_beams = s->n_beams;
  if (n_vehicles) *n_vehicles = s->n;
  return AFE_OK;
}

extern "C" int afe_range_sensor_destroy(afe_range_sensor *s) {
  if (!s) return AFE_ERR_INVALID_ARG;
  (void)hipSetDevice(s->device);
  (void)hipDeviceSynchronize();      // an update on some stream may still be reading the beam table
  delete s;
  return AFE_OK;
}
