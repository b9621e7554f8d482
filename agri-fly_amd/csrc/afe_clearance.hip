// afe_clearance.hip -- nearest point of a static triangle mesh for every vehicle (or explicit point), and the
// device-resident contact monitor built on it.  The C ABI is in include/agrifly_engine.h ("mesh clearance").
//
// THE DEFINITION (tests/clearance_checker.py restates it in numpy float64, operation for operation; kernel and checker
// must give the same bits, so the ORDER of the operations below is part of the contract).  Everything is IEEE double with
// contraction off; only + - * / and comparisons appear, each correctly rounded on gfx950 and in numpy.
//
//   dot(u, v) = u.x*v.x + u.y*v.y + u.z*v.z                       (left to right)
//   per triangle, once, at creation:   a = (double)v0,  ab = (double)v1 - a,  ac = (double)v2 - a,
//        n = (ab.y*ac.z - ab.z*ac.y,  ab.z*ac.x - ab.x*ac.z,  ab.x*ac.y - ab.y*ac.x)
//        degenerate  <=>  NOT( dot(n, n) > 1e-24 * (dot(ab, ab) * dot(ac, ac)) )       (sine of the corner at a <= 1e-12:
//        coincident vertices and collinear triangles; a float32 sliver is NOT degenerate)
//   per point p:   ap = p - a,  bp = ap - ab,  cp = ap - ac,
//        d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp)
//   tail(s, t):   m = ab*s + ac*t  (per axis),  q = ap - m,  dist2 = dot(q, q),  closest = a + m
//
//   REGIONS (Ericson, Real-Time Collision Detection, 5.1.5), tried in this order, the first that accepts gives (s, t);
//   a region whose parameter is a quotient accepts only with a denominator > 0 (the textbook form divides 0 by 0 when a == b):
//     A    d1 <= 0 and d2 <= 0                                                          (0, 0)
//     B    d3 >= 0 and d4 <= d3                                                         (1, 0)
//     AB   vc = d1*d4 - d3*d2;  vc <= 0 and d1 >= 0 and d3 <= 0 and (d1 - d3) > 0       (d1 / (d1 - d3), 0)
//     C    d6 >= 0 and d5 <= d6                                                         (0, 1)
//     AC   vb = d5*d2 - d1*d6;  vb <= 0 and d2 >= 0 and d6 <= 0 and (d2 - d6) > 0       (0, d2 / (d2 - d6))
//     BC   va = d3*d6 - d5*d4;  e43 = d4 - d3, e56 = d5 - d6;
//          va <= 0 and e43 >= 0 and e56 >= 0 and (e43 + e56) > 0                        t = e43 / (e43 + e56), s = 1 - t
//     IN   den = (va + vb) + vc;  den > 0                                               r = 1 / den, s = vb*r, t = vc*r
//   dist2 = tail(s, t).
//
//   SEGMENT RULE, used instead when the triangle is degenerate, when no region accepted, or when the dist2 above is not
//   < +inf (which makes the definition total: a finite dist2 >= 0 for every finite triangle and point whose squares do
//   not overflow).  The triangle is measured as the nearest of its three sides, parameters clamped, a side of zero length
//   being its end point:  clamp(w) = w < 0 ? 0 : (w > 1 ? 1 : w)
//     AB   l = dot(ab, ab);                 s = l > 0 ? clamp(d1 / l) : 0,          t = 0
//     AC   l = dot(ac, ac);                 s = 0,                                  t = l > 0 ? clamp(d2 / l) : 0
//     BC   e = ac - ab,  l = dot(e, e);     w = l > 0 ? clamp(dot(e, bp) / l) : 0,  s = 1 - w,  t = w
//   dist2 = the smallest tail(s, t) of the three; a later side replaces an earlier one only when strictly smaller; a NaN
//   replaces nothing (start from +inf).
//
//   WINNER over the triangles: only dist2 < +inf and dist2 <= max_dist2 count (max_dist2 = max_dist*max_dist, formed once
//   on the host in double); the smallest dist2 wins, among bitwise-equal dist2 the lowest index in the order given to
//   afe_clearance_map_create.  A point with no such triangle: dist2 = +inf, index -1, closest = NaN.  A point with a
//   non-finite coordinate: the same, without a walk.
//
// THE STRUCTURE.  Its own handle and its own tree (the camera's, afe_render.hip, is built for 64 coherent rays walking by
// scalar loads: pair nodes in eight mirrored copies with ray-inflated boxes).  Here the points of neighbouring lanes are not
// neighbours in space, so the walk is per lane: a plain binary tree in one copy, median splits on the longest axis of the
// centroid bounds with the input index as the tie-break (balanced whatever the centroids do: depth <= 2 + log2(n / 4), far below
// the 32-entry stack), leaves of 1..4 triangles, exact float32 boxes.  A node record is 64 B, 32 B per child = two dwordx4
// loads: {lo.xyz, ref}, {hi.xyz, -}.  Triangles whose box covers more than a quarter of the scene's (a ground plane's two;
// at most 16) stay out of the tree and are tested first, brute force, which also gives every low-flying point its pruning
// distance before the walk.
//
// NO OUTPUT BIT DEPENDS ON THE BOXES.  The box lower bound lb (per axis max(lo - p, 0, p - hi) in double, squared and summed)
// may only ever err towards visiting: a subtree or triangle is skipped only if  lb * (1 - 2^-40) > best + E, with
// E = 2^-40 * S and S = the squared distance from p to the farthest corner of the scene's box.  The computed dist2 of a
// triangle differs from the exact one by rounding that is ABSOLUTE in the scale of the operands (q = ap - m cancels near the
// surface): at most about 40 roundings of 1.1e-16 on terms bounded by |ap|^2 + |ab|^2 + |ac|^2 <= 9 S, i.e. 4e-14 S, twenty
// times below E = 9e-13 S.  So a skipped triangle's computed dist2 is strictly greater than `best` and could neither win nor
// tie.  (A relative slack alone would not do: a point on an edge has best = 0 and a neighbour's box 1e-9 away.)
//
// The walk's stack lives in LDS as [level][lane] (32 x 256 x 4 B = 32 KB per block, conflict-free: a lane only ever touches
// its own column); a runtime-indexed private array would go to scratch.  Between two updates: the swept monitor (SWEPT CLEARANCE below).
//
// PATH CLEARANCE (afe_clearance_paths, afe_clearance_plans_engine; tests/path_checker.py restates it on top of the checker
// above).  Same rules: IEEE double, contraction off, + - * / and comparisons, the order below is the contract.
//   A path: coeffs c[6][3] (t^5 .. t^0 per axis, the layout of afe_plan_output::coeffs), a time range (t_begin, t_end),
//   optionally an origin o[3] and a row-major matrix R[9].  K = n_samples, 2 <= K <= 4096.
//   sample time:   t_k = t_begin + (t_end - t_begin) * ((double)k / (double)(K - 1))  for k < K - 1;   t_{K-1} = t_end exactly
//   sample point:  per axis, Horner:  p = c[0];  p = p*t + c[j]  for j = 1 .. 5
//        with R:      w.x = o.x + ((R0*p.x + R1*p.y) + R2*p.z),  w.y and w.z with rows 1 and 2
//        without R:   w = o + p;     without o either:  w = p   (no zero is added: a -0 stays -0)
//   per sample:    (d2_k, tri_k, closest_k) = the UNBOUNDED point query above at w  (non-finite w: +inf, -1, NaN)
//   the record (afe_path_clearance), with radius2 = radius*radius and max_dist2 = max_dist*max_dist formed once on the host:
//        n_nonfinite  = #{k : w has a non-finite coordinate}
//        n_hit        = #{k : d2_k <= radius2};   k_first_hit = the lowest such k (-1: none), tri_first_hit = tri of that k,
//                       t_first_hit = t of that k (NaN: none)
//        min_dist2    = the smallest d2_k among the samples with d2_k < +inf and d2_k <= max_dist2;  k_min = the lowest k among bitwise-equal
//                       minima;  tri_min, closest[3], t_min from that sample.  No such sample: +inf, -1, -1, NaN, NaN.
//   afe_clearance_plans_engine: o = the vehicle's position, R = the camera-to-world matrix of att * mount, both formed with
//   the camera's own function (afe_pose.h, shared with afe_camera_pose_kernel), the range is [0, tf]; a plan with
//   found == 0 is not sampled and gets the empty record (+inf, every index -1, NaNs, both counts 0).
//
// One wave per path, one sample per lane, batches of 64 samples; four paths per block, so the [32][256] stack carries over;
// no barrier anywhere.  The sample points only ever exist in registers.  A lane starts its walk with the bound
// max(radius2, best), best = the wave's smallest d2 of the earlier batches (initially max_dist2), wave-uniform.  No output
// bit depends on that: a sample is a hit iff its own d2 <= radius2 and the bound never drops below radius2; clr_eval accepts
// ties at the bound, so a sample at or below the bound gets its exact d2, triangle and closest point; a later sample that
// only ties the running minimum loses on k; a sample above the bound can be neither.  Reduction per batch by wave
// operations: min of (d2, lane) by a butterfly, first hit by ballot + first set bit, n_hit by popcount; lane 0 writes the
// record.  Between two samples a path can come closer than at both: afe_clearance_paths_swept measures the chords (below).
//
// SWEPT CLEARANCE (afe_clearance_segments, afe_contact_monitor_create_swept, afe_clearance_paths_swept,
// afe_clearance_plans_engine_swept; tests/swept_checker.py restates it on top of the checker above).  The exact squared
// distance between a SEGMENT P0 -> P1 and the mesh.  Same rules: IEEE double, contraction off, + - * / and comparisons, the
// order below is the contract.  evaluate(p) is THE DEFINITION above for the point p (its dist2, +inf where it gives nothing
// below +inf, and its closest point a + (ab*s + ac*t)); dot and clamp as above.
//   One triangle (a, ab, ac, degenerate) against one segment; the candidates, in this order:
//     d = P1 - P0;  A = dot(d, d)
//     0   evaluate(P0)                                                     segment parameter s = 0
//         if NOT (A > 0): no further candidate (a segment of zero length is the point query, bit for bit)
//     1   evaluate(P1)                                                     s = 1
//     2   the plane crossing, only if not degenerate:
//         u0 = P0 - a, u1 = P1 - a,  n = ab x ac (the order of the creation formula),  h0 = dot(n, u0), h1 = dot(n, u1)
//         only if (h0 > 0 and h1 < 0) or (h0 < 0 and h1 > 0):   s = h0 / (h0 - h1),  x = P0 + d*s (per axis),  evaluate(x)
//     3, 4, 5   the segment against the side AB (o = 0, g = ab), AC (o = 0, g = ac), BC (o = ab, g = ac - ab), in the a-frame:
//         r = u0 - o;  E = dot(g, g);  F = dot(g, r);  C = dot(d, r);  B = dot(d, g)
//         E > 0 false:   t = 0,  s = clamp(-C / A)
//         else:   den = A*E - B*B;  s = den > 0 ? clamp((B*F - C*E) / den) : 0;  t = (B*s + F) / E
//                 t < 0:  t = 0, s = clamp(-C / A);      t > 1:  t = 1, s = clamp((B - C) / A)
//         q = (r + d*s) - g*t (per axis);  dist2 = dot(q, q);  closest = a + (o + g*t)
//   The triangle's answer starts at +inf; a candidate replaces it only when strictly smaller, a NaN replaces nothing; its
//   kind is the number of the candidate that holds it, its s that candidate's s.
//   WINNER over the triangles as above: only dist2 < +inf and dist2 <= max_dist2 count, the smallest wins, among bitwise-
//   equal dist2 the lowest input index.  No such triangle, or a segment with a non-finite coordinate (no walk): dist2 = +inf,
//   s = NaN, closest = NaN, index -1, kind -1.
//   The definition is exact: two sets that do not meet attain their distance at an end of the segment, on the triangle's
//   boundary, or along a stretch parallel to the face that reaches one of the two; a proper crossing is candidate 2,
//   an overlap in the plane an end point or a side.  A pierced triangle gives something like 1e-30, not 0: part of the bits.
//
//   The walk (seg_walk) is clr_walk's, with the lower bound between the segment's own axis-aligned box and the node's or
//   triangle's box: per axis max(lo - smax, 0, smin - hi) in double, squared and summed.  No output bit depends on it: every
//   candidate's dist2 is |q|^2 of two actual points, one of the segment and one of the triangle, up to the roundings of
//   forming q, so it cannot fall below the true distance by more than those; a badly conditioned den or h0 - h1 moves s
//   along the segment, which can only make the candidate larger.  Candidates 0, 1, 3, 4, 5 are formed in the a-frame like the
//   point query's (about 40 roundings on terms bounded by |u0|^2 + |d|^2 + |ab|^2 + |ac|^2 <= 13 S, S = the larger of the two
//   end points' farthest-corner terms): within 2^-40 S as above.  Candidate 2's point x = P0 + d*s is rounded at the scale of
//   the COORDINATES, 3 roundings of 2^-53 |x| per axis, so x lies up to delta = 2^-50 M' off the segment (M' the larger norm
//   of the end points) and its dist2 up to 2 D delta <= 2^-50 (S + M'^2) below the true one.  THE SLACK IS THEREFORE WIDENED
//   for the swept kernels only:  E = 2^-40 (S + M),  M = the larger of |P0|^2 and |P1|^2 -- nothing near the origin, 3e-5 m^2
//   four kilometres from it.  So a skipped triangle's computed dist2 is strictly above `best`, as for points.
//   The segment's box is loose for a long diagonal segment; that costs time, never bits.  The swept entries are meant for
//   tick-to-tick motion and the chords of a sampled path.
//
//   The swept monitor keeps, per vehicle, the double-precision world position its last update formed (anchors added) and a
//   valid flag; an update measures the segment from there to the current position and then stores the current one (the flag
//   is set iff that position is finite).  No previous position (creation, afe_contact_monitor_reset, a non-finite one): the
//   segment is the point.  The latches and counts are the point monitor's.
//   The swept audit: sample points w_k exactly as in PATH CLEARANCE; chord k = (w_k, w_k+1), k = 0 .. K-2, answered by the
//   UNBOUNDED segment query (an end with a non-finite coordinate: +inf, counted in n_nonfinite); the record
//   (afe_path_sweep) is afe_path_clearance's over chords, plus s_min and s_first_hit; the time of a chord's closest point is
//   t_k + (t_k+1 - t_k) * s.  One wave per path, one chord per lane, batches of 64 chords, the bound carried as above.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <mutex>
#include <type_traits>
#include <vector>

#include "afe_clearance_map.h"
#include "afe_consumer.h"
#include "afe_pose.h"

namespace {

using afe::DevBuf;
using afe::EngineAccess;
using afe::PinnedBuf;
using afe::StreamTimer;
using namespace afe::clr;   // the map's records and constants (afe_clearance_map.h)

struct Best {
  double d2;
  int32_t idx;
  double cx, cy, cz;
};

__device__ __forceinline__ double clr_dot(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
  return ax * bx + ay * by + az * bz;
}

__device__ __forceinline__ double clr_clamp(double w) { return w < 0.0 ? 0.0 : (w > 1.0 ? 1.0 : w); }

// squared distance from p to the box, in double from the exact float32 faces (lower bound of every distance into it)
__device__ __forceinline__ double clr_box_lb(const float4 lo, const float4 hi, double px, double py, double pz) {
#pragma clang fp contract(off)
  const double dx = fmax(fmax((double)lo.x - px, 0.0), px - (double)hi.x);
  const double dy = fmax(fmax((double)lo.y - py, 0.0), py - (double)hi.y);
  const double dz = fmax(fmax((double)lo.z - pz, 0.0), pz - (double)hi.z);
  return dx * dx + dy * dy + dz * dz;
}

// "may only err towards visiting": false for NaN, for best = +inf, for slack = +inf
__device__ __forceinline__ bool clr_skip(double lb, double best, double slack) {
#pragma clang fp contract(off)
  return lb * (1.0 - 0x1p-40) > best + slack;
}

// the definition (file header), one triangle against one point; updates the winner.  THE SAME ARITHMETIC STANDS A SECOND TIME
// in clr_point below, for the swept evaluator: a change to the definition is made in both (tests/test_gpu_swept.py compares
// the two on the device, zero-length segments against the point query and degenerate triangles included).
__device__ __forceinline__ void clr_eval(const CTri *T, int32_t index, int32_t degenerate, double px, double py, double pz, Best &b) {
#pragma clang fp contract(off)
  const double ax = T->a[0], ay = T->a[1], az = T->a[2];
  const double abx = T->ab[0], aby = T->ab[1], abz = T->ab[2];
  const double acx = T->ac[0], acy = T->ac[1], acz = T->ac[2];
  const double apx = px - ax, apy = py - ay, apz = pz - az;
  const double bpx = apx - abx, bpy = apy - aby, bpz = apz - abz;
  const double d1 = clr_dot(abx, aby, abz, apx, apy, apz), d2 = clr_dot(acx, acy, acz, apx, apy, apz);
  double s = 0.0, t = 0.0, mx, my, mz, qx, qy, qz;
  double d = std::numeric_limits<double>::infinity();
  bool accepted = false;
  if (!degenerate) {
    const double cpx = apx - acx, cpy = apy - acy, cpz = apz - acz;
    const double d3 = clr_dot(abx, aby, abz, bpx, bpy, bpz), d4 = clr_dot(acx, acy, acz, bpx, bpy, bpz);
    const double d5 = clr_dot(abx, aby, abz, cpx, cpy, cpz), d6 = clr_dot(acx, acy, acz, cpx, cpy, cpz);
    if (d1 <= 0.0 && d2 <= 0.0) { accepted = true; }
    else if (d3 >= 0.0 && d4 <= d3) { s = 1.0; accepted = true; }
    else {
      const double vc = d1 * d4 - d3 * d2, den_ab = d1 - d3;
      if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0 && den_ab > 0.0) { s = d1 / den_ab; accepted = true; }
      else if (d6 >= 0.0 && d5 <= d6) { t = 1.0; accepted = true; }
      else {
        const double vb = d5 * d2 - d1 * d6, den_ac = d2 - d6;
        if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0 && den_ac > 0.0) { t = d2 / den_ac; accepted = true; }
        else {
          const double va = d3 * d6 - d5 * d4, e43 = d4 - d3, e56 = d5 - d6, den_bc = e43 + e56;
          if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0 && den_bc > 0.0) { t = e43 / den_bc; s = 1.0 - t; accepted = true; }
          else {
            const double den = (va + vb) + vc;
            if (den > 0.0) { const double r = 1.0 / den; s = vb * r; t = vc * r; accepted = true; }
          }
        }
      }
    }
    if (accepted) {
      mx = abx * s + acx * t; my = aby * s + acy * t; mz = abz * s + acz * t;
      qx = apx - mx; qy = apy - my; qz = apz - mz;
      d = clr_dot(qx, qy, qz, qx, qy, qz);
    }
  }
  if (!(d < std::numeric_limits<double>::infinity())) {     // the segment rule (degenerate / nothing accepted / not finite)
    d = std::numeric_limits<double>::infinity();
    s = 0.0; t = 0.0;
    const double ex = acx - abx, ey = acy - aby, ez = acz - abz;
    const double l_ab = clr_dot(abx, aby, abz, abx, aby, abz), l_ac = clr_dot(acx, acy, acz, acx, acy, acz);
    const double l_bc = clr_dot(ex, ey, ez, ex, ey, ez);
    const double w_ab = l_ab > 0.0 ? clr_clamp(d1 / l_ab) : 0.0;
    const double w_ac = l_ac > 0.0 ? clr_clamp(d2 / l_ac) : 0.0;
    const double w_bc = l_bc > 0.0 ? clr_clamp(clr_dot(ex, ey, ez, bpx, bpy, bpz) / l_bc) : 0.0;
    for (int side = 0; side < 3; side++) {
      const double ss = side == 0 ? w_ab : (side == 1 ? 0.0 : 1.0 - w_bc);
      const double tt = side == 0 ? 0.0 : (side == 1 ? w_ac : w_bc);
      const double nx = abx * ss + acx * tt, ny = aby * ss + acy * tt, nz = abz * ss + acz * tt;
      const double rx = apx - nx, ry = apy - ny, rz = apz - nz;
      const double dd = clr_dot(rx, ry, rz, rx, ry, rz);
      if (dd < d) { d = dd; s = ss; t = tt; }
    }
    mx = abx * s + acx * t; my = aby * s + acy * t; mz = abz * s + acz * t;
  }
  if (d < std::numeric_limits<double>::infinity() && (d < b.d2 || (d == b.d2 && index < b.idx))) {
    b.d2 = d;
    b.idx = index;
    b.cx = ax + mx; b.cy = ay + my; b.cz = az + mz;
  }
}

// clr_eval's arithmetic once more, for the swept evaluator, which needs the answer and not the winner's update: one triangle
// (a, ab, ac, degenerate) against one point gives dist2 (+inf: nothing below +inf) and m = ab*s + ac*t of the closest point
// a + m.  (Kept beside clr_eval, not under it: the point kernels are to compile to exactly what they were.)
__device__ __forceinline__ void clr_point(double ax, double ay, double az, double abx, double aby, double abz, double acx, double acy, double acz,
                                          int32_t degenerate, double px, double py, double pz, double &d, double &mx, double &my, double &mz) {
#pragma clang fp contract(off)
  const double apx = px - ax, apy = py - ay, apz = pz - az;
  const double bpx = apx - abx, bpy = apy - aby, bpz = apz - abz;
  const double d1 = clr_dot(abx, aby, abz, apx, apy, apz), d2 = clr_dot(acx, acy, acz, apx, apy, apz);
  double s = 0.0, t = 0.0, qx, qy, qz;
  d = std::numeric_limits<double>::infinity();
  bool accepted = false;
  if (!degenerate) {
    const double cpx = apx - acx, cpy = apy - acy, cpz = apz - acz;
    const double d3 = clr_dot(abx, aby, abz, bpx, bpy, bpz), d4 = clr_dot(acx, acy, acz, bpx, bpy, bpz);
    const double d5 = clr_dot(abx, aby, abz, cpx, cpy, cpz), d6 = clr_dot(acx, acy, acz, cpx, cpy, cpz);
    if (d1 <= 0.0 && d2 <= 0.0) { accepted = true; }
    else if (d3 >= 0.0 && d4 <= d3) { s = 1.0; accepted = true; }
    else {
      const double vc = d1 * d4 - d3 * d2, den_ab = d1 - d3;
      if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0 && den_ab > 0.0) { s = d1 / den_ab; accepted = true; }
      else if (d6 >= 0.0 && d5 <= d6) { t = 1.0; accepted = true; }
      else {
        const double vb = d5 * d2 - d1 * d6, den_ac = d2 - d6;
        if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0 && den_ac > 0.0) { t = d2 / den_ac; accepted = true; }
        else {
          const double va = d3 * d6 - d5 * d4, e43 = d4 - d3, e56 = d5 - d6, den_bc = e43 + e56;
          if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0 && den_bc > 0.0) { t = e43 / den_bc; s = 1.0 - t; accepted = true; }
          else {
            const double den = (va + vb) + vc;
            if (den > 0.0) { const double r = 1.0 / den; s = vb * r; t = vc * r; accepted = true; }
          }
        }
      }
    }
    if (accepted) {
      mx = abx * s + acx * t; my = aby * s + acy * t; mz = abz * s + acz * t;
      qx = apx - mx; qy = apy - my; qz = apz - mz;
      d = clr_dot(qx, qy, qz, qx, qy, qz);
    }
  }
  if (!(d < std::numeric_limits<double>::infinity())) {     // the segment rule (degenerate / nothing accepted / not finite)
    d = std::numeric_limits<double>::infinity();
    s = 0.0; t = 0.0;
    const double ex = acx - abx, ey = acy - aby, ez = acz - abz;
    const double l_ab = clr_dot(abx, aby, abz, abx, aby, abz), l_ac = clr_dot(acx, acy, acz, acx, acy, acz);
    const double l_bc = clr_dot(ex, ey, ez, ex, ey, ez);
    const double w_ab = l_ab > 0.0 ? clr_clamp(d1 / l_ab) : 0.0;
    const double w_ac = l_ac > 0.0 ? clr_clamp(d2 / l_ac) : 0.0;
    const double w_bc = l_bc > 0.0 ? clr_clamp(clr_dot(ex, ey, ez, bpx, bpy, bpz) / l_bc) : 0.0;
    for (int side = 0; side < 3; side++) {
      const double ss = side == 0 ? w_ab : (side == 1 ? 0.0 : 1.0 - w_bc);
      const double tt = side == 0 ? 0.0 : (side == 1 ? w_ac : w_bc);
      const double nx = abx * ss + acx * tt, ny = aby * ss + acy * tt, nz = abz * ss + acz * tt;
      const double rx = apx - nx, ry = apy - ny, rz = apz - nz;
      const double dd = clr_dot(rx, ry, rz, rx, ry, rz);
      if (dd < d) { d = dd; s = ss; t = tt; }
    }
    mx = abx * s + acx * t; my = aby * s + acy * t; mz = abz * s + acz * t;
  }
}

// box of the triangle first (32 B), the double-precision part only if the box could hold a winner
template <bool COUNT>
__device__ __forceinline__ void clr_test(const CTri *T, double px, double py, double pz, double slack, Best &b, unsigned &n_box, unsigned &n_eval) {
  const float4 *head = reinterpret_cast<const float4 *>(T);
  const float4 h0 = head[0], h1 = head[1];        // lo.xyz hi.x | hi.yz index degenerate
  float4 lo, hi;
  lo.x = h0.x; lo.y = h0.y; lo.z = h0.z; lo.w = 0.0f;
  hi.x = h0.w; hi.y = h1.x; hi.z = h1.y; hi.w = 0.0f;
  if (COUNT) n_box++;
  if (clr_skip(clr_box_lb(lo, hi, px, py, pz), b.d2, slack)) return;
  if (COUNT) n_eval++;
  clr_eval(T, __float_as_int(h1.z), __float_as_int(h1.w), px, py, pz, b);
}

// The walk for one finite point, starting from the bound and winner in b: the triangles kept out of the tree, then the tree,
// nearer child first.  `col` is the lane's column of the block's stack.  Shared by the point query and the path kernel.
template <bool COUNT>
__device__ __forceinline__ void clr_walk(const ClrArgs &g, double px, double py, double pz, Best &b, uint32_t (*stack)[kBlock], int col,
                                         unsigned &n_nodes, unsigned &n_box, unsigned &n_eval) {
#pragma clang fp contract(off)
  // S: squared distance to the farthest corner of the scene's box (bounds |p - vertex|^2 for every vertex)
  const double fx = fmax(fabs(px - g.scene_lo[0]), fabs(px - g.scene_hi[0]));
  const double fy = fmax(fabs(py - g.scene_lo[1]), fabs(py - g.scene_hi[1]));
  const double fz = fmax(fabs(pz - g.scene_lo[2]), fabs(pz - g.scene_hi[2]));
  const double slack = 0x1p-40 * (fx * fx + fy * fy + fz * fz);
  for (uint32_t k = 0; k < g.n_big; k++) clr_test<COUNT>(g.tris + g.big_first + k, px, py, pz, slack, b, n_box, n_eval);
  uint32_t cur = g.root_ref;
  if (cur != kNone) {
    float4 lo, hi;
    lo.x = g.root_lo[0]; lo.y = g.root_lo[1]; lo.z = g.root_lo[2]; lo.w = 0.0f;
    hi.x = g.root_hi[0]; hi.y = g.root_hi[1]; hi.z = g.root_hi[2]; hi.w = 0.0f;
    if (clr_skip(clr_box_lb(lo, hi, px, py, pz), b.d2, slack)) cur = kNone;
  }
  int sp = 0;
  while (cur != kNone) {                 // bounded: every node is entered at most once
    if (cur & kLeafBit) {
      const uint32_t first = cur & kFirstMask, cnt = (cur >> 28) & 7u;
      for (uint32_t k = 0; k < cnt; k++) clr_test<COUNT>(g.tris + first + k, px, py, pz, slack, b, n_box, n_eval);
      cur = kNone;
    } else {
      if (COUNT) n_nodes++;
      const float4 *rec = reinterpret_cast<const float4 *>(g.nodes + cur);
      const float4 lo0 = rec[0], hi0 = rec[1], lo1 = rec[2], hi1 = rec[3];
      const double lb0 = clr_box_lb(lo0, hi0, px, py, pz), lb1 = clr_box_lb(lo1, hi1, px, py, pz);
      const bool go0 = !clr_skip(lb0, b.d2, slack), go1 = !clr_skip(lb1, b.d2, slack);
      const uint32_t ref0 = (uint32_t)__float_as_int(lo0.w), ref1 = (uint32_t)__float_as_int(lo1.w);
      if (go0 && go1) {
        const bool near0 = lb0 <= lb1;
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

template <bool MONITOR, bool COUNT>
__global__ void __launch_bounds__(kBlock) afe_clearance_kernel(ClrArgs g) {
#pragma clang fp contract(off)
  __shared__ uint32_t stack[kStack][kBlock];
  const int lane = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * kBlock + lane;
  const bool valid = i < g.count;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  double px = nan, py = nan, pz = nan;
  if (valid) {
    const int64_t v = g.first + i;
    if (g.elem_size == 8) {
      const double *P = (const double *)g.pos;
      px = P[v]; py = P[g.stride + v]; pz = P[2 * g.stride + v];
    } else {
      const float *P = (const float *)g.pos;
      px = (double)P[v]; py = (double)P[g.stride + v]; pz = (double)P[2 * g.stride + v];
    }
    if (g.anchor_xy) { px = g.anchor_xy[v] + px; py = g.anchor_xy[g.stride + v] + py; }
  }
  Best b;
  b.d2 = g.max_dist2; b.idx = 0x7fffffff; b.cx = nan; b.cy = nan; b.cz = nan;
  unsigned n_nodes = 0, n_box = 0, n_eval = 0;
  if (valid && __builtin_isfinite(px) && __builtin_isfinite(py) && __builtin_isfinite(pz)) {
    clr_walk<COUNT>(g, px, py, pz, b, stack, lane, n_nodes, n_box, n_eval);
  }
  const bool found = b.idx != 0x7fffffff;
  if (valid) {
    if (g.dist2_out) g.dist2_out[i] = found ? b.d2 : inf;
    if (g.tri_out) g.tri_out[i] = found ? b.idx : -1;
    if (g.closest_out) {
      g.closest_out[i] = found ? b.cx : nan;
      g.closest_out[g.out_stride + i] = found ? b.cy : nan;
      g.closest_out[2 * g.out_stride + i] = found ? b.cz : nan;
    }
  }
  if (MONITOR) {
    bool now = false, ever = false;
    if (valid) {
      const int64_t v = g.first + i;
      if (found && b.d2 < g.min_dist2[v]) g.min_dist2[v] = b.d2;
      now = found && b.d2 <= g.contact2;
      uint64_t latched = g.first_us[v];
      if (now && latched == ~uint64_t(0)) {
        g.first_us[v] = g.now_us;
        g.first_tri[v] = b.idx;
        latched = g.now_us;
      }
      ever = latched != ~uint64_t(0);
    }
    // the two counts: ballot + popcount, then ONE vector atomic per wave (lanes 0 and 1 of it, one word each)
    const unsigned long long n_now = (unsigned long long)__popcll(__ballot(now));
    const unsigned long long n_ever = (unsigned long long)__popcll(__ballot(ever));
    const int wl = lane & 63;
    if (wl < 2 && (n_now | n_ever)) atomicAdd(g.counts + wl, wl == 0 ? n_now : n_ever);
  }
  if (COUNT && valid) {
    atomicAdd(g.stats + 0, (unsigned long long)n_nodes);
    atomicAdd(g.stats + 1, (unsigned long long)n_box);
    atomicAdd(g.stats + 2, (unsigned long long)n_eval);
  }
}

__global__ void __launch_bounds__(kBlock) afe_clearance_reset_kernel(double *min_dist2, uint64_t *first_us, int32_t *first_tri, int64_t first,
                                                                      int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  min_dist2[first + i] = std::numeric_limits<double>::infinity();
  first_us[first + i] = ~uint64_t(0);
  first_tri[first + i] = -1;
}

// ---------------------------------------------------------------------------------------
// swept clearance (the definition: file header, SWEPT CLEARANCE)
// ---------------------------------------------------------------------------------------
struct SegBest {
  double d2, s;
  double cx, cy, cz;
  int32_t idx, kind;
};

// the swept definition, one triangle against one segment P0 -> P1; updates the winner.  The two candidate loops stay loops
// (one copy of the point evaluator and one of the side test in the code); what differs between their turns is selected
// into scalars, never indexed.
__device__ __forceinline__ void seg_eval(const CTri *T, int32_t index, int32_t degenerate, double p0x, double p0y, double p0z, double p1x,
                                         double p1y, double p1z, SegBest &b) {
#pragma clang fp contract(off)
  const double inf = std::numeric_limits<double>::infinity();
  const double ax = T->a[0], ay = T->a[1], az = T->a[2];
  const double abx = T->ab[0], aby = T->ab[1], abz = T->ab[2];
  const double acx = T->ac[0], acy = T->ac[1], acz = T->ac[2];
  const double dx = p1x - p0x, dy = p1y - p0y, dz = p1z - p0z;
  const double A = clr_dot(dx, dy, dz, dx, dy, dz);
  const bool moving = A > 0.0;
  const double u0x = p0x - ax, u0y = p0y - ay, u0z = p0z - az;
  double best = inf, best_s = 0.0, cx = 0.0, cy = 0.0, cz = 0.0;
  int kind = 0;
  const int n_points = moving ? (degenerate ? 2 : 3) : 1;
#pragma unroll 1
  for (int c = 0; c < n_points; c++) {            // candidates 0, 1, 2: points of the segment against the triangle
    double s = 0.0, x = p0x, y = p0y, z = p0z;
    if (c == 1) { s = 1.0; x = p1x; y = p1y; z = p1z; }
    if (c == 2) {
      const double u1x = p1x - ax, u1y = p1y - ay, u1z = p1z - az;
      const double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
      const double h0 = clr_dot(nx, ny, nz, u0x, u0y, u0z), h1 = clr_dot(nx, ny, nz, u1x, u1y, u1z);
      if (!((h0 > 0.0 && h1 < 0.0) || (h0 < 0.0 && h1 > 0.0))) break;
      s = h0 / (h0 - h1);
      x = p0x + dx * s; y = p0y + dy * s; z = p0z + dz * s;
    }
    double d, mx, my, mz;
    clr_point(ax, ay, az, abx, aby, abz, acx, acy, acz, degenerate, x, y, z, d, mx, my, mz);
    if (d < best) { best = d; best_s = s; kind = c; cx = ax + mx; cy = ay + my; cz = az + mz; }
  }
  if (moving) {
#pragma unroll 1
    for (int side = 0; side < 3; side++) {        // candidates 3, 4, 5: the segment against AB, AC, BC
      const double ox = side == 2 ? abx : 0.0, oy = side == 2 ? aby : 0.0, oz = side == 2 ? abz : 0.0;
      const double gx = side == 0 ? abx : (side == 1 ? acx : acx - abx);
      const double gy = side == 0 ? aby : (side == 1 ? acy : acy - aby);
      const double gz = side == 0 ? abz : (side == 1 ? acz : acz - abz);
      const double rx = u0x - ox, ry = u0y - oy, rz = u0z - oz;
      const double E = clr_dot(gx, gy, gz, gx, gy, gz), F = clr_dot(gx, gy, gz, rx, ry, rz);
      const double Cc = clr_dot(dx, dy, dz, rx, ry, rz), B = clr_dot(dx, dy, dz, gx, gy, gz);
      double s, t;
      if (!(E > 0.0)) {
        t = 0.0; s = clr_clamp(-Cc / A);
      } else {
        const double den = A * E - B * B;
        s = den > 0.0 ? clr_clamp((B * F - Cc * E) / den) : 0.0;
        t = (B * s + F) / E;
        if (t < 0.0) { t = 0.0; s = clr_clamp(-Cc / A); }
        else if (t > 1.0) { t = 1.0; s = clr_clamp((B - Cc) / A); }
      }
      const double qx = (rx + dx * s) - gx * t, qy = (ry + dy * s) - gy * t, qz = (rz + dz * s) - gz * t;
      const double dd = clr_dot(qx, qy, qz, qx, qy, qz);
      if (dd < best) { best = dd; best_s = s; kind = 3 + side; cx = ax + (ox + gx * t); cy = ay + (oy + gy * t); cz = az + (oz + gz * t); }
    }
  }
  if (best < inf && (best < b.d2 || (best == b.d2 && index < b.idx))) {
    b.d2 = best; b.s = best_s;
    b.idx = index; b.kind = kind;
    b.cx = cx; b.cy = cy; b.cz = cz;
  }
}

// squared distance between the segment's own box [slo, shi] and the box (lower bound of every distance between the two)
__device__ __forceinline__ double seg_box_lb(const float4 lo, const float4 hi, double slx, double sly, double slz, double shx, double shy,
                                             double shz) {
#pragma clang fp contract(off)
  const double dx = fmax(fmax((double)lo.x - shx, 0.0), slx - (double)hi.x);
  const double dy = fmax(fmax((double)lo.y - shy, 0.0), sly - (double)hi.y);
  const double dz = fmax(fmax((double)lo.z - shz, 0.0), slz - (double)hi.z);
  return dx * dx + dy * dy + dz * dz;
}

struct SegQuery {       // one lane's segment: the end points and their box
  double p0x, p0y, p0z, p1x, p1y, p1z;
  double slx, sly, slz, shx, shy, shz;
  double slack;
};

template <bool COUNT>
__device__ __forceinline__ void seg_test(const CTri *T, const SegQuery &q, SegBest &b, unsigned &n_box, unsigned &n_eval) {
  const float4 *head = reinterpret_cast<const float4 *>(T);
  const float4 h0 = head[0], h1 = head[1];        // lo.xyz hi.x | hi.yz index degenerate
  float4 lo, hi;
  lo.x = h0.x; lo.y = h0.y; lo.z = h0.z; lo.w = 0.0f;
  hi.x = h0.w; hi.y = h1.x; hi.z = h1.y; hi.w = 0.0f;
  if (COUNT) n_box++;
  if (clr_skip(seg_box_lb(lo, hi, q.slx, q.sly, q.slz, q.shx, q.shy, q.shz), b.d2, q.slack)) return;
  if (COUNT) n_eval++;
  seg_eval(T, __float_as_int(h1.z), __float_as_int(h1.w), q.p0x, q.p0y, q.p0z, q.p1x, q.p1y, q.p1z, b);
}

// clr_walk for one finite segment: the same order (the triangles kept out of the tree, then the tree, nearer child first),
// the lower bound taken from the segment's box, the slack widened as the file header says.
template <bool COUNT>
__device__ __forceinline__ void seg_walk(const ClrArgs &g, double p0x, double p0y, double p0z, double p1x, double p1y, double p1z, SegBest &b,
                                         uint32_t (*stack)[kBlock], int col, unsigned &n_nodes, unsigned &n_box, unsigned &n_eval) {
#pragma clang fp contract(off)
  SegQuery q;
  q.p0x = p0x; q.p0y = p0y; q.p0z = p0z; q.p1x = p1x; q.p1y = p1y; q.p1z = p1z;
  q.slx = fmin(p0x, p1x); q.sly = fmin(p0y, p1y); q.slz = fmin(p0z, p1z);
  q.shx = fmax(p0x, p1x); q.shy = fmax(p0y, p1y); q.shz = fmax(p0z, p1z);
  // S: the larger of the end points' farthest-corner terms; M: the larger squared norm of the end points (candidate 2's point
  // x = P0 + d*s is rounded at the scale of the coordinates themselves)
  const double fx = fmax(fmax(fabs(p0x - g.scene_lo[0]), fabs(p0x - g.scene_hi[0])), fmax(fabs(p1x - g.scene_lo[0]), fabs(p1x - g.scene_hi[0])));
  const double fy = fmax(fmax(fabs(p0y - g.scene_lo[1]), fabs(p0y - g.scene_hi[1])), fmax(fabs(p1y - g.scene_lo[1]), fabs(p1y - g.scene_hi[1])));
  const double fz = fmax(fmax(fabs(p0z - g.scene_lo[2]), fabs(p0z - g.scene_hi[2])), fmax(fabs(p1z - g.scene_lo[2]), fabs(p1z - g.scene_hi[2])));
  const double M = fmax(clr_dot(p0x, p0y, p0z, p0x, p0y, p0z), clr_dot(p1x, p1y, p1z, p1x, p1y, p1z));
  q.slack = 0x1p-40 * ((fx * fx + fy * fy + fz * fz) + M);
  for (uint32_t k = 0; k < g.n_big; k++) seg_test<COUNT>(g.tris + g.big_first + k, q, b, n_box, n_eval);
  uint32_t cur = g.root_ref;
  if (cur != kNone) {
    float4 lo, hi;
    lo.x = g.root_lo[0]; lo.y = g.root_lo[1]; lo.z = g.root_lo[2]; lo.w = 0.0f;
    hi.x = g.root_hi[0]; hi.y = g.root_hi[1]; hi.z = g.root_hi[2]; hi.w = 0.0f;
    if (clr_skip(seg_box_lb(lo, hi, q.slx, q.sly, q.slz, q.shx, q.shy, q.shz), b.d2, q.slack)) cur = kNone;
  }
  int sp = 0;
  while (cur != kNone) {                 // bounded: every node is entered at most once
    if (cur & kLeafBit) {
      const uint32_t first = cur & kFirstMask, cnt = (cur >> 28) & 7u;
      for (uint32_t k = 0; k < cnt; k++) seg_test<COUNT>(g.tris + first + k, q, b, n_box, n_eval);
      cur = kNone;
    } else {
      if (COUNT) n_nodes++;
      const float4 *rec = reinterpret_cast<const float4 *>(g.nodes + cur);
      const float4 lo0 = rec[0], hi0 = rec[1], lo1 = rec[2], hi1 = rec[3];
      const double lb0 = seg_box_lb(lo0, hi0, q.slx, q.sly, q.slz, q.shx, q.shy, q.shz);
      const double lb1 = seg_box_lb(lo1, hi1, q.slx, q.sly, q.slz, q.shx, q.shy, q.shz);
      const bool go0 = !clr_skip(lb0, b.d2, q.slack), go1 = !clr_skip(lb1, b.d2, q.slack);
      const uint32_t ref0 = (uint32_t)__float_as_int(lo0.w), ref1 = (uint32_t)__float_as_int(lo1.w);
      if (go0 && go1) {
        const bool near0 = lb0 <= lb1;
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

// One segment per lane.  Explicit segments: P1 is read as the point kernel reads its point (g.pos, planar doubles), P0 from
// `p0` in the same layout, a record per segment goes to `out`.  MONITOR: P1 is the vehicle's position formed as the point
// monitor forms it, P0 the position the vehicle's last update formed (prev, planar [3][g.stride]; prev_valid 0: none, the
// segment is the point P1); the latches are the point monitor's.
struct SegArgs {
  ClrArgs g;
  const double *p0;
  afe_segment_clearance *out;     // indexed by i
  double *prev;
  uint32_t *prev_valid;
  int64_t prev_stride;
};

template <bool MONITOR, bool COUNT>
__global__ void __launch_bounds__(kBlock) afe_swept_kernel(SegArgs a) {
#pragma clang fp contract(off)
  __shared__ uint32_t stack[kStack][kBlock];
  const ClrArgs &g = a.g;
  const int lane = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * kBlock + lane;
  const bool valid = i < g.count;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  double p0x = nan, p0y = nan, p0z = nan, p1x = nan, p1y = nan, p1z = nan;
  if (valid) {
    const int64_t v = g.first + i;
    if (g.elem_size == 8) {
      const double *P = (const double *)g.pos;
      p1x = P[v]; p1y = P[g.stride + v]; p1z = P[2 * g.stride + v];
    } else {
      const float *P = (const float *)g.pos;
      p1x = (double)P[v]; p1y = (double)P[g.stride + v]; p1z = (double)P[2 * g.stride + v];
    }
    if (g.anchor_xy) { p1x = g.anchor_xy[v] + p1x; p1y = g.anchor_xy[g.stride + v] + p1y; }
    if (MONITOR) {
      const bool has = a.prev_valid[v] != 0;
      p0x = has ? a.prev[v] : p1x; p0y = has ? a.prev[a.prev_stride + v] : p1y; p0z = has ? a.prev[2 * a.prev_stride + v] : p1z;
      a.prev[v] = p1x; a.prev[a.prev_stride + v] = p1y; a.prev[2 * a.prev_stride + v] = p1z;
      a.prev_valid[v] = (__builtin_isfinite(p1x) && __builtin_isfinite(p1y) && __builtin_isfinite(p1z)) ? 1u : 0u;
    } else {
      p0x = a.p0[v]; p0y = a.p0[g.stride + v]; p0z = a.p0[2 * g.stride + v];
    }
  }
  SegBest b;
  b.d2 = g.max_dist2; b.s = nan; b.idx = 0x7fffffff; b.kind = -1; b.cx = nan; b.cy = nan; b.cz = nan;
  unsigned n_nodes = 0, n_box = 0, n_eval = 0;
  if (valid && __builtin_isfinite(p0x) && __builtin_isfinite(p0y) && __builtin_isfinite(p0z) && __builtin_isfinite(p1x) && __builtin_isfinite(p1y) &&
      __builtin_isfinite(p1z)) {
    seg_walk<COUNT>(g, p0x, p0y, p0z, p1x, p1y, p1z, b, stack, lane, n_nodes, n_box, n_eval);
  }
  const bool found = b.idx != 0x7fffffff;
  if (!MONITOR && valid && a.out) {
    afe_segment_clearance *r = a.out + i;
    r->dist2 = found ? b.d2 : inf;
    r->s = found ? b.s : nan;
    r->closest[0] = found ? b.cx : nan; r->closest[1] = found ? b.cy : nan; r->closest[2] = found ? b.cz : nan;
    r->tri = found ? b.idx : -1;
    r->kind = found ? b.kind : -1;
  }
  if (MONITOR) {
    bool now = false, ever = false;
    if (valid) {
      const int64_t v = g.first + i;
      if (found && b.d2 < g.min_dist2[v]) g.min_dist2[v] = b.d2;
      now = found && b.d2 <= g.contact2;
      uint64_t latched = g.first_us[v];
      if (now && latched == ~uint64_t(0)) {
        g.first_us[v] = g.now_us;
        g.first_tri[v] = b.idx;
        latched = g.now_us;
      }
      ever = latched != ~uint64_t(0);
    }
    const unsigned long long n_now = (unsigned long long)__popcll(__ballot(now));
    const unsigned long long n_ever = (unsigned long long)__popcll(__ballot(ever));
    const int wl = lane & 63;
    if (wl < 2 && (n_now | n_ever)) atomicAdd(g.counts + wl, wl == 0 ? n_now : n_ever);
  }
  if (COUNT && valid) {
    atomicAdd(g.stats + 0, (unsigned long long)n_nodes);
    atomicAdd(g.stats + 1, (unsigned long long)n_box);
    atomicAdd(g.stats + 2, (unsigned long long)n_eval);
  }
}

// ---------------------------------------------------------------------------------------
// path clearance (the definition: file header)
// ---------------------------------------------------------------------------------------
constexpr int kPathsPerBlock = kBlock / 64;
constexpr int kMinSamples = 2, kMaxSamples = 4096;
constexpr int64_t kMaxPaths = int64_t(1) << 30;       // blocks stay far below 2^31

struct PathArgs {
  ClrArgs t;                    // the tree's part (nodes .. scene_hi); nothing else of it is read
  int64_t n_paths;
  int n_samples;
  double radius2, max_dist2;
  // explicit paths, indexed by the path i
  const double *coeffs;         // [n][6][3]
  const double *t_range;        // planar [2][n]
  const double *origin;         // planar [3][n] or NULL
  const double *rot;            // planar [9][n] or NULL
  // plans of the engine's vehicles first + i
  const afe_plan_output *plans; // [n]
  const void *pos, *att;        // the engine's slabs: planar, `stride` elements between components
  const double *anchor_xy;
  int64_t stride, first;
  int elem_size;                // 4 or 8
  double mount[4];
  afe_path_clearance *out;      // [n]
  unsigned long long *n_colliding;   // one word, or NULL
  unsigned long long *stats;    // counting build: [0] nodes visited, [1] triangle box tests, [2] fp64 evaluations
};

// sample k of K: its time and its world point
__host__ __device__ __forceinline__ void path_sample(const double (&c)[18], double tb, double te, bool has_o, const double (&o)[3], bool has_r,
                                                     const double (&R)[9], int k, int K, double &t, double &wx, double &wy, double &wz) {
#pragma clang fp contract(off)
  t = k == K - 1 ? te : tb + (te - tb) * ((double)k / (double)(K - 1));
  double p[3];
  for (int a = 0; a < 3; a++) {
    double v = c[a];
    for (int j = 1; j < 6; j++) v = v * t + c[3 * j + a];
    p[a] = v;
  }
  if (has_r) {
    wx = o[0] + ((R[0] * p[0] + R[1] * p[1]) + R[2] * p[2]);
    wy = o[1] + ((R[3] * p[0] + R[4] * p[1]) + R[5] * p[2]);
    wz = o[2] + ((R[6] * p[0] + R[7] * p[1]) + R[8] * p[2]);
  } else if (has_o) {
    wx = o[0] + p[0]; wy = o[1] + p[1]; wz = o[2] + p[2];
  } else {
    wx = p[0]; wy = p[1]; wz = p[2];
  }
}

// smallest (d, l) of the wave in every lane; among equal d the lowest l.  Every lane of the wave takes part.
__device__ __forceinline__ void wave_min_d2_lane(double &d, int &l) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double od = __shfl_xor(d, off);
    const int ol = __shfl_xor(l, off);
    if (od < d || (od == d && ol < l)) { d = od; l = ol; }
  }
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}

// The kernel's arguments, read where they are used.  Held in scalar registers from the kernel's entry to its end, the two
// dozen that only the top of a batch or the record's store needs would push the walk's working set into spills; behind a
// pointer the compiler cannot see through, each is a scalar load from the (cached) argument segment at its use.
__device__ __forceinline__ const PathArgs &path_args() {
#if defined(__HIP_DEVICE_COMPILE__)
  auto p = __builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const PathArgs *)p;
#else
  __builtin_unreachable();      // (the host pass only parses device code)
#endif
}

template <bool ENGINE, bool COUNT>
__global__ void __launch_bounds__(kBlock) afe_path_clearance_kernel(PathArgs) {      // the one argument: offset 0 of the segment
#pragma clang fp contract(off)
  __shared__ uint32_t stack[kStack][kBlock];
  const PathArgs &a0 = path_args();
  const int col = threadIdx.x, lane = col & 63;
  const int64_t path = (int64_t)blockIdx.x * kPathsPerBlock + __builtin_amdgcn_readfirstlane(col >> 6);
  if (path >= a0.n_paths) return;         // a wave without a path falls through (no barrier below)
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const int K = a0.n_samples;
  const bool sampled = ENGINE ? a0.plans[path].found != 0 : true;
  double best = a0.max_dist2;             // wave-uniform: the smallest d2 of the batches so far
  int k_min = -1, tri_min = -1, k_first = -1, tri_first = -1, n_hit = 0, n_nonfinite = 0;
  double cx = nan, cy = nan, cz = nan, t_min = nan, t_first = nan;
  unsigned n_nodes = 0, n_box = 0, n_eval = 0;
  for (int base = 0; sampled && base < K; base += 64) {       // at most 64 batches
    const int k = base + lane;
    const bool valid = k < K;
    // The path's 30-odd wave-uniform values are fetched again for every batch (scalar loads that hit the cache; the pose is a
    // few dozen operations) instead of being held across the walk, for the same reason as the arguments.
    const PathArgs &a = path_args();
    const int64_t pi = path;
    double c[18], o[3] = {0.0, 0.0, 0.0}, R[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double tb, te;
    bool has_o, has_r;
    if (ENGINE) {
      const afe_plan_output *plan = a.plans + pi;
      const double *src = &plan->coeffs[0][0];
#pragma unroll
      for (int j = 0; j < 18; j++) c[j] = src[j];
      tb = 0.0; te = plan->tf;
      has_o = true; has_r = true;
      afe::camera_pose(a.pos, a.att, a.anchor_xy, a.stride, a.elem_size, a.mount, a.first + pi, o, R);
    } else {
      const double *src = a.coeffs + 18 * pi;
#pragma unroll
      for (int j = 0; j < 18; j++) c[j] = src[j];
      tb = a.t_range[pi]; te = a.t_range[a.n_paths + pi];
      has_o = a.origin != nullptr; has_r = a.rot != nullptr;
      if (has_o) {
#pragma unroll
        for (int j = 0; j < 3; j++) o[j] = a.origin[j * a.n_paths + pi];
      }
      if (has_r) {
#pragma unroll
        for (int j = 0; j < 9; j++) R[j] = a.rot[j * a.n_paths + pi];
      }
    }
    double t, wx, wy, wz;
    path_sample(c, tb, te, has_o, o, has_r, R, valid ? k : K - 1, K, t, wx, wy, wz);
    const bool finite = __builtin_isfinite(wx) && __builtin_isfinite(wy) && __builtin_isfinite(wz);
    Best b;
    b.d2 = fmax(a.radius2, best); b.idx = 0x7fffffff; b.cx = nan; b.cy = nan; b.cz = nan;
    if (valid && finite) clr_walk<COUNT>(a.t, wx, wy, wz, b, stack, col, n_nodes, n_box, n_eval);
    const bool found = b.idx != 0x7fffffff;             // then b.d2 is this sample's own d2, b.idx and b.c its own winner
    // hits: ballot, first set bit, popcount
    const unsigned long long hits = __ballot(found && b.d2 <= path_args().radius2);
    const int first_lane = hits ? __ffsll((long long)hits) - 1 : 0;
    const int tri_at = __shfl(b.idx, first_lane);
    const double t_at = __shfl(t, first_lane);
    if (hits && k_first < 0) { k_first = base + first_lane; tri_first = tri_at; t_first = t_at; }
    n_hit += __popcll(hits);
    n_nonfinite += __popcll(__ballot(valid && !finite));
    // closest approach: (d2, lane) of the batch, then against the batches before (a tie loses: its k is higher)
    const bool cand = found && b.d2 <= best;
    double md = cand ? b.d2 : inf;
    int ml = cand ? lane : 64;
    wave_min_d2_lane(md, ml);
    const int src_lane = ml & 63;
    const int tri_w = __shfl(b.idx, src_lane);
    const double cx_w = __shfl(b.cx, src_lane), cy_w = __shfl(b.cy, src_lane), cz_w = __shfl(b.cz, src_lane), t_w = __shfl(t, src_lane);
    if (ml < 64 && (md < best || k_min < 0)) {
      best = md; k_min = base + ml; tri_min = tri_w; cx = cx_w; cy = cy_w; cz = cz_w; t_min = t_w;
    }
  }
  const PathArgs &a = path_args();
  if (lane == 0) {
    afe_path_clearance *r = a.out + path;
    r->min_dist2 = k_min >= 0 ? best : inf;
    r->closest[0] = cx; r->closest[1] = cy; r->closest[2] = cz;
    r->t_min = t_min;
    r->t_first_hit = t_first;
    r->k_min = k_min; r->tri_min = tri_min;
    r->k_first_hit = k_first; r->tri_first_hit = tri_first;
    r->n_hit = n_hit; r->n_nonfinite = n_nonfinite;
    if (a.n_colliding && n_hit > 0) atomicAdd(a.n_colliding, 1ull);      // one integer vector atomic per colliding path
  }
  if (COUNT) {
    const unsigned long long s0 = wave_sum(n_nodes), s1 = wave_sum(n_box), s2 = wave_sum(n_eval);
    if (lane < 3) atomicAdd(a.stats + lane, lane == 0 ? s0 : (lane == 1 ? s1 : s2));
  }
}

// The swept audit: afe_path_clearance_kernel's structure with one CHORD (w_k, w_k+1) per lane, K - 1 chords.  PathArgs is the
// sampled kernel's, unchanged; `out` points at afe_path_sweep records here.
template <bool ENGINE, bool COUNT>
__global__ void __launch_bounds__(kBlock) afe_path_sweep_kernel(PathArgs) {      // the one argument: offset 0 of the segment
#pragma clang fp contract(off)
  __shared__ uint32_t stack[kStack][kBlock];
  const PathArgs &a0 = path_args();
  const int col = threadIdx.x, lane = col & 63;
  const int64_t path = (int64_t)blockIdx.x * kPathsPerBlock + __builtin_amdgcn_readfirstlane(col >> 6);
  if (path >= a0.n_paths) return;         // a wave without a path falls through (no barrier below)
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const int K = a0.n_samples;
  const bool sampled = ENGINE ? a0.plans[path].found != 0 : true;
  double best = a0.max_dist2;             // wave-uniform: the smallest d2 of the batches so far
  int k_min = -1, tri_min = -1, k_first = -1, tri_first = -1, n_hit = 0, n_nonfinite = 0;
  double cx = nan, cy = nan, cz = nan, t_min = nan, t_first = nan, s_min = nan, s_first = nan;
  unsigned n_nodes = 0, n_box = 0, n_eval = 0;
  for (int base = 0; sampled && base < K - 1; base += 64) {   // at most 64 batches
    const int k = base + lane;
    const bool valid = k < K - 1;
    const PathArgs &a = path_args();      // fetched again for every batch, as in the sampled kernel
    const int64_t pi = path;
    double c[18], o[3] = {0.0, 0.0, 0.0}, R[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double tb, te;
    bool has_o, has_r;
    if (ENGINE) {
      const afe_plan_output *plan = a.plans + pi;
      const double *src = &plan->coeffs[0][0];
#pragma unroll
      for (int j = 0; j < 18; j++) c[j] = src[j];
      tb = 0.0; te = plan->tf;
      has_o = true; has_r = true;
      afe::camera_pose(a.pos, a.att, a.anchor_xy, a.stride, a.elem_size, a.mount, a.first + pi, o, R);
    } else {
      const double *src = a.coeffs + 18 * pi;
#pragma unroll
      for (int j = 0; j < 18; j++) c[j] = src[j];
      tb = a.t_range[pi]; te = a.t_range[a.n_paths + pi];
      has_o = a.origin != nullptr; has_r = a.rot != nullptr;
      if (has_o) {
#pragma unroll
        for (int j = 0; j < 3; j++) o[j] = a.origin[j * a.n_paths + pi];
      }
      if (has_r) {
#pragma unroll
        for (int j = 0; j < 9; j++) R[j] = a.rot[j * a.n_paths + pi];
      }
    }
    const int kk = valid ? k : K - 2;
    double t0, t1, w0x, w0y, w0z, w1x, w1y, w1z;
    path_sample(c, tb, te, has_o, o, has_r, R, kk, K, t0, w0x, w0y, w0z);
    path_sample(c, tb, te, has_o, o, has_r, R, kk + 1, K, t1, w1x, w1y, w1z);
    const bool finite = __builtin_isfinite(w0x) && __builtin_isfinite(w0y) && __builtin_isfinite(w0z) && __builtin_isfinite(w1x) &&
                        __builtin_isfinite(w1y) && __builtin_isfinite(w1z);
    SegBest b;
    b.d2 = fmax(a.radius2, best); b.s = nan; b.idx = 0x7fffffff; b.kind = -1; b.cx = nan; b.cy = nan; b.cz = nan;
    if (valid && finite) seg_walk<COUNT>(a.t, w0x, w0y, w0z, w1x, w1y, w1z, b, stack, col, n_nodes, n_box, n_eval);
    const bool found = b.idx != 0x7fffffff;             // then b is this chord's own answer
    const double t = t0 + (t1 - t0) * b.s;              // the time of the chord's closest point
    const unsigned long long hits = __ballot(found && b.d2 <= path_args().radius2);
    const int first_lane = hits ? __ffsll((long long)hits) - 1 : 0;
    const int tri_at = __shfl(b.idx, first_lane);
    const double t_at = __shfl(t, first_lane), s_at = __shfl(b.s, first_lane);
    if (hits && k_first < 0) { k_first = base + first_lane; tri_first = tri_at; t_first = t_at; s_first = s_at; }
    n_hit += __popcll(hits);
    n_nonfinite += __popcll(__ballot(valid && !finite));
    const bool cand = found && b.d2 <= best;
    double md = cand ? b.d2 : inf;
    int ml = cand ? lane : 64;
    wave_min_d2_lane(md, ml);
    const int src_lane = ml & 63;
    const int tri_w = __shfl(b.idx, src_lane);
    const double cx_w = __shfl(b.cx, src_lane), cy_w = __shfl(b.cy, src_lane), cz_w = __shfl(b.cz, src_lane);
    const double t_w = __shfl(t, src_lane), s_w = __shfl(b.s, src_lane);
    if (ml < 64 && (md < best || k_min < 0)) {
      best = md; k_min = base + ml; tri_min = tri_w; cx = cx_w; cy = cy_w; cz = cz_w; t_min = t_w; s_min = s_w;
    }
  }
  const PathArgs &a = path_args();
  if (lane == 0) {
    afe_path_sweep *r = (afe_path_sweep *)a.out + path;
    r->min_dist2 = k_min >= 0 ? best : inf;
    r->closest[0] = cx; r->closest[1] = cy; r->closest[2] = cz;
    r->t_min = t_min;
    r->t_first_hit = t_first;
    r->k_min = k_min; r->tri_min = tri_min;
    r->k_first_hit = k_first; r->tri_first_hit = tri_first;
    r->n_hit = n_hit; r->n_nonfinite = n_nonfinite;
    r->s_min = s_min; r->s_first_hit = s_first;
    if (a.n_colliding && n_hit > 0) atomicAdd(a.n_colliding, 1ull);
  }
  if (COUNT) {
    const unsigned long long s0 = wave_sum(n_nodes), s1 = wave_sum(n_box), s2 = wave_sum(n_eval);
    if (lane < 3) atomicAdd(a.stats + lane, lane == 0 ? s0 : (lane == 1 ? s1 : s2));
  }
}

// ---------------------------------------------------------------------------------------
// host: the hierarchy
// ---------------------------------------------------------------------------------------
struct FBox {
  float lo[3], hi[3];
  void reset() { for (int k = 0; k < 3; k++) { lo[k] = std::numeric_limits<float>::infinity(); hi[k] = -lo[k]; } }
  void grow(const float *p) { for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], p[k]); hi[k] = std::max(hi[k], p[k]); } }
  void grow(const FBox &o) { grow(o.lo); grow(o.hi); }
  double half_area() const {
    const double x = (double)hi[0] - lo[0], y = (double)hi[1] - lo[1], z = (double)hi[2] - lo[2];
    return x * y + y * z + z * x;
  }
  bool holds(const float *p) const { for (int k = 0; k < 3; k++) if (!(p[k] >= lo[k] && p[k] <= hi[k])) return false; return true; }
  bool holds(const FBox &o) const { return holds(o.lo) && holds(o.hi); }
};

// the definition's flag, in the definition's operation order
int degenerate_flag(const double ab[3], const double ac[3]) {
#pragma clang fp contract(off)
  const double n0 = ab[1] * ac[2] - ab[2] * ac[1], n1 = ab[2] * ac[0] - ab[0] * ac[2], n2 = ab[0] * ac[1] - ab[1] * ac[0];
  const double nn = n0 * n0 + n1 * n1 + n2 * n2;
  const double l_ab = ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2], l_ac = ac[0] * ac[0] + ac[1] * ac[1] + ac[2] * ac[2];
  return nn > 1e-24 * (l_ab * l_ac) ? 0 : 1;
}

struct HostMap {
  const float *tri = nullptr;       // the caller's triangles
  int64_t n_tri = 0, n_small = 0;
  std::vector<int32_t> order;       // leaf order -> input index: the tree's triangles, then the ones kept out of it
  std::vector<CNode> nodes;
  uint32_t root_ref = kNone;
  FBox root_box, scene;
  int depth = 0, max_leaf = 0;

  FBox tri_box(int32_t t) const {
    FBox b; b.reset();
    for (int v = 0; v < 3; v++) b.grow(tri + 9 * (int64_t)t + 3 * v);
    return b;
  }
  double centroid(int32_t t, int axis) const {
    const float *p = tri + 9 * (int64_t)t;
    return ((double)p[axis] + (double)p[3 + axis]) + (double)p[6 + axis];
  }
  uint32_t build_range(int64_t lo, int64_t hi, int level, FBox &box) {
    depth = std::max(depth, level);
    box.reset();
    for (int64_t k = lo; k < hi; k++) box.grow(tri_box(order[(size_t)k]));
    if (hi - lo <= kLeafMax) {
      max_leaf = std::max(max_leaf, (int)(hi - lo));
      return kLeafBit | ((uint32_t)(hi - lo) << 28) | (uint32_t)lo;
    }
    double clo[3], chi[3];
    for (int a = 0; a < 3; a++) { clo[a] = std::numeric_limits<double>::infinity(); chi[a] = -clo[a]; }
    for (int64_t k = lo; k < hi; k++)
      for (int a = 0; a < 3; a++) { const double c = centroid(order[(size_t)k], a); clo[a] = std::min(clo[a], c); chi[a] = std::max(chi[a], c); }
    int axis = 0;
    for (int a = 1; a < 3; a++) if (chi[a] - clo[a] > chi[axis] - clo[axis]) axis = a;
    // median by count: balanced whatever the centroids are (all coincident: the split is by input index)
    const int64_t mid = lo + (hi - lo) / 2;
    std::nth_element(order.begin() + lo, order.begin() + mid, order.begin() + hi, [&](int32_t x, int32_t y) {
      const double cx = centroid(x, axis), cy = centroid(y, axis);
      return cx < cy || (cx == cy && x < y);
    });
    const size_t me = nodes.size();
    nodes.push_back(CNode());
    FBox b0, b1;
    const uint32_t r0 = build_range(lo, mid, level + 1, b0);
    const uint32_t r1 = build_range(mid, hi, level + 1, b1);
    CNode &nd = nodes[me];
    std::memset(&nd, 0, sizeof(nd));
    for (int k = 0; k < 3; k++) { nd.c[0].lo[k] = b0.lo[k]; nd.c[0].hi[k] = b0.hi[k]; nd.c[1].lo[k] = b1.lo[k]; nd.c[1].hi[k] = b1.hi[k]; }
    nd.c[0].ref = r0;
    nd.c[1].ref = r1;
    return (uint32_t)me;
  }

  int build(const float *triangles, int64_t n) {
    tri = triangles; n_tri = n;
    scene.reset();
    for (int64_t i = 0; i < 3 * n; i++) scene.grow(triangles + 3 * i);
    std::vector<int32_t> small_ix, big_ix;
    const double scene_area = scene.half_area();
    for (int64_t i = 0; i < n; i++) (tri_box((int32_t)i).half_area() > 0.25 * scene_area ? big_ix : small_ix).push_back((int32_t)i);
    if ((int)big_ix.size() > kMaxBig || small_ix.empty()) {   // nothing special about this mesh: everything into the tree
      small_ix.resize((size_t)n);
      for (int64_t i = 0; i < n; i++) small_ix[(size_t)i] = (int32_t)i;
      big_ix.clear();
    }
    n_small = (int64_t)small_ix.size();
    order = small_ix;
    nodes.clear(); depth = 0; max_leaf = 0;
    root_ref = build_range(0, n_small, 1, root_box);
    order.insert(order.end(), big_ix.begin(), big_ix.end());
    return depth <= kStack ? AFE_OK : AFE_ERR_OUT_OF_RANGE;
  }

  // every triangle in exactly one leaf (or once in the out-of-tree list), every box holding what hangs below it
  bool verify_ref(uint32_t ref, const FBox &box, int level, std::vector<int> &seen, int &deepest) const {
    deepest = std::max(deepest, level);
    if (level > kStack) return false;
    if (ref & kLeafBit) {
      const int64_t first = ref & kFirstMask, cnt = (ref >> 28) & 7u;
      if (cnt < 1 || cnt > kLeafMax || first + cnt > n_small) return false;
      for (int64_t k = first; k < first + cnt; k++) {
        const int32_t t = order[(size_t)k];
        seen[(size_t)t]++;
        if (!box.holds(tri_box(t))) return false;
      }
      return true;
    }
    if (ref >= nodes.size()) return false;
    const CNode &nd = nodes[ref];
    for (int c = 0; c < 2; c++) {
      FBox cb;
      for (int k = 0; k < 3; k++) { cb.lo[k] = nd.c[c].lo[k]; cb.hi[k] = nd.c[c].hi[k]; }
      if (!box.holds(cb) || !verify_ref(nd.c[c].ref, cb, level + 1, seen, deepest)) return false;
    }
    return true;
  }
  bool verify() const {
    std::vector<int> seen((size_t)n_tri, 0);
    int deepest = 0;
    if (!scene.holds(root_box) || !verify_ref(root_ref, root_box, 1, seen, deepest) || deepest != depth) return false;
    for (int64_t k = n_small; k < n_tri; k++) seen[(size_t)order[(size_t)k]]++;
    for (int64_t t = 0; t < n_tri; t++) if (seen[(size_t)t] != 1) return false;
    return true;
  }

  std::vector<CTri> pack() const {
    std::vector<CTri> out((size_t)n_tri);
    for (int64_t k = 0; k < n_tri; k++) {
      const int32_t t = order[(size_t)k];
      const float *src = tri + 9 * (int64_t)t;
      CTri &T = out[(size_t)k];
      std::memset(&T, 0, sizeof(T));
      const FBox tb = tri_box(t);
      for (int a = 0; a < 3; a++) {
        T.lo[a] = tb.lo[a]; T.hi[a] = tb.hi[a];
        T.a[a] = (double)src[a];
        T.ab[a] = (double)src[3 + a] - T.a[a];
        T.ac[a] = (double)src[6 + a] - T.a[a];
      }
      T.index = t;
      T.degenerate = degenerate_flag(T.ab, T.ac);
    }
    return out;
  }
};

bool mesh_ok(const float *triangles, int64_t n_tri) {
  if (!triangles || n_tri <= 0 || n_tri > kMaxTri) return false;
  for (int64_t i = 0; i < 9 * n_tri; i++) if (!std::isfinite(triangles[i])) return false;
  return true;
}

}  // namespace

// (struct afe_clearance_map: afe_clearance_map.h)

struct afe_contact_monitor {
  afe_engine *engine = nullptr;        // borrowed
  afe_clearance_map *map = nullptr;    // borrowed
  int64_t n = 0;
  int device = 0;
  double contact2 = 0, search2 = 0;
  DevBuf min_dist2, first_us, first_tri;      // double, uint64, int32 per vehicle
  DevBuf counts;                              // two unsigned long long
  PinnedBuf<> counts_host;                    // the same
  // the swept monitor only: every vehicle's position as its last update formed it, planar double [3][n], and whether there is one (uint32)
  DevBuf prev, prev_valid;
};

namespace {

// launches the query for `count` points on `stream`, in runs below 2^31 threads
template <bool MONITOR, bool COUNT>
int launch_query(ClrArgs g, hipStream_t stream, float *kernel_ms) {
  StreamTimer timer(stream, kernel_ms != nullptr);
  if (!timer.ok()) return AFE_ERR_HIP;
  int rc = AFE_OK;
  const int64_t total = g.count, first = g.first;
  double *d2 = g.dist2_out, *cl = g.closest_out;
  int32_t *ti = g.tri_out;
  for (int64_t done = 0; done < total && rc == AFE_OK; done += kPointsPerLaunch) {
    const int64_t n = std::min(total - done, kPointsPerLaunch);
    g.first = first + done;
    g.count = n;
    g.dist2_out = d2 ? d2 + done : nullptr;
    g.tri_out = ti ? ti + done : nullptr;
    g.closest_out = cl ? cl + done : nullptr;
    hipLaunchKernelGGL((afe_clearance_kernel<MONITOR, COUNT>), dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, g);
    rc = hipGetLastError() == hipSuccess ? AFE_OK : AFE_ERR_HIP;
  }
  return timer.finish(rc, kernel_ms);
}

bool radius_ok(double max_dist) { return max_dist > 0.0; }   // false for NaN, 0, negatives; +inf passes

int query_points(afe_clearance_map *m, int64_t n_points, const double *pos, double max_dist, double *dist2_out, int32_t *tri_out,
                 double *closest_out, float *kernel_ms, uint64_t *stats) {
  if (hipSetDevice(m->device) != hipSuccess) return AFE_ERR_HIP;
  const size_t n = (size_t)n_points;
  DevBuf d_pos, d_d2, d_tri, d_cl, d_stats;
  if (!d_pos.upload(pos, n * 24) || !d_d2.alloc(n * 8) || !d_tri.alloc(n * 4) || (closest_out && !d_cl.alloc(n * 24)) || (stats && !d_stats.alloc(24))) {
    (void)hipGetLastError();
    return AFE_ERR_HIP;
  }
  if (stats && hipMemset(d_stats.get(), 0, 24) != hipSuccess) return AFE_ERR_HIP;
  ClrArgs g = m->base;
  g.max_dist2 = max_dist * max_dist;
  g.pos = d_pos.get(); g.anchor_xy = nullptr; g.stride = n_points; g.first = 0; g.count = n_points; g.elem_size = 8;
  g.dist2_out = (double *)d_d2.get(); g.tri_out = (int32_t *)d_tri.get(); g.closest_out = (double *)d_cl.get(); g.out_stride = n_points;
  g.stats = (unsigned long long *)d_stats.get();
  float ms = 0;
  const int rc = stats ? launch_query<false, true>(g, nullptr, &ms) : launch_query<false, false>(g, nullptr, &ms);
  if (rc != AFE_OK) return rc;
  if (kernel_ms) *kernel_ms = ms;
  if (!d_d2.download(dist2_out, n * 8) || !d_tri.download(tri_out, n * 4) || (closest_out && !d_cl.download(closest_out, n * 24))) return AFE_ERR_HIP;
  if (stats) {
    unsigned long long host[3];
    if (!d_stats.download(host, 24)) return AFE_ERR_HIP;
    for (int k = 0; k < 3; k++) stats[k] = host[k];
    stats[3] = (uint64_t)n_points;
  }
  return AFE_OK;
}

// the swept kernel for g.count segments on `stream`, in runs below 2^31 threads
template <bool MONITOR, bool COUNT>
int launch_swept(SegArgs a, hipStream_t stream, float *kernel_ms) {
  StreamTimer timer(stream, kernel_ms != nullptr);
  if (!timer.ok()) return AFE_ERR_HIP;
  int rc = AFE_OK;
  const int64_t total = a.g.count, first = a.g.first;
  afe_segment_clearance *out = a.out;
  for (int64_t done = 0; done < total && rc == AFE_OK; done += kPointsPerLaunch) {
    const int64_t n = std::min(total - done, kPointsPerLaunch);
    a.g.first = first + done;
    a.g.count = n;
    a.out = out ? out + done : nullptr;
    hipLaunchKernelGGL((afe_swept_kernel<MONITOR, COUNT>), dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, a);
    rc = hipGetLastError() == hipSuccess ? AFE_OK : AFE_ERR_HIP;
  }
  return timer.finish(rc, kernel_ms);
}

int query_segments(afe_clearance_map *m, int64_t n_seg, const double *p0, const double *p1, double max_dist, afe_segment_clearance *out,
                   float *kernel_ms, uint64_t *stats) {
  if (hipSetDevice(m->device) != hipSuccess) return AFE_ERR_HIP;
  const size_t n = (size_t)n_seg;
  DevBuf d_p0, d_p1, d_out, d_stats;
  if (!d_p0.upload(p0, n * 24) || !d_p1.upload(p1, n * 24) || (out && !d_out.alloc(n * sizeof(afe_segment_clearance))) || (stats && !d_stats.alloc(24))) {
    (void)hipGetLastError();
    return AFE_ERR_HIP;
  }
  if (stats && hipMemset(d_stats.get(), 0, 24) != hipSuccess) return AFE_ERR_HIP;
  SegArgs a;
  std::memset(&a, 0, sizeof(a));
  a.g = m->base;
  a.g.max_dist2 = max_dist * max_dist;
  a.g.pos = d_p1.get(); a.g.anchor_xy = nullptr; a.g.stride = n_seg; a.g.first = 0; a.g.count = n_seg; a.g.elem_size = 8;
  a.g.stats = (unsigned long long *)d_stats.get();
  a.p0 = (const double *)d_p0.get();
  a.out = (afe_segment_clearance *)d_out.get();
  float ms = 0;
  const int rc = stats ? launch_swept<false, true>(a, nullptr, &ms) : launch_swept<false, false>(a, nullptr, &ms);
  if (rc != AFE_OK) return rc;
  if (kernel_ms) *kernel_ms = ms;
  if (out && !d_out.download(out, n * sizeof(afe_segment_clearance))) return AFE_ERR_HIP;
  if (stats) {
    unsigned long long host[3];
    if (!d_stats.download(host, 24)) return AFE_ERR_HIP;
    for (int k = 0; k < 3; k++) stats[k] = host[k];
    stats[3] = (uint64_t)n_seg;
  }
  return AFE_OK;
}

}  // namespace

extern "C" int afe_clearance_map_create(int device, const float *triangles, int64_t n_tri, afe_clearance_map **out) {
  if (!out || !mesh_ok(triangles, n_tri)) return AFE_ERR_INVALID_ARG;
  int dev = 0;
  int rc = afe::pick_gfx950(device, &dev);
  if (rc != AFE_OK) return rc;
  HostMap h;
  rc = h.build(triangles, n_tri);
  if (rc != AFE_OK) return rc;
  const std::vector<CTri> packed = h.pack();
  afe_clearance_map *m = new afe_clearance_map();
  m->device = dev;
  m->n_tri = n_tri;
  m->n_nodes = (int64_t)h.nodes.size();
  m->depth = h.depth;
  for (int k = 0; k < 3; k++) { m->bounds[k] = h.scene.lo[k]; m->bounds[3 + k] = h.scene.hi[k]; }
  const size_t node_bytes = std::max<size_t>(h.nodes.size(), 1) * sizeof(CNode);
  if (!m->nodes.alloc(node_bytes) || !m->tris.alloc(packed.size() * sizeof(CTri)) ||
      (!h.nodes.empty() && hipMemcpy(m->nodes.get(), h.nodes.data(), h.nodes.size() * sizeof(CNode), hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemcpy(m->tris.get(), packed.data(), packed.size() * sizeof(CTri), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    (void)afe_clearance_map_destroy(m);
    return AFE_ERR_HIP;
  }
  ClrArgs &g = m->base;
  std::memset(&g, 0, sizeof(g));
  g.nodes = m->nodes.as<CNode>(); g.tris = m->tris.as<CTri>();
  g.root_ref = h.root_ref;
  g.big_first = (uint32_t)h.n_small; g.n_big = (uint32_t)(n_tri - h.n_small);
  for (int k = 0; k < 3; k++) {
    g.root_lo[k] = h.root_box.lo[k]; g.root_hi[k] = h.root_box.hi[k];
    g.scene_lo[k] = (double)h.scene.lo[k]; g.scene_hi[k] = (double)h.scene.hi[k];
  }
  *out = m;
  return AFE_OK;
}

extern "C" int afe_clearance_map_destroy(afe_clearance_map *m) {
  if (!m) return AFE_ERR_INVALID_ARG;
  (void)hipSetDevice(m->device);
  (void)hipDeviceSynchronize();      // a query on some stream may still be reading the tables
  delete m;
  return AFE_OK;
}

extern "C" int afe_clearance_map_info(const afe_clearance_map *m, int64_t *n_tri, int64_t *n_nodes, int *depth, double bounds[6]) {
  if (!m) return AFE_ERR_INVALID_ARG;
  if (n_tri) *n_tri = m->n_tri;
  if (n_nodes) *n_nodes = m->n_nodes;
  if (depth) *depth = m->depth;
  if (bounds) for (int k = 0; k < 6; k++) bounds[k] = m->bounds[k];
  return AFE_OK;
}

extern "C" int afe_clearance_check_hierarchy(const float *triangles, int64_t n_tri, int64_t *n_nodes, int *depth, int *max_leaf) {
  if (!mesh_ok(triangles, n_tri)) return AFE_ERR_INVALID_ARG;
  HostMap h;
  const int rc = h.build(triangles, n_tri);
  if (rc != AFE_OK) return rc;
  if (!h.verify()) return AFE_ERR_OUT_OF_RANGE;
  if (n_nodes) *n_nodes = (int64_t)h.nodes.size();
  if (depth) *depth = h.depth;
  if (max_leaf) *max_leaf = h.max_leaf;
  return AFE_OK;
}

extern "C" int afe_clearance_query(afe_clearance_map *m, int64_t n_points, const double *pos, double max_dist, double *dist2_out,
                                   int32_t *tri_out, double *closest_out, float *kernel_ms) {
  if (!m || n_points < 0 || !pos || !dist2_out || !tri_out || !radius_ok(max_dist)) return AFE_ERR_INVALID_ARG;
  if (n_points > kMaxPoints) return AFE_ERR_OUT_OF_RANGE;
  if (n_points == 0) return AFE_OK;
  return query_points(m, n_points, pos, max_dist, dist2_out, tri_out, closest_out, kernel_ms, nullptr);
}

extern "C" int afe_clearance_query_stats(afe_clearance_map *m, int64_t n_points, const double *pos, double max_dist, uint64_t stats[4],
                                         float *kernel_ms) {
  if (!m || n_points <= 0 || !pos || !stats || !radius_ok(max_dist)) return AFE_ERR_INVALID_ARG;
  if (n_points > kMaxPoints) return AFE_ERR_OUT_OF_RANGE;
  std::vector<double> d2((size_t)n_points);
  std::vector<int32_t> ti((size_t)n_points);
  return query_points(m, n_points, pos, max_dist, d2.data(), ti.data(), nullptr, kernel_ms, stats);
}

extern "C" int afe_clearance_segments(afe_clearance_map *m, int64_t n, const double *p0, const double *p1, double max_dist,
                                      afe_segment_clearance *out, float *kernel_ms) {
  if (!m || n < 0 || !p0 || !p1 || !out || !radius_ok(max_dist)) return AFE_ERR_INVALID_ARG;
  if (n > kMaxPoints) return AFE_ERR_OUT_OF_RANGE;
  if (n == 0) return AFE_OK;
  return query_segments(m, n, p0, p1, max_dist, out, kernel_ms, nullptr);
}

extern "C" int afe_clearance_segments_stats(afe_clearance_map *m, int64_t n, const double *p0, const double *p1, double max_dist, uint64_t stats[4],
                                            float *kernel_ms) {
  if (!m || n <= 0 || !p0 || !p1 || !stats || !radius_ok(max_dist)) return AFE_ERR_INVALID_ARG;
  if (n > kMaxPoints) return AFE_ERR_OUT_OF_RANGE;
  return query_segments(m, n, p0, p1, max_dist, nullptr, kernel_ms, stats);
}

extern "C" int afe_clearance_query_engine(afe_engine *e, afe_clearance_map *m, int64_t first, int64_t count, double max_dist, void *dist2_out,
                                          void *tri_out, void *closest_out, int out_is_device, float *kernel_ms) {
  if (!e || !m || first < 0 || count < 0 || !radius_ok(max_dist)) return AFE_ERR_INVALID_ARG;
  if (count > 0 && (!dist2_out || !tri_out)) return AFE_ERR_INVALID_ARG;
  if (afe::engine_range_bad(e, first, count)) return AFE_ERR_OUT_OF_RANGE;
  if (count == 0) return AFE_OK;          // a valid range of nothing: answered before the engine is touched
  EngineAccess acc;
  int rc = afe::engine_enter(e, &acc);     // (ends a resident grid, as the camera does)
  if (rc != AFE_OK) return rc;
  if (acc.device != m->device) return AFE_ERR_INVALID_ARG;
  const afe_device_view &view = acc.view;
  const size_t n = (size_t)count;
  DevBuf d_d2, d_tri, d_cl;
  ClrArgs g = m->base;
  g.max_dist2 = max_dist * max_dist;
  g.pos = view.pos; g.anchor_xy = view.pos_anchor_xy; g.stride = view.stride; g.first = first; g.count = count; g.elem_size = view.state_elem_size;
  g.out_stride = count;
  if (out_is_device) {
    g.dist2_out = (double *)dist2_out; g.tri_out = (int32_t *)tri_out; g.closest_out = (double *)closest_out;
  } else {
    if (!d_d2.alloc(n * 8) || !d_tri.alloc(n * 4) || (closest_out && !d_cl.alloc(n * 24))) { (void)hipGetLastError(); return AFE_ERR_HIP; }
    g.dist2_out = (double *)d_d2.get(); g.tri_out = (int32_t *)d_tri.get(); g.closest_out = (double *)d_cl.get();
  }
  float ms = 0;
  rc = launch_query<false, false>(g, acc.stream, &ms);     // synchronises (timing)
  if (rc != AFE_OK) return rc;
  if (kernel_ms) *kernel_ms = ms;
  if (!out_is_device && (!d_d2.download(dist2_out, n * 8) || !d_tri.download(tri_out, n * 4) || (closest_out && !d_cl.download(closest_out, n * 24))))
    return AFE_ERR_HIP;
  return AFE_OK;
}

// ---------------------------------------------------------------------------------------
// path clearance
// ---------------------------------------------------------------------------------------
namespace {

bool path_radii_ok(double radius, double max_dist) { return radius > 0.0 && std::isfinite(radius) && radius <= max_dist; }   // NaN fails; +inf max_dist passes
bool path_samples_ok(int n_samples) { return n_samples >= kMinSamples && n_samples <= kMaxSamples; }

// one launch on `stream`; with kernel_ms, waits for it
template <bool ENGINE>
int launch_paths(const PathArgs &a, bool swept, hipStream_t stream, float *kernel_ms) {
  StreamTimer timer(stream, kernel_ms != nullptr);
  if (!timer.ok()) return AFE_ERR_HIP;
  const dim3 grid((unsigned)((a.n_paths + kPathsPerBlock - 1) / kPathsPerBlock)), block(kBlock);
  // path_args() reads the argument segment from offset 0: the kernel takes PathArgs by value and nothing else
  static_assert(std::is_same<decltype(&afe_path_clearance_kernel<ENGINE, false>), void (*)(PathArgs)>::value, "one by-value PathArgs");
  bool counting = false;
  if constexpr (!ENGINE) counting = a.stats != nullptr;        // (the counting build serves explicit paths only)
  static_assert(std::is_same<decltype(&afe_path_sweep_kernel<ENGINE, false>), void (*)(PathArgs)>::value, "one by-value PathArgs");
  if (swept) {
    if constexpr (!ENGINE) { if (counting) hipLaunchKernelGGL((afe_path_sweep_kernel<false, true>), grid, block, 0, stream, a); }
    if (!counting) hipLaunchKernelGGL((afe_path_sweep_kernel<ENGINE, false>), grid, block, 0, stream, a);
  } else {
    if constexpr (!ENGINE) { if (counting) hipLaunchKernelGGL((afe_path_clearance_kernel<false, true>), grid, block, 0, stream, a); }
    if (!counting) hipLaunchKernelGGL((afe_path_clearance_kernel<ENGINE, false>), grid, block, 0, stream, a);
  }
  return timer.finish(hipGetLastError() == hipSuccess ? AFE_OK : AFE_ERR_HIP, kernel_ms);
}

int paths_args_check(afe_clearance_map *m, int64_t n_paths, const double *coeffs, const double *t_range, const double *origin, const double *rot,
                     int n_samples, double radius, double max_dist) {
  if (!m || n_paths < 0 || !path_radii_ok(radius, max_dist) || (rot && !origin)) return AFE_ERR_INVALID_ARG;
  if (n_paths > 0 && (!coeffs || !t_range)) return AFE_ERR_INVALID_ARG;
  if (!path_samples_ok(n_samples) || n_paths > kMaxPaths) return AFE_ERR_OUT_OF_RANGE;
  return AFE_OK;
}

// explicit paths: uploads the host arrays, downloads the records (out may be NULL: discarded); swept: afe_path_sweep records
int run_paths(afe_clearance_map *m, int64_t n_paths, const double *coeffs, const double *t_range, const double *origin, const double *rot,
              int n_samples, double radius, double max_dist, bool swept, void *out, int64_t *n_colliding, float *kernel_ms, uint64_t *stats) {
  const size_t rec_size = swept ? sizeof(afe_path_sweep) : sizeof(afe_path_clearance);
  if (hipSetDevice(m->device) != hipSuccess) return AFE_ERR_HIP;
  const size_t n = (size_t)n_paths;
  DevBuf d_c, d_t, d_o, d_r, d_out, d_words;
  if (!d_c.upload(coeffs, n * 144) || !d_t.upload(t_range, n * 16) || (origin && !d_o.upload(origin, n * 24)) || (rot && !d_r.upload(rot, n * 72)) ||
      !d_out.alloc(n * rec_size) || !d_words.alloc(32) || hipMemset(d_words.get(), 0, 32) != hipSuccess) {
    (void)hipGetLastError();
    return AFE_ERR_HIP;
  }
  PathArgs a;
  std::memset(&a, 0, sizeof(a));
  a.t = m->base;
  a.n_paths = n_paths; a.n_samples = n_samples;
  a.radius2 = radius * radius; a.max_dist2 = max_dist * max_dist;
  a.coeffs = (const double *)d_c.get(); a.t_range = (const double *)d_t.get(); a.origin = (const double *)d_o.get(); a.rot = (const double *)d_r.get();
  a.out = (afe_path_clearance *)d_out.get();
  a.n_colliding = (unsigned long long *)d_words.get();
  a.stats = stats ? (unsigned long long *)d_words.get() + 1 : nullptr;
  float ms = 0;
  const int rc = launch_paths<false>(a, swept, nullptr, &ms);
  if (rc != AFE_OK) return rc;
  if (kernel_ms) *kernel_ms = ms;
  unsigned long long words[4];
  if ((out && !d_out.download(out, n * rec_size)) || !d_words.download(words, 32)) return AFE_ERR_HIP;
  if (n_colliding) *n_colliding = (int64_t)words[0];
  if (stats) {
    for (int k = 0; k < 3; k++) stats[k] = words[1 + k];
    stats[3] = (uint64_t)n_paths * (uint64_t)(swept ? n_samples - 1 : n_samples);
  }
  return AFE_OK;
}

}  // namespace

extern "C" int afe_path_sample_points(const double *coeffs18, double t_begin, double t_end, const double *origin3, const double *rot9,
                                      int n_samples, double *t_out, double *xyz_out) {
  if (!coeffs18 || !t_out || !xyz_out || (rot9 && !origin3)) return AFE_ERR_INVALID_ARG;
  if (!path_samples_ok(n_samples)) return AFE_ERR_OUT_OF_RANGE;
  double c[18], o[3] = {0.0, 0.0, 0.0}, R[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < 18; k++) c[k] = coeffs18[k];
  if (origin3) for (int k = 0; k < 3; k++) o[k] = origin3[k];
  if (rot9) for (int k = 0; k < 9; k++) R[k] = rot9[k];
  const size_t K = (size_t)n_samples;
  for (int k = 0; k < n_samples; k++)
    path_sample(c, t_begin, t_end, origin3 != nullptr, o, rot9 != nullptr, R, k, n_samples, t_out[k], xyz_out[k], xyz_out[K + k], xyz_out[2 * K + k]);
  return AFE_OK;
}

extern "C" int afe_clearance_paths(afe_clearance_map *m, int64_t n_paths, const double *coeffs, const double *t_range, const double *origin,
                                   const double *rot, int n_samples, double radius, double max_dist, afe_path_clearance *out, int64_t *n_colliding,
                                   float *kernel_ms) {
  const int rc = paths_args_check(m, n_paths, coeffs, t_range, origin, rot, n_samples, radius, max_dist);
  if (rc != AFE_OK) return rc;
  if (n_paths > 0 && !out) return AFE_ERR_INVALID_ARG;
  if (n_paths == 0) { if (n_colliding) *n_colliding = 0; return AFE_OK; }
  return run_paths(m, n_paths, coeffs, t_range, origin, rot, n_samples, radius, max_dist, false, out, n_colliding, kernel_ms, nullptr);
}

extern "C" int afe_clearance_paths_stats(afe_clearance_map *m, int64_t n_paths, const double *coeffs, const double *t_range, const double *origin,
                                         const double *rot, int n_samples, double radius, double max_dist, uint64_t stats[4], float *kernel_ms) {
  const int rc = paths_args_check(m, n_paths, coeffs, t_range, origin, rot, n_samples, radius, max_dist);
  if (rc != AFE_OK) return rc;
  if (n_paths <= 0 || !stats) return AFE_ERR_INVALID_ARG;
  return run_paths(m, n_paths, coeffs, t_range, origin, rot, n_samples, radius, max_dist, false, nullptr, nullptr, kernel_ms, stats);
}

extern "C" int afe_clearance_paths_swept(afe_clearance_map *m, int64_t n_paths, const double *coeffs, const double *t_range, const double *origin,
                                         const double *rot, int n_samples, double radius, double max_dist, afe_path_sweep *out,
                                         int64_t *n_colliding, float *kernel_ms) {
  const int rc = paths_args_check(m, n_paths, coeffs, t_range, origin, rot, n_samples, radius, max_dist);
  if (rc != AFE_OK) return rc;
  if (n_paths > 0 && !out) return AFE_ERR_INVALID_ARG;
  if (n_paths == 0) { if (n_colliding) *n_colliding = 0; return AFE_OK; }
  return run_paths(m, n_paths, coeffs, t_range, origin, rot, n_samples, radius, max_dist, true, out, n_colliding, kernel_ms, nullptr);
}

extern "C" int afe_clearance_paths_swept_stats(afe_clearance_map *m, int64_t n_paths, const double *coeffs, const double *t_range,
                                               const double *origin, const double *rot, int n_samples, double radius, double max_dist,
                                               uint64_t stats[4], float *kernel_ms) {
  const int rc = paths_args_check(m, n_paths, coeffs, t_range, origin, rot, n_samples, radius, max_dist);
  if (rc != AFE_OK) return rc;
  if (n_paths <= 0 || !stats) return AFE_ERR_INVALID_ARG;
  return run_paths(m, n_paths, coeffs, t_range, origin, rot, n_samples, radius, max_dist, true, nullptr, nullptr, kernel_ms, stats);
}

extern "C" int afe_path_chord_deviation(const double *coeffs18, double t_begin, double t_end, const double *rot9, int n_samples, double *bound_m) {
  if (!coeffs18 || !bound_m) return AFE_ERR_INVALID_ARG;
  if (!path_samples_ok(n_samples)) return AFE_ERR_OUT_OF_RANGE;
  const double T = std::max(std::fabs(t_begin), std::fabs(t_end)), h = std::fabs(t_end - t_begin) / (double)(n_samples - 1);
  double sum2 = 0.0;
  for (int a = 0; a < 3; a++) {       // |p''| per axis: 20 c0 t^3 + 12 c1 t^2 + 6 c2 t + 2 c3, term by term
    const double m = ((std::fabs(coeffs18[a]) * 20.0 * T + std::fabs(coeffs18[3 + a]) * 12.0) * T + std::fabs(coeffs18[6 + a]) * 6.0) * T +
                     std::fabs(coeffs18[9 + a]) * 2.0;
    sum2 += m * m;
  }
  double scale = 1.0;
  if (rot9) {
    double f2 = 0.0;
    for (int k = 0; k < 9; k++) f2 += rot9[k] * rot9[k];
    scale = std::sqrt(f2);
  }
  *bound_m = (h * h / 8.0) * std::sqrt(sum2) * scale * (1.0 + 0x1p-40);
  return AFE_OK;
}

namespace {
// afe_clearance_plans_engine and its swept sibling (afe_path_sweep records)
int plans_engine(afe_engine *e, afe_clearance_map *m, int64_t first, int64_t count, const double mount[4], const afe_plan_output *plans,
                 int n_samples, double radius, double max_dist, bool swept, void *out, int64_t *n_colliding, float *kernel_ms) {
  if (!e || !m || first < 0 || count < 0 || !path_radii_ok(radius, max_dist)) return AFE_ERR_INVALID_ARG;
  if (count > 0 && (!plans || !out)) return AFE_ERR_INVALID_ARG;
  if (!path_samples_ok(n_samples)) return AFE_ERR_OUT_OF_RANGE;
  if (afe::engine_range_bad(e, first, count) || count > kMaxPaths) return AFE_ERR_OUT_OF_RANGE;
  if (count == 0) { if (n_colliding) *n_colliding = 0; return AFE_OK; }   // a valid range of nothing: answered before the engine is touched
  EngineAccess acc;
  int rc = afe::engine_enter(e, &acc);     // (ends a resident grid, as the camera does)
  if (rc != AFE_OK) return rc;
  if (acc.device != m->device) return AFE_ERR_INVALID_ARG;
  const afe_device_view &view = acc.view;
  const hipStream_t stream = acc.stream;
  const size_t n = (size_t)count, plan_bytes = n * sizeof(afe_plan_output), rec_bytes = n * (swept ? sizeof(afe_path_sweep) : sizeof(afe_path_clearance));
  std::lock_guard<std::mutex> turn(m->scratch_lock);
  if (m->scratch.capacity() < plan_bytes + rec_bytes + 8) {
    if (hipStreamSynchronize(stream) != hipSuccess) return AFE_ERR_HIP;
    if (!m->scratch.alloc(plan_bytes + rec_bytes + 8)) { (void)hipGetLastError(); return AFE_ERR_HIP; }
  }
  char *base = m->scratch.as<char>();        // records | plans | counter: every part 8-byte aligned
  PathArgs a;
  std::memset(&a, 0, sizeof(a));
  a.t = m->base;
  a.n_paths = count; a.n_samples = n_samples;
  a.radius2 = radius * radius; a.max_dist2 = max_dist * max_dist;
  a.out = (afe_path_clearance *)base;
  a.plans = (const afe_plan_output *)(base + rec_bytes);
  a.n_colliding = (unsigned long long *)(base + rec_bytes + plan_bytes);
  a.pos = view.pos; a.att = view.att; a.anchor_xy = view.pos_anchor_xy; a.stride = view.stride; a.first = first; a.elem_size = view.state_elem_size;
  static const double identity[4] = {1.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < 4; k++) a.mount[k] = (mount ? mount : identity)[k];
  // the plans are the only upload
  // (an error below leaves work in flight on the scratch and on `out`: wait for it before the next caller gets its turn)
  const auto fail = [&](int status) { (void)hipStreamSynchronize(stream); return status; };
  if (hipMemcpyAsync((void *)a.plans, plans, plan_bytes, hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemsetAsync(a.n_colliding, 0, 8, stream) != hipSuccess)
    return fail(AFE_ERR_HIP);
  float ms = 0;
  rc = launch_paths<true>(a, swept, stream, kernel_ms ? &ms : nullptr);
  if (rc != AFE_OK) return fail(rc);
  if (kernel_ms) *kernel_ms = ms;
  unsigned long long colliding = 0;
  if (hipMemcpyAsync(out, a.out, rec_bytes, hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipMemcpyAsync(&colliding, a.n_colliding, 8, hipMemcpyDeviceToHost, stream) != hipSuccess)
    return fail(AFE_ERR_HIP);
  if (hipStreamSynchronize(stream) != hipSuccess) return AFE_ERR_HIP;
  if (n_colliding) *n_colliding = (int64_t)colliding;
  return AFE_OK;
}
}  // namespace

extern "C" int afe_clearance_plans_engine(afe_engine *e, afe_clearance_map *m, int64_t first, int64_t count, const double mount[4],
                                          const afe_plan_output *plans, int n_samples, double radius, double max_dist, afe_path_clearance *out,
                                          int64_t *n_colliding, float *kernel_ms) {
  return plans_engine(e, m, first, count, mount, plans, n_samples, radius, max_dist, false, out, n_colliding, kernel_ms);
}

extern "C" int afe_clearance_plans_engine_swept(afe_engine *e, afe_clearance_map *m, int64_t first, int64_t count, const double mount[4],
                                                const afe_plan_output *plans, int n_samples, double radius, double max_dist, afe_path_sweep *out,
                                                int64_t *n_colliding, float *kernel_ms) {
  return plans_engine(e, m, first, count, mount, plans, n_samples, radius, max_dist, true, out, n_colliding, kernel_ms);
}

// ---------------------------------------------------------------------------------------
// the contact monitor
// ---------------------------------------------------------------------------------------
namespace {
int monitor_reset_range(afe_contact_monitor *c, int64_t first, int64_t count, hipStream_t stream) {
  for (int64_t done = 0; done < count; done += kPointsPerLaunch) {
    const int64_t n = std::min(count - done, kPointsPerLaunch);
    hipLaunchKernelGGL(afe_clearance_reset_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, c->min_dist2.as<double>(),
                       c->first_us.as<uint64_t>(), c->first_tri.as<int32_t>(), first + done, n);
    if (hipGetLastError() != hipSuccess) return AFE_ERR_HIP;
  }
  // the swept monitor forgets where these vehicles were: their next update is the zero-length segment
  if (c->prev_valid.get() && hipMemsetAsync(c->prev_valid.as<uint32_t>() + first, 0, (size_t)count * 4, stream) != hipSuccess) return AFE_ERR_HIP;
  return AFE_OK;
}
}  // namespace

namespace {
int monitor_create(afe_engine *e, afe_clearance_map *m, double contact_radius, double search_radius, bool swept, afe_contact_monitor **out) {
  if (!e || !m || !out) return AFE_ERR_INVALID_ARG;
  if (!(contact_radius > 0.0) || !(contact_radius <= search_radius) || !std::isfinite(search_radius)) return AFE_ERR_INVALID_ARG;
  EngineAccess acc;
  int rc = afe::engine_enter(e, &acc);
  if (rc != AFE_OK) return rc;
  if (acc.device != m->device) return AFE_ERR_INVALID_ARG;
  afe_contact_monitor *c = new afe_contact_monitor();
  c->engine = e; c->map = m; c->n = acc.view.n_vehicles; c->device = acc.device;
  c->contact2 = contact_radius * contact_radius;
  c->search2 = search_radius * search_radius;
  const size_t n = (size_t)c->n;
  if (!c->min_dist2.alloc(n * 8) || !c->first_us.alloc(n * 8) || !c->first_tri.alloc(n * 4) || !c->counts.alloc(16) ||
      !c->counts_host.alloc(16) || (swept && (!c->prev.alloc(n * 24) || !c->prev_valid.alloc(n * 4)))) {
    (void)hipGetLastError();
    (void)afe_contact_monitor_destroy(c);
    return AFE_ERR_HIP;
  }
  rc = monitor_reset_range(c, 0, c->n, acc.stream);
  if (rc == AFE_OK && hipStreamSynchronize(acc.stream) != hipSuccess) rc = AFE_ERR_HIP;
  if (rc != AFE_OK) { (void)afe_contact_monitor_destroy(c); return rc; }
  *out = c;
  return AFE_OK;
}
}  // namespace

extern "C" int afe_contact_monitor_create(afe_engine *e, afe_clearance_map *m, double contact_radius, double search_radius,
                                          afe_contact_monitor **out) {
  return monitor_create(e, m, contact_radius, search_radius, false, out);
}

extern "C" int afe_contact_monitor_create_swept(afe_engine *e, afe_clearance_map *m, double contact_radius, double search_radius,
                                                afe_contact_monitor **out) {
  return monitor_create(e, m, contact_radius, search_radius, true, out);
}

extern "C" int afe_contact_monitor_update(afe_contact_monitor *c, int64_t *n_in_contact, int64_t *n_ever_in_contact) {
  if (!c) return AFE_ERR_INVALID_ARG;
  EngineAccess acc;
  int rc = afe::engine_enter(c->engine, &acc);
  if (rc != AFE_OK) return rc;
  const afe_device_view &view = acc.view;
  const hipStream_t stream = acc.stream;
  if (view.n_vehicles != c->n) return AFE_ERR_INVALID_ARG;
  uint64_t now_us = 0;
  rc = afe_time_us(c->engine, &now_us);
  if (rc != AFE_OK) return rc;
  ClrArgs g = c->map->base;
  g.max_dist2 = c->search2;
  g.pos = view.pos; g.anchor_xy = view.pos_anchor_xy; g.stride = view.stride; g.first = 0; g.count = c->n; g.elem_size = view.state_elem_size;
  g.min_dist2 = c->min_dist2.as<double>(); g.first_us = c->first_us.as<uint64_t>(); g.first_tri = c->first_tri.as<int32_t>();
  g.counts = c->counts.as<unsigned long long>();
  g.contact2 = c->contact2; g.now_us = now_us;
  if (hipMemsetAsync(g.counts, 0, 16, stream) != hipSuccess) return AFE_ERR_HIP;
  if (c->prev.get()) {
    SegArgs a;
    std::memset(&a, 0, sizeof(a));
    a.g = g;
    a.prev = c->prev.as<double>(); a.prev_valid = c->prev_valid.as<uint32_t>(); a.prev_stride = c->n;
    rc = launch_swept<true, false>(a, stream, nullptr);
  } else {
    rc = launch_query<true, false>(g, stream, nullptr);
  }
  if (rc != AFE_OK) return rc;
  // the only bytes that cross the bus: one 16-byte copy
  const unsigned long long *counts_host = c->counts_host.as<unsigned long long>();
  if (hipMemcpyAsync(c->counts_host.get(), g.counts, 16, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
    return AFE_ERR_HIP;
  if (n_in_contact) *n_in_contact = (int64_t)counts_host[0];
  if (n_ever_in_contact) *n_ever_in_contact = (int64_t)counts_host[1];
  return AFE_OK;
}

extern "C" int afe_contact_monitor_get(afe_contact_monitor *c, int64_t first, int64_t count, double *min_dist2, uint64_t *first_contact_us,
                                       int32_t *first_contact_tri) {
  if (!c || first < 0 || count < 0) return AFE_ERR_INVALID_ARG;
  if (first > c->n || count > c->n - first) return AFE_ERR_OUT_OF_RANGE;
  if (count == 0) return AFE_OK;
  hipStream_t stream = nullptr;
  int device = 0;
  afe::engine_stream_device(c->engine, (void **)&stream, &device);
  if (hipSetDevice(device) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return AFE_ERR_HIP;
  const size_t n = (size_t)count;
  if ((min_dist2 && hipMemcpy(min_dist2, c->min_dist2.as<double>() + first, n * 8, hipMemcpyDeviceToHost) != hipSuccess) ||
      (first_contact_us && hipMemcpy(first_contact_us, c->first_us.as<uint64_t>() + first, n * 8, hipMemcpyDeviceToHost) != hipSuccess) ||
      (first_contact_tri && hipMemcpy(first_contact_tri, c->first_tri.as<int32_t>() + first, n * 4, hipMemcpyDeviceToHost) != hipSuccess))
    return AFE_ERR_HIP;
  return AFE_OK;
}

extern "C" int afe_contact_monitor_reset(afe_contact_monitor *c, int64_t first, int64_t count) {
  if (!c || first < 0 || count < 0) return AFE_ERR_INVALID_ARG;
  if (first > c->n || count > c->n - first) return AFE_ERR_OUT_OF_RANGE;
  if (count == 0) return AFE_OK;
  hipStream_t stream = nullptr;
  int device = 0;
  afe::engine_stream_device(c->engine, (void **)&stream, &device);
  if (hipSetDevice(device) != hipSuccess) return AFE_ERR_HIP;
  return monitor_reset_range(c, first, count, stream);
}

extern "C" int afe_contact_monitor_destroy(afe_contact_monitor *c) {
  if (!c) return AFE_ERR_INVALID_ARG;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  delete c;
  return AFE_OK;
}
