// afe_stats.hip -- ensemble statistics on the device: per-group reductions of the vehicles' state and per-vehicle
// latches, read from the engine's slabs.  The C ABI is in include/agrifly_engine.h ("ensemble statistics").
// Nothing here writes a slab, and no step kernel knows about it.
//
// THE DEFINITION (tests/stats_checker.py restates it in numpy float64, operation for operation; kernels and checker must
// give the same values, so the ORDER of the operations below is part of the contract).  Everything is IEEE double with
// contraction off; only + - * and comparisons appear, each correctly rounded on gfx950 and in numpy.  fp32 slabs are
// widened exactly.  Device and checker may differ in the sign of a zero and in nothing else.
//
//   per vehicle i, reference point (rx, ry, rz):
//     X = anchor_x + (double)px     Y = anchor_y + (double)py     Z = (double)pz            (as afe_get_state forms them)
//     dx = X - rx    dy = Y - ry    dz = Z - rz
//     h2 = dx*dx + dy*dy                               horizontal deviation squared
//     dz2 = dz*dz
//     v2 = (vx*vx + vy*vy) + vz*vz                     w2 = (wx*wx + wy*wy) + wz*wz       (w: body rates)
//     up = ((qw*qw - qx*qx) - qy*qy) + qz*qz           R[8] of the attitude's rotation matrix: the cosine of the tilt
//     valid    = every one of the 13 state values (position, velocity, attitude, rates) and dx, dy, dz is finite
//     grounded = valid and Z <= 0
//
//   GROUPS are contiguous index ranges: n_groups + 1 non-decreasing edges, 0 <= edges[0], edges[n_groups] <= n_vehicles;
//   group g is [edges[g], edges[g+1]).  Empty groups are allowed; vehicles outside every group are never read or written.
//
//   SUMS follow a fixed tree.  For a group with leaves a[0..n), indexed from the group's own first vehicle: at level
//   s = 1, 2, 4, ... while s < n, for every j that is a multiple of 2s with j + s < n:  a[j] = a[j] + a[j+s].  The sum is a[0]
//   (+0.0 for an empty group).  The "now" sums (sum_h2, sum_dz, sum_dz2, sum_v2, sum_w2) have the leaf +0.0 for a vehicle that
//   is not valid; the latch sums (sum_peak_h2, sum_acc_h2) take every vehicle's latch as it stands after this update.
//   The tree over n leaves is the tree over each aligned run of 256 leaves followed by the same tree over the run totals
//   (and so on, recursively), and a pair whose second member does not exist may as well add +0.0 (x + 0.0 == x but for the
//   sign of a zero): that is what the kernels do -- 64-lane xor butterfly (lane 0 holds the tree's value; addition is
//   commutative, so which lane of a pair is the left one does not matter), four wave totals as (w0 + w1) + (w2 + w3), one
//   partial per chunk of 256 vehicles, then the same over the partials in tiles of 256.
//
//   EXTREMES: a candidate replaces the held value only if it compares strictly greater (max) or smaller (min); start
//   from -inf (max) / +inf (min), which is also the answer for a group without candidates.  A NaN therefore never
//   replaces anything (only `up` can be one, for a finite attitude whose squares overflow).  The "now" extremes (max_h2,
//   min_dz, max_dz, max_v2, max_w2, min_up) run over the valid vehicles, max_peak_h2 and min_min_up over every vehicle's
//   latch after this update.  Arg-max: the lowest engine-local index among the vehicles holding the maximum, -1 with no
//   candidate.
//
//   LATCHES, per vehicle, updated by each update in which the vehicle is valid:
//     peak_h2 = h2 > peak_h2 ? h2 : peak_h2   (initially +0.0)      min_up = up < min_up ? up : min_up   (initially +inf)
//     acc_h2 = acc_h2 + h2   (initially +0.0; one addition per update, in update order)             n_valid += 1
//   first_grounded_us is set the first time `grounded` holds, first_invalid_us the first time the vehicle is not valid,
//   both to afe_time_us of that update; UINT64_MAX means never.
//
//   COUNTS: count = edges[g+1] - edges[g]; n_invalid, n_grounded now; n_ever_invalid, n_ever_grounded = vehicles whose
//   time latch is set after this update; sum_n_valid = the sum of the n_valid latches.
//
//   HISTOGRAM (optional): up to 63 ascending finite edges e_k > 0 in metres, e_k*e_k formed once on the host in double.
//   A valid vehicle falls into bin #{k : e_k*e_k <= h2}.  Integer counts do not depend on order: vector atomics in LDS,
//   then in global memory.
//
// THE STRUCTURE.  Two launches on the engine's stream, no hand-off between workgroups inside a launch, no floating-point
// atomics.  Chunk kernel: one 256-thread block per chunk of 256 consecutive vehicles of ONE group, chunks aligned to the
// group's first vehicle (table built on the host at creation); every lane loads its vehicle (planar, coalesced), updates
// the latches, and the block reduces 22 words to one partial record (planar [22][n_chunks]).  Group kernel: one block per
// group reduces that group's partials in tiles of 256, in place (tile t of a pass reads slots [256 t, 256 t + 256) and
// writes slot t <= 256 t), until one is left, and writes afe_group_stats.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "afe_consumer.h"

static_assert(sizeof(afe_group_stats) == 23 * 8, "afe_group_stats: 8-byte members only, the layout is ABI");

namespace {

constexpr int kBlock = 256;
constexpr int kMaxGroups = 65536;
constexpr int kMaxHistEdges = 63;
constexpr int kWords = 22;                               // 8-byte words of one partial record
constexpr int64_t kChunksPerLaunch = int64_t(1) << 22;   // a launch stays below 2^31 threads (HIP truncates silently)
constexpr int64_t kNoIndex = std::numeric_limits<int64_t>::max();
constexpr uint64_t kNever = ~uint64_t(0);

struct Chunk {          // 256 (the group's last one: 1..256) consecutive vehicles of one group
  int64_t first;
  int32_t group;
  int32_t len;
};
static_assert(sizeof(Chunk) == 16, "one dwordx4 per chunk");

// What a block reduces: the words of one partial record.  Named members only (an indexed array would live in scratch).
struct Rec {
  double sum_h2, sum_dz, sum_dz2, sum_v2, sum_w2, sum_peak, sum_acc;           // tree sums
  double max_h2, max_dz, max_v2, max_w2, max_peak;                             // replace only if greater
  double min_dz, min_up, min_min_up;                                           // replace only if smaller
  long long arg_h2, arg_peak;                                                  // lowest index holding the maximum; kNoIndex: none
  long long n_invalid, n_grounded, n_ever_invalid, n_ever_grounded, sum_n_valid;
};

__device__ __forceinline__ Rec rec_identity() {
  const double inf = std::numeric_limits<double>::infinity();
  Rec r;
  r.sum_h2 = r.sum_dz = r.sum_dz2 = r.sum_v2 = r.sum_w2 = r.sum_peak = r.sum_acc = 0.0;
  r.max_h2 = r.max_dz = r.max_v2 = r.max_w2 = r.max_peak = -inf;
  r.min_dz = r.min_up = r.min_min_up = inf;
  r.arg_h2 = r.arg_peak = kNoIndex;
  r.n_invalid = r.n_grounded = r.n_ever_invalid = r.n_ever_grounded = r.sum_n_valid = 0;
  return r;
}

__device__ __forceinline__ void take_max(double &v, double o) { v = o > v ? o : v; }
__device__ __forceinline__ void take_min(double &v, double o) { v = o < v ? o : v; }
__device__ __forceinline__ void take_argmax(double &v, long long &i, double ov, long long oi) {
  const bool take = ov > v || (ov == v && oi < i);
  v = take ? ov : v;
  i = take ? oi : i;
}

// a (+)= b, the definition's pairing: a is the left member
__device__ __forceinline__ void rec_combine(Rec &a, const Rec &b) {
#pragma clang fp contract(off)
  a.sum_h2 = a.sum_h2 + b.sum_h2; a.sum_dz = a.sum_dz + b.sum_dz; a.sum_dz2 = a.sum_dz2 + b.sum_dz2;
  a.sum_v2 = a.sum_v2 + b.sum_v2; a.sum_w2 = a.sum_w2 + b.sum_w2;
  a.sum_peak = a.sum_peak + b.sum_peak; a.sum_acc = a.sum_acc + b.sum_acc;
  take_argmax(a.max_h2, a.arg_h2, b.max_h2, b.arg_h2);
  take_argmax(a.max_peak, a.arg_peak, b.max_peak, b.arg_peak);
  take_max(a.max_dz, b.max_dz); take_max(a.max_v2, b.max_v2); take_max(a.max_w2, b.max_w2);
  take_min(a.min_dz, b.min_dz); take_min(a.min_up, b.min_up); take_min(a.min_min_up, b.min_min_up);
  a.n_invalid += b.n_invalid; a.n_grounded += b.n_grounded; a.n_ever_invalid += b.n_ever_invalid;
  a.n_ever_grounded += b.n_ever_grounded; a.sum_n_valid += b.sum_n_valid;
}

__device__ __forceinline__ Rec rec_shfl_xor(const Rec &r, int s) {
  Rec o;
  o.sum_h2 = __shfl_xor(r.sum_h2, s); o.sum_dz = __shfl_xor(r.sum_dz, s); o.sum_dz2 = __shfl_xor(r.sum_dz2, s);
  o.sum_v2 = __shfl_xor(r.sum_v2, s); o.sum_w2 = __shfl_xor(r.sum_w2, s);
  o.sum_peak = __shfl_xor(r.sum_peak, s); o.sum_acc = __shfl_xor(r.sum_acc, s);
  o.max_h2 = __shfl_xor(r.max_h2, s); o.max_dz = __shfl_xor(r.max_dz, s); o.max_v2 = __shfl_xor(r.max_v2, s);
  o.max_w2 = __shfl_xor(r.max_w2, s); o.max_peak = __shfl_xor(r.max_peak, s);
  o.min_dz = __shfl_xor(r.min_dz, s); o.min_up = __shfl_xor(r.min_up, s); o.min_min_up = __shfl_xor(r.min_min_up, s);
  o.arg_h2 = __shfl_xor(r.arg_h2, s); o.arg_peak = __shfl_xor(r.arg_peak, s);
  o.n_invalid = __shfl_xor(r.n_invalid, s); o.n_grounded = __shfl_xor(r.n_grounded, s);
  o.n_ever_invalid = __shfl_xor(r.n_ever_invalid, s); o.n_ever_grounded = __shfl_xor(r.n_ever_grounded, s);
  o.sum_n_valid = __shfl_xor(r.sum_n_valid, s);
  return o;
}

// The tree over the block's 256 leaves (thread t holds leaf t): the result is in thread 0.  Six butterfly levels inside
// each wave, then lanes 0..3 of wave 0 take the four wave totals through two more: lane 0 forms (w0 + w1) + (w2 + w3).
// `lds` holds 4 records; the closing barrier lets the caller use it again.
__device__ __forceinline__ void block_reduce(Rec &r, Rec *lds) {
#pragma clang fp contract(off)
#pragma unroll 1
  for (int s = 1; s < 64; s <<= 1) {
    const Rec o = rec_shfl_xor(r, s);
    rec_combine(r, o);
  }
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = r;
  __syncthreads();
  if (threadIdx.x < 64) {
    r = lds[threadIdx.x & 3];
#pragma unroll 1
    for (int s = 1; s < 4; s <<= 1) {
      const Rec o = rec_shfl_xor(r, s);
      rec_combine(r, o);
    }
  }
  __syncthreads();
}

struct StatsArgs {
  // the engine's slabs: planar, `stride` elements between components
  const void *pos, *vel, *att, *ang_vel;
  const double *anchor_xy;
  int64_t stride;
  // the monitor's arrays, indexed by the engine-local vehicle index; ref is planar [3][n]
  int64_t n;
  double *ref;
  double *peak_h2, *min_up, *acc_h2;
  long long *n_valid;
  unsigned long long *first_grounded_us, *first_invalid_us;
  // the layout
  const Chunk *chunks;
  const int64_t *edges;             // n_groups + 1
  const int64_t *group_chunk0;      // n_groups + 1: group g's chunks are [group_chunk0[g], group_chunk0[g+1])
  int64_t chunk_base;               // first chunk of this launch
  int64_t n_chunks;                 // all of them: the partials' plane stride
  unsigned long long *part;         // planar [kWords][n_chunks]
  // the histogram
  const double *hist_e2;
  int n_edges;                      // 0: off
  unsigned long long *hist;         // [n_groups][n_edges + 1]
  afe_group_stats *groups_out;
  unsigned long long now_us;
};

__device__ __forceinline__ unsigned long long d2u(double x) { return (unsigned long long)__double_as_longlong(x); }
__device__ __forceinline__ double u2d(unsigned long long x) { return __longlong_as_double((long long)x); }

__device__ __forceinline__ void part_store(const StatsArgs &g, int64_t c, const Rec &r) {
  unsigned long long *p = g.part + c;
  const int64_t S = g.n_chunks;
  p[0 * S] = d2u(r.sum_h2); p[1 * S] = d2u(r.sum_dz); p[2 * S] = d2u(r.sum_dz2); p[3 * S] = d2u(r.sum_v2); p[4 * S] = d2u(r.sum_w2);
  p[5 * S] = d2u(r.sum_peak); p[6 * S] = d2u(r.sum_acc);
  p[7 * S] = d2u(r.max_h2); p[8 * S] = d2u(r.max_dz); p[9 * S] = d2u(r.max_v2); p[10 * S] = d2u(r.max_w2); p[11 * S] = d2u(r.max_peak);
  p[12 * S] = d2u(r.min_dz); p[13 * S] = d2u(r.min_up); p[14 * S] = d2u(r.min_min_up);
  p[15 * S] = (unsigned long long)r.arg_h2; p[16 * S] = (unsigned long long)r.arg_peak;
  p[17 * S] = (unsigned long long)r.n_invalid; p[18 * S] = (unsigned long long)r.n_grounded;
  p[19 * S] = (unsigned long long)r.n_ever_invalid; p[20 * S] = (unsigned long long)r.n_ever_grounded;
  p[21 * S] = (unsigned long long)r.sum_n_valid;
}
__device__ __forceinline__ Rec part_load(const StatsArgs &g, int64_t c) {
  const unsigned long long *p = g.part + c;
  const int64_t S = g.n_chunks;
  Rec r;
  r.sum_h2 = u2d(p[0 * S]); r.sum_dz = u2d(p[1 * S]); r.sum_dz2 = u2d(p[2 * S]); r.sum_v2 = u2d(p[3 * S]); r.sum_w2 = u2d(p[4 * S]);
  r.sum_peak = u2d(p[5 * S]); r.sum_acc = u2d(p[6 * S]);
  r.max_h2 = u2d(p[7 * S]); r.max_dz = u2d(p[8 * S]); r.max_v2 = u2d(p[9 * S]); r.max_w2 = u2d(p[10 * S]); r.max_peak = u2d(p[11 * S]);
  r.min_dz = u2d(p[12 * S]); r.min_up = u2d(p[13 * S]); r.min_min_up = u2d(p[14 * S]);
  r.arg_h2 = (long long)p[15 * S]; r.arg_peak = (long long)p[16 * S];
  r.n_invalid = (long long)p[17 * S]; r.n_grounded = (long long)p[18 * S];
  r.n_ever_invalid = (long long)p[19 * S]; r.n_ever_grounded = (long long)p[20 * S];
  r.sum_n_valid = (long long)p[21 * S];
  return r;
}

template <typename T>
__global__ void __launch_bounds__(kBlock) afe_stats_chunk_kernel(StatsArgs g) {
#pragma clang fp contract(off)
  __shared__ Rec lds[4];
  __shared__ unsigned long long bins[kMaxHistEdges + 1];
  const int64_t c = g.chunk_base + blockIdx.x;
  const Chunk ch = g.chunks[c];
  const int lane = threadIdx.x;
  if (g.n_edges > 0 && lane <= g.n_edges) bins[lane] = 0;
  if (g.n_edges > 0) __syncthreads();
  Rec r = rec_identity();
  if (lane < ch.len) {
    const int64_t v = ch.first + lane, S = g.stride;
    const T *P = (const T *)g.pos, *V = (const T *)g.vel, *Q = (const T *)g.att, *W = (const T *)g.ang_vel;
    const double px = (double)P[v], py = (double)P[S + v], pz = (double)P[2 * S + v];
    const double vx = (double)V[v], vy = (double)V[S + v], vz = (double)V[2 * S + v];
    const double qw = (double)Q[v], qx = (double)Q[S + v], qy = (double)Q[2 * S + v], qz = (double)Q[3 * S + v];
    const double wx = (double)W[v], wy = (double)W[S + v], wz = (double)W[2 * S + v];
    const double X = g.anchor_xy[v] + px, Y = g.anchor_xy[S + v] + py, Z = pz;
    const double dx = X - g.ref[v], dy = Y - g.ref[g.n + v], dz = Z - g.ref[2 * g.n + v];
    double peak = g.peak_h2[v], mup = g.min_up[v], acc = g.acc_h2[v];
    long long nv = g.n_valid[v];
    unsigned long long t_gr = g.first_grounded_us[v], t_inv = g.first_invalid_us[v];
    const bool valid = __builtin_isfinite(px) && __builtin_isfinite(py) && __builtin_isfinite(pz) && __builtin_isfinite(vx) &&
                       __builtin_isfinite(vy) && __builtin_isfinite(vz) && __builtin_isfinite(qw) && __builtin_isfinite(qx) &&
                       __builtin_isfinite(qy) && __builtin_isfinite(qz) && __builtin_isfinite(wx) && __builtin_isfinite(wy) &&
                       __builtin_isfinite(wz) && __builtin_isfinite(dx) && __builtin_isfinite(dy) && __builtin_isfinite(dz);
    if (valid) {
      const double h2 = dx * dx + dy * dy;
      const double dz2 = dz * dz;
      const double v2 = (vx * vx + vy * vy) + vz * vz;
      const double w2 = (wx * wx + wy * wy) + wz * wz;
      const double up = ((qw * qw - qx * qx) - qy * qy) + qz * qz;
      const bool grounded = Z <= 0.0;
      peak = h2 > peak ? h2 : peak;
      mup = up < mup ? up : mup;
      acc = acc + h2;
      nv += 1;
      g.peak_h2[v] = peak; g.min_up[v] = mup; g.acc_h2[v] = acc; g.n_valid[v] = nv;
      if (grounded && t_gr == kNever) { t_gr = g.now_us; g.first_grounded_us[v] = t_gr; }
      r.sum_h2 = h2; r.sum_dz = dz; r.sum_dz2 = dz2; r.sum_v2 = v2; r.sum_w2 = w2;
      r.max_h2 = h2; r.arg_h2 = v;
      r.max_dz = dz; r.min_dz = dz; r.max_v2 = v2; r.max_w2 = w2;
      take_min(r.min_up, up);              // (a NaN stays out)
      r.n_grounded = grounded ? 1 : 0;
      if (g.n_edges > 0) {
        int bin = 0;
        for (int k = 0; k < g.n_edges; k++) bin += g.hist_e2[k] <= h2 ? 1 : 0;
        atomicAdd(&bins[bin], 1ull);
      }
    } else {
      r.n_invalid = 1;
      if (t_inv == kNever) { t_inv = g.now_us; g.first_invalid_us[v] = t_inv; }
    }
    r.sum_peak = peak; r.sum_acc = acc;
    r.max_peak = peak; r.arg_peak = v;
    take_min(r.min_min_up, mup);
    r.n_ever_grounded = t_gr != kNever ? 1 : 0;
    r.n_ever_invalid = t_inv != kNever ? 1 : 0;
    r.sum_n_valid = nv;
  }
  block_reduce(r, lds);          // (its barriers also order the LDS histogram)
  if (lane == 0) part_store(g, c, r);
  if (g.n_edges > 0 && lane <= g.n_edges) {
    const unsigned long long k = bins[lane];
    if (k) atomicAdd(g.hist + (int64_t)ch.group * (g.n_edges + 1) + lane, k);
  }
}

__global__ void __launch_bounds__(kBlock) afe_stats_group_kernel(StatsArgs g) {
#pragma clang fp contract(off)
  __shared__ Rec lds[4];
  const int grp = blockIdx.x;
  const int64_t c0 = g.group_chunk0[grp];
  int64_t cnt = g.group_chunk0[grp + 1] - c0;
  Rec r = rec_identity();
  while (cnt > 0) {
    const int64_t tiles = (cnt + kBlock - 1) / kBlock;
    for (int64_t t = 0; t < tiles; t++) {
      const int64_t k = t * kBlock + threadIdx.x;
      r = k < cnt ? part_load(g, c0 + k) : rec_identity();
      block_reduce(r, lds);
      if (tiles > 1 && threadIdx.x == 0) part_store(g, c0 + t, r);
    }
    if (tiles == 1) break;       // thread 0 holds the group's record
    __syncthreads();             // the tile totals are this block's own stores: visible to it after the barrier
    cnt = tiles;
  }
  if (threadIdx.x == 0) {
    afe_group_stats o;
    o.count = g.edges[grp + 1] - g.edges[grp];
    o.n_invalid = r.n_invalid; o.n_grounded = r.n_grounded;
    o.n_ever_invalid = r.n_ever_invalid; o.n_ever_grounded = r.n_ever_grounded;
    o.sum_n_valid = r.sum_n_valid;
    o.argmax_h2 = r.arg_h2 == kNoIndex ? -1 : r.arg_h2;
    o.argmax_peak_h2 = r.arg_peak == kNoIndex ? -1 : r.arg_peak;
    o.sum_h2 = r.sum_h2; o.sum_dz = r.sum_dz; o.sum_dz2 = r.sum_dz2; o.sum_v2 = r.sum_v2; o.sum_w2 = r.sum_w2;
    o.max_h2 = r.max_h2; o.min_dz = r.min_dz; o.max_dz = r.max_dz; o.max_v2 = r.max_v2; o.max_w2 = r.max_w2; o.min_up = r.min_up;
    o.sum_peak_h2 = r.sum_peak; o.sum_acc_h2 = r.sum_acc;
    o.max_peak_h2 = r.max_peak; o.min_min_up = r.min_min_up;
    g.groups_out[grp] = o;
  }
}

// latches back to initial (RESET) and / or the reference to where the vehicles are now (MARK), vehicles [first, first + count)
template <typename T>
__global__ void __launch_bounds__(kBlock) afe_stats_init_kernel(StatsArgs g, int64_t first, int64_t count, int reset, int mark) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  const int64_t v = first + i;
  if (reset) {
    g.peak_h2[v] = 0.0;
    g.min_up[v] = std::numeric_limits<double>::infinity();
    g.acc_h2[v] = 0.0;
    g.n_valid[v] = 0;
    g.first_grounded_us[v] = kNever;
    g.first_invalid_us[v] = kNever;
  }
  if (mark) {
    const T *P = (const T *)g.pos;
    const int64_t S = g.stride;
    g.ref[v] = g.anchor_xy[v] + (double)P[v];
    g.ref[g.n + v] = g.anchor_xy[S + v] + (double)P[S + v];
    g.ref[2 * g.n + v] = (double)P[2 * S + v];
  }
}

// ---------------------------------------------------------------------------------------
// host: the layout
// ---------------------------------------------------------------------------------------
struct Layout {
  int64_t n_chunks = 0;
  int levels = 0;
  std::vector<Chunk> chunks;            // filled only when asked for
  std::vector<int64_t> group_chunk0;
};

int build_layout(const int64_t *edges, int n_groups, int64_t n_vehicles, bool want_table, Layout &L) {
  if (!edges || n_groups < 1 || n_groups > kMaxGroups || n_vehicles < 0) return AFE_ERR_INVALID_ARG;
  if (edges[0] < 0) return AFE_ERR_INVALID_ARG;
  for (int g = 0; g < n_groups; g++) if (edges[g + 1] < edges[g]) return AFE_ERR_INVALID_ARG;
  if (edges[n_groups] > n_vehicles) return AFE_ERR_OUT_OF_RANGE;
  L.n_chunks = 0; L.levels = 0;
  if (want_table) L.group_chunk0.assign((size_t)n_groups + 1, 0);
  for (int g = 0; g < n_groups; g++) {
    const int64_t size = edges[g + 1] - edges[g];
    const int64_t nc = size / kBlock + (size % kBlock ? 1 : 0);
    int lv = 0;
    while (lv < 62 && (int64_t(1) << lv) < size) lv++;
    L.levels = std::max(L.levels, lv);
    if (want_table) {
      for (int64_t k = 0; k < nc; k++) {
        Chunk c;
        c.first = edges[g] + k * kBlock;
        c.group = g;
        c.len = (int32_t)std::min<int64_t>(kBlock, size - k * kBlock);
        L.chunks.push_back(c);
      }
      L.group_chunk0[(size_t)g + 1] = L.n_chunks + nc;
    }
    L.n_chunks += nc;
  }
  return AFE_OK;
}

}  // namespace

struct afe_stats_monitor {
  afe_engine *engine = nullptr;     // borrowed
  int device = 0;
  int64_t n = 0;
  int n_groups = 0, n_edges = 0;
  int64_t n_chunks = 0;
  uint64_t n_updates = 0;
  afe::DevBuf arena;                // one allocation: reference, latches, tables, partials
  StatsArgs args;                   // the monitor's part of the kernel arguments
  double *hist_e2 = nullptr;        // device, kMaxHistEdges doubles
  afe::DevBuf result;               // n_groups records, then the histogram
  afe::PinnedBuf<> result_host;     // the same
};

namespace {

size_t up256(size_t x) { return (x + 255) & ~size_t(255); }

// engine access for one call: stream, device and view (passes the engine's entry gate: a resident grid ends, a failed
// engine refuses by naming its first failure)
int enter(afe_stats_monitor *m, hipStream_t *stream, StatsArgs *g, int *elem) {
  afe::EngineAccess acc;
  const int rc = afe::engine_enter(m->engine, &acc);
  if (rc != AFE_OK) return rc;
  const afe_device_view &view = acc.view;
  if (view.n_vehicles != m->n || acc.device != m->device) return AFE_ERR_INVALID_ARG;
  *stream = acc.stream;
  *g = m->args;
  g->pos = view.pos; g->vel = view.vel; g->att = view.att; g->ang_vel = view.ang_vel;
  g->anchor_xy = view.pos_anchor_xy; g->stride = view.stride;
  *elem = view.state_elem_size;
  return AFE_OK;
}

int launch_init(const StatsArgs &g, int elem, int64_t first, int64_t count, int reset, int mark, hipStream_t stream) {
  const int64_t per = kChunksPerLaunch * kBlock;
  for (int64_t done = 0; done < count; done += per) {
    const int64_t n = std::min(count - done, per);
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
    if (elem == 8) hipLaunchKernelGGL(afe_stats_init_kernel<double>, grid, dim3(kBlock), 0, stream, g, first + done, n, reset, mark);
    else hipLaunchKernelGGL(afe_stats_init_kernel<float>, grid, dim3(kBlock), 0, stream, g, first + done, n, reset, mark);
    if (hipGetLastError() != hipSuccess) return AFE_ERR_HIP;
  }
  return AFE_OK;
}

int alloc_result(afe_stats_monitor *m, int n_edges) {
  const size_t bytes = (size_t)m->n_groups * sizeof(afe_group_stats) + (n_edges ? (size_t)m->n_groups * (n_edges + 1) * 8 : 0);
  if (!m->result.reserve(bytes, bytes) || !m->result_host.reserve(bytes, bytes)) {
    (void)hipGetLastError();
    return AFE_ERR_HIP;
  }
  return AFE_OK;
}

bool range_bad(int64_t first, int64_t count) { return first < 0 || count < 0; }

}  // namespace

extern "C" int afe_stats_check_layout(const int64_t *edges, int n_groups, int64_t n_vehicles, int64_t *n_chunks, int *levels) {
  Layout L;
  const int rc = build_layout(edges, n_groups, n_vehicles, false, L);
  if (rc != AFE_OK) return rc;
  if (n_chunks) *n_chunks = L.n_chunks;
  if (levels) *levels = L.levels;
  return AFE_OK;
}

extern "C" int afe_stats_create(afe_engine *e, const int64_t *edges, int n_groups, afe_stats_monitor **out) {
  if (!e || !edges || !out) return AFE_ERR_INVALID_ARG;
  int64_t first_global = 0, n = 0;
  afe::engine_shard(e, &first_global, &n);
  Layout L;
  int rc = build_layout(edges, n_groups, n, true, L);
  if (rc != AFE_OK) return rc;
  afe_stats_monitor *m = new afe_stats_monitor();
  m->engine = e; m->n = n; m->n_groups = n_groups; m->n_chunks = L.n_chunks;
  afe::EngineAccess acc;
  rc = afe::engine_enter(e, &acc);
  if (rc == AFE_OK && acc.view.n_vehicles != n) rc = AFE_ERR_INVALID_ARG;
  if (rc != AFE_OK) { delete m; return rc; }
  m->device = acc.device;
  const afe_device_view &view = acc.view;
  const hipStream_t stream = acc.stream;
  // one arena: [3][n] reference, six latch arrays, chunk table, edges, group_chunk0, partials
  const size_t N = (size_t)n, NC = (size_t)std::max<int64_t>(L.n_chunks, 1), NG = (size_t)n_groups + 1;
  size_t off = 0;
  const size_t o_ref = off; off += up256(N * 24);
  size_t o_latch[6];
  for (int k = 0; k < 6; k++) { o_latch[k] = off; off += up256(N * 8); }
  const size_t o_chunks = off; off += up256(NC * sizeof(Chunk));
  const size_t o_edges = off; off += up256(NG * 8);
  const size_t o_gc0 = off; off += up256(NG * 8);
  const size_t o_part = off; off += up256(NC * kWords * 8);
  const size_t o_e2 = off; off += up256(kMaxHistEdges * 8);
  bool ok = m->arena.alloc(off);
  unsigned char *A = m->arena.as<unsigned char>();
  std::memset(&m->args, 0, sizeof(m->args));
  StatsArgs &g = m->args;
  if (ok) {
    g.n = n;
    g.ref = (double *)(A + o_ref);
    g.peak_h2 = (double *)(A + o_latch[0]); g.min_up = (double *)(A + o_latch[1]); g.acc_h2 = (double *)(A + o_latch[2]);
    g.n_valid = (long long *)(A + o_latch[3]);
    g.first_grounded_us = (unsigned long long *)(A + o_latch[4]); g.first_invalid_us = (unsigned long long *)(A + o_latch[5]);
    g.chunks = (const Chunk *)(A + o_chunks); g.edges = (const int64_t *)(A + o_edges); g.group_chunk0 = (const int64_t *)(A + o_gc0);
    g.n_chunks = (int64_t)NC;
    g.part = (unsigned long long *)(A + o_part);
    m->hist_e2 = (double *)(A + o_e2);
    g.hist_e2 = m->hist_e2;
    ok = (L.chunks.empty() || hipMemcpy(A + o_chunks, L.chunks.data(), L.chunks.size() * sizeof(Chunk), hipMemcpyHostToDevice) == hipSuccess) &&
         hipMemcpy(A + o_edges, edges, NG * 8, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(A + o_gc0, L.group_chunk0.data(), NG * 8, hipMemcpyHostToDevice) == hipSuccess;
  }
  rc = ok ? alloc_result(m, 0) : AFE_ERR_HIP;
  if (rc == AFE_OK && n > 0) {
    StatsArgs run = g;
    run.pos = view.pos; run.anchor_xy = view.pos_anchor_xy; run.stride = view.stride;
    rc = launch_init(run, view.state_elem_size, 0, n, 1, 1, stream);
    if (rc == AFE_OK && hipStreamSynchronize(stream) != hipSuccess) rc = AFE_ERR_HIP;
  }
  if (rc != AFE_OK) { (void)hipGetLastError(); (void)afe_stats_destroy(m); return rc; }
  *out = m;
  return AFE_OK;
}

extern "C" int afe_stats_destroy(afe_stats_monitor *m) {
  if (!m) return AFE_ERR_INVALID_ARG;
  (void)hipSetDevice(m->device);
  (void)hipDeviceSynchronize();
  delete m;
  return AFE_OK;
}

extern "C" int afe_stats_info(const afe_stats_monitor *m, int *n_groups, int64_t *n_vehicles, int *n_hist_edges, uint64_t *n_updates) {
  if (!m) return AFE_ERR_INVALID_ARG;
  if (n_groups) *n_groups = m->n_groups;
  if (n_vehicles) *n_vehicles = m->n;
  if (n_hist_edges) *n_hist_edges = m->n_edges;
  if (n_updates) *n_updates = m->n_updates;
  return AFE_OK;
}

extern "C" int afe_stats_set_reference(afe_stats_monitor *m, int64_t first, int64_t count, const double *pos3) {
  if (!m || range_bad(first, count)) return AFE_ERR_INVALID_ARG;
  if (first > m->n || count > m->n - first) return AFE_ERR_OUT_OF_RANGE;   // (no sum: it can wrap)
  if (pos3) for (int64_t k = 0; k < 3 * count; k++) if (!std::isfinite(pos3[k])) return AFE_ERR_INVALID_ARG;
  if (count == 0) return AFE_OK;
  hipStream_t stream = nullptr;
  StatsArgs g;
  int elem = 0;
  const int erc = enter(m, &stream, &g, &elem);
  if (erc != AFE_OK) return erc;
  if (!pos3) return launch_init(g, elem, first, count, 0, 1, stream);
  if (hipStreamSynchronize(stream) != hipSuccess) return AFE_ERR_HIP;      // an update may still be reading the reference
  for (int k = 0; k < 3; k++)
    if (hipMemcpy(g.ref + (size_t)k * m->n + first, pos3 + (size_t)k * count, (size_t)count * 8, hipMemcpyHostToDevice) != hipSuccess) return AFE_ERR_HIP;
  return AFE_OK;
}

extern "C" int afe_stats_set_histogram(afe_stats_monitor *m, const double *edges_m, int n_edges) {
  if (!m || n_edges < 0 || n_edges > kMaxHistEdges || (n_edges > 0 && !edges_m)) return AFE_ERR_INVALID_ARG;
  double e2[kMaxHistEdges];
  for (int k = 0; k < n_edges; k++) {
    if (!std::isfinite(edges_m[k]) || !(edges_m[k] > 0.0) || (k > 0 && !(edges_m[k] > edges_m[k - 1]))) return AFE_ERR_INVALID_ARG;
    e2[k] = edges_m[k] * edges_m[k];
  }
  if (n_edges == 0) { m->n_edges = 0; return AFE_OK; }
  hipStream_t stream = nullptr;
  StatsArgs g;
  int elem = 0;
  const int erc = enter(m, &stream, &g, &elem);
  if (erc != AFE_OK) return erc;
  if (hipStreamSynchronize(stream) != hipSuccess) return AFE_ERR_HIP;      // an update may still be reading the old edges
  const int rc = alloc_result(m, n_edges);
  if (rc != AFE_OK) return rc;
  if (hipMemcpy(m->hist_e2, e2, (size_t)n_edges * 8, hipMemcpyHostToDevice) != hipSuccess) return AFE_ERR_HIP;
  m->n_edges = n_edges;
  return AFE_OK;
}

extern "C" int afe_stats_update(afe_stats_monitor *m, afe_group_stats *groups_out, int64_t *hist_out) {
  if (!m || !groups_out || (hist_out && m->n_edges == 0)) return AFE_ERR_INVALID_ARG;
  hipStream_t stream = nullptr;
  StatsArgs g;
  int elem = 0;
  const int erc = enter(m, &stream, &g, &elem);
  if (erc != AFE_OK) return erc;
  uint64_t now_us = 0;
  int rc = afe_time_us(m->engine, &now_us);
  if (rc != AFE_OK) return rc;
  const size_t rec_bytes = (size_t)m->n_groups * sizeof(afe_group_stats);
  const size_t hist_bytes = m->n_edges ? (size_t)m->n_groups * (m->n_edges + 1) * 8 : 0;
  g.now_us = now_us;
  g.n_edges = m->n_edges;
  g.groups_out = m->result.as<afe_group_stats>();
  g.hist = (unsigned long long *)(m->result.as<unsigned char>() + rec_bytes);
  if (hist_bytes && hipMemsetAsync(g.hist, 0, hist_bytes, stream) != hipSuccess) return AFE_ERR_HIP;
  for (int64_t done = 0; done < m->n_chunks; done += kChunksPerLaunch) {
    const int64_t nc = std::min(m->n_chunks - done, kChunksPerLaunch);
    g.chunk_base = done;
    if (elem == 8) hipLaunchKernelGGL(afe_stats_chunk_kernel<double>, dim3((unsigned)nc), dim3(kBlock), 0, stream, g);
    else hipLaunchKernelGGL(afe_stats_chunk_kernel<float>, dim3((unsigned)nc), dim3(kBlock), 0, stream, g);
    if (hipGetLastError() != hipSuccess) return AFE_ERR_HIP;
  }
  hipLaunchKernelGGL(afe_stats_group_kernel, dim3((unsigned)m->n_groups), dim3(kBlock), 0, stream, g);
  if (hipGetLastError() != hipSuccess) return AFE_ERR_HIP;
  // the only bytes that cross the bus: the group records and the histogram, one copy
  if (hipMemcpyAsync(m->result_host.get(), m->result.get(), rec_bytes + hist_bytes, hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess)
    return AFE_ERR_HIP;
  m->n_updates++;
  std::memcpy(groups_out, m->result_host.get(), rec_bytes);
  if (hist_out) std::memcpy(hist_out, m->result_host.as<unsigned char>() + rec_bytes, hist_bytes);
  return AFE_OK;
}

extern "C" int afe_stats_get(afe_stats_monitor *m, int64_t first, int64_t count, double *peak_h2, double *min_up, double *acc_h2, int64_t *n_valid,
                             uint64_t *first_grounded_us, uint64_t *first_invalid_us) {
  if (!m || range_bad(first, count)) return AFE_ERR_INVALID_ARG;
  if (first > m->n || count > m->n - first) return AFE_ERR_OUT_OF_RANGE;
  if (count == 0) return AFE_OK;
  hipStream_t stream = nullptr;
  int device = 0;
  afe::engine_stream_device(m->engine, (void **)&stream, &device);
  if (hipSetDevice(device) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return AFE_ERR_HIP;
  const StatsArgs &g = m->args;
  const size_t bytes = (size_t)count * 8;
  if ((peak_h2 && hipMemcpy(peak_h2, g.peak_h2 + first, bytes, hipMemcpyDeviceToHost) != hipSuccess) ||
      (min_up && hipMemcpy(min_up, g.min_up + first, bytes, hipMemcpyDeviceToHost) != hipSuccess) ||
      (acc_h2 && hipMemcpy(acc_h2, g.acc_h2 + first, bytes, hipMemcpyDeviceToHost) != hipSuccess) ||
      (n_valid && hipMemcpy(n_valid, g.n_valid + first, bytes, hipMemcpyDeviceToHost) != hipSuccess) ||
      (first_grounded_us && hipMemcpy(first_grounded_us, g.first_grounded_us + first, bytes, hipMemcpyDeviceToHost) != hipSuccess) ||
      (first_invalid_us && hipMemcpy(first_invalid_us, g.first_invalid_us + first, bytes, hipMemcpyDeviceToHost) != hipSuccess))
    return AFE_ERR_HIP;
  return AFE_OK;
}

extern "C" int afe_stats_reset(afe_stats_monitor *m, int64_t first, int64_t count) {
  if (!m || range_bad(first, count)) return AFE_ERR_INVALID_ARG;
  if (first > m->n || count > m->n - first) return AFE_ERR_OUT_OF_RANGE;
  if (count == 0) return AFE_OK;
  hipStream_t stream = nullptr;
  StatsArgs g;
  int elem = 0;
  const int erc = enter(m, &stream, &g, &elem);
  if (erc != AFE_OK) return erc;
  return launch_init(g, elem, first, count, 1, 0, stream);
}
