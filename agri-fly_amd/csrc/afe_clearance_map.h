// afe_clearance_map.h -- the clearance map's device records and its handle, shared by the two translation units that walk
// the map: afe_clearance.hip (distance queries, which also builds the map) and afe_raycast.hip (first-hit ray queries).
// Internal to the library.  The tree, its records and what each field means are described in afe_clearance.hip (THE STRUCTURE).
#pragma once
#include <stdint.h>

#include <mutex>

#include "afe_consumer.h"

namespace afe {
namespace clr {

constexpr int kBlock = 256;
constexpr int kStack = 32;
constexpr int kLeafMax = 4;
constexpr int kMaxBig = 16;
constexpr uint32_t kLeafBit = 0x80000000u, kNone = 0xffffffffu, kFirstMask = 0x0fffffffu;
constexpr int64_t kMaxTri = 0x0ffffff0;
constexpr int64_t kMaxPoints = int64_t(1) << 40;
constexpr int64_t kPointsPerLaunch = int64_t(1) << 30;   // a launch stays below 2^31 threads (HIP truncates silently)

// One triangle as the kernel wants it (112 B = seven dwordx4): box and identity first (one 32-byte fetch decides whether the
// double-precision part is needed), then a, ab, ac already in double.
struct CTri {
  float lo[3], hi[3];
  int32_t index;        // in the order given to afe_clearance_map_create
  int32_t degenerate;   // the definition's flag
  double a[3], ab[3], ac[3];
  int32_t pad[2];
};
static_assert(sizeof(CTri) == 112, "seven dwordx4 per triangle");

struct CChild {
  float lo[3];
  uint32_t ref;    // inner child: index of its CNode; leaf child: kLeafBit | count << 28 | first triangle (leaf order)
  float hi[3];
  uint32_t pad;
};
struct CNode { CChild c[2]; };
static_assert(sizeof(CNode) == 64, "two dwordx4 per child");

struct ClrArgs {
  const CNode *nodes;
  const CTri *tris;
  uint32_t root_ref;          // kNone: nothing in the tree
  uint32_t big_first, n_big;  // triangles kept out of the tree: slots [big_first, big_first + n_big)
  float root_lo[3], root_hi[3];
  double scene_lo[3], scene_hi[3];
  double max_dist2;
  // the points: planar, `stride` elements between components, element `first + i`
  const void *pos;
  const double *anchor_xy;    // engine state: x, y relative to this (afe_device_view::pos_anchor_xy); NULL: absolute
  int64_t stride, first, count;
  int elem_size;              // 4 or 8
  // query outputs (any may be NULL), indexed by i; closest planar [3][out_stride]
  double *dist2_out;
  int32_t *tri_out;
  double *closest_out;
  int64_t out_stride;
  // monitor latches, indexed by first + i
  double *min_dist2;
  uint64_t *first_us;
  int32_t *first_tri;
  unsigned long long *counts;   // [0] in contact now, [1] ever in contact
  double contact2;
  uint64_t now_us;
  unsigned long long *stats;    // counting build: [0] nodes visited, [1] triangle box tests, [2] fp64 evaluations
};

}  // namespace clr
}  // namespace afe

struct afe_clearance_map {
  int device = 0;
  int64_t n_tri = 0, n_nodes = 0;
  int depth = 0;
  double bounds[6] = {0, 0, 0, 0, 0, 0};
  afe::DevBuf nodes, tris;   // CNode, CTri
  afe::clr::ClrArgs base;    // the tree's part of the kernel arguments
  // afe_clearance_plans_engine's device scratch (plans, records, one counter), grown on demand; calls take turns on it
  std::mutex scratch_lock;
  afe::DevBuf scratch;
};
