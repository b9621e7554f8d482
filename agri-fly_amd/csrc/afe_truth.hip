// afe_truth.hip -- the depth-image ground truth of the RAPPIDS planner and its conservativeness tally on the device:
// DepthImagePlanner::IsCollisionFreeGroundTruth (DepthImagePlanner.cpp:1031-1098) and MeasureConservativeness
// (:972-1002), the test of Section IV.A of the RAPPIDS paper.  The C ABI is in include/agrifly_engine.h ("image truth").
//
// THE DEFINITION (tests/truth_checker.py restates it in numpy float64, operation for operation; kernel and checker must
// give the same bits, so the ORDER of the operations below is part of the contract).  Everything is IEEE double with
// contraction off; only + - * /, sqrt, one narrowing to float and comparisons appear, each correctly rounded on gfx950 and
// in numpy.  The frame is the camera frame (x right, y down, z into the image).
//
//   A path: coeffs c[6][3] (t^5 .. t^0 per axis, the layout of afe_plan_output::coeffs) and a range [t_begin, t_end).
//   The configuration is an afe_planner_config (width W, height H, focal_length f, cx, cy, depth_scale, the two radii,
//   min_checking_dist); timestep is an argument (the reference uses 0.1).
//
//   sample times:  t_0 = t_begin,  t_{k+1} = t_k + timestep  (the reference's running sum, NOT k * timestep);  a sample
//        exists while t_k < t_end;  their count is K (0 when t_begin >= t_end or either is a NaN).  K > 4096 is refused.
//   position:      per axis the power form of Trajectory.hpp:81-83, left to right:
//                      p = c0*t*t*t*t*t + c1*t*t*t*t + c2*t*t*t + c3*t*t + c4*t + c5            (not Horner)
//   scalars:       ignore = uint16(true_vehicle_radius / depth_scale),  edge = int(f * true_vehicle_radius / min_checking_dist),
//                  both truncating; formed once on the host.
//   skipped:       a sample with p.z < min_checking_dist is skipped in BOTH passes (a NaN compares false: not skipped).
//   field-of-view pass, over all samples first:   px = p.x*f/p.z + cx,  py = p.y*f/p.z + cy  (left to right);
//        the sample violates the view iff  px <= edge || px > W - edge || py <= edge || py > H - edge.
//        The lowest violating k, if any:  verdict 1, k_fov, t_fov;  no pixel is looked at.
//   pixel pass, only without verdict 1, samples in increasing k, for every pixel (x, y) with depth[y*W + x] > ignore:
//        ex = (x - cx)/f,  ey = (y - cy)/f
//        n  = (double)(float)sqrt(ex*ex + ey*ey + 1.0*1.0)              (Vec3::GetUnitVector narrows the norm to float)
//        u  = (ex/n, ey/n, 1.0/n)
//        d  = p.x*u.x + p.y*u.y + p.z*u.z
//        s  = d*d - (p.x*p.x + p.y*p.y + p.z*p.z) + r*r                  (r = planning_vehicle_radius; pow(., 2) is the product)
//        if s >= 0:   m = depth*depth_scale,  q = (m*ex, m*ey, m*1.0);
//                     the pixel occludes iff  sqrt(q.x*q.x + q.y*q.y + q.z*q.z) < d + sqrt(s)
//        The first sample with an occluding pixel:  verdict 2, k_hit, t_hit, pixel_hit = the lowest y*W + x among that
//        sample's occluding pixels.  Otherwise verdict 0.
//   the record (afe_image_truth):  n_samples = K;  n_checked = the samples whose pixels were examined, up to and including
//        k_hit (0 with verdict 1);  absent fields are -1 / NaN.  The empty record (a plan with found == 0): verdict -1, every
//        index -1, NaNs, both counts 0.
//
// THE STRUCTURE.  One wave per path, four paths per 256-thread block, no LDS, no barrier.  The field-of-view pass takes one
// sample per lane in batches of 64 (every lane follows the serial time sum and keeps the term of its own k), a ballot and
// the first set bit give the lowest violating k.  The pixel pass goes sample by sample, lanes over pixels, in row-major
// chunks of 64: the first chunk with a ballot hit ends the path, its first set bit is the lowest occluding pixel.
//
// NO OUTPUT BIT DEPENDS ON THE RECTANGLE.  Only a ray that meets the planning sphere (s >= 0) can occlude, so a sample
// scans the pixel rectangle that bounds the sphere's image instead of W x H pixels.  The bound: the line through the
// origin along (e, 1) in the xz plane passes within R of (p.x, p.z) iff e lies between
//        (p.x*p.z -+ R*sqrt(p.x^2 + p.z^2 - R^2)) / (p.z^2 - R^2)           (p.z > R),
// and a ray in space is never nearer to the centre than its projection is to the projected centre; likewise y.  With an
// exactly unit u, s >= 0 says "the ray passes within r".  What the computed s can add to that: (1) u is not unit -- n was
// narrowed to float, so |u| = 1 + eps, |eps| <= 2^-24 (+ 2^-52), d is scaled by it and d*d grows by at most 2^-22.9 |p|^2;
// (2) the dozen roundings of d, d*d, |p|^2 and the two sums, each <= 2^-53 of a term bounded by |p|^2 + r^2: < 2^-49
// (|p|^2 + r^2).  So s >= 0 implies  dist(ray, centre)^2 <= r^2 + 2^-22 |p|^2,  and the rectangle is formed with
//        R^2 = r^2 + 2^-20 |p|^2                                                (four times that),
// only where p.z^2 - R^2 > 2^-10 p.z^2 (the quotient's denominator then carries a relative error below 2^-42, the
// pixel coordinate one below 2^-40 of its magnitude, which is at most a few 10^4 where it matters), and is widened by TWO
// whole pixels outward on every side before it is clamped to the image.  Everything else -- p.z at or below that, a
// non-finite value anywhere -- scans the full image.  Inside the rectangle the definition's own test decides every pixel;
// tests/truth_checker.py visits all W x H pixels and is the judge.
//
// CANDIDATES (afe_image_truth_candidates).  Candidate c of planner i is formed exactly as afe_rappids_plan* forms it:
// deproject, c_generate and candidate_poly of afe_planner.h (the planner calls the same functions), range [0, Tf).  The
// verdicts go out as one byte each; the tally (afe_conservativeness) is formed by a second kernel, one wave per planner,
// ballots and popcounts over the flags afe_rappids_plan* filled and the verdicts, one set of integer vector atomics per
// planner.  Only candidates with the VelocityAdmissible bit (4) were collision-checked by the planner and count.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "afe_consumer.h"
#include "afe_planner.h"

namespace afe {
namespace {

constexpr int kBlock = 256;
constexpr int kPathsPerBlock = kBlock / 64;
constexpr int kMaxSamples = 4096;
constexpr int64_t kMaxPaths = int64_t(1) << 30;       // blocks stay far below 2^31
constexpr int64_t kMaxPixels = int64_t(1) << 24;      // a pixel index and a rectangle's area fit 32 bits with room

enum { MODE_PATHS = 0, MODE_PLANS = 1, MODE_CANDS = 2 };

struct TruthArgs {
  PlannerConfig cfg;
  int64_t n;                      // paths (candidates: n_planners * n_candidates)
  const uint16_t *images;         // [n_images][H][W]
  const int32_t *image_index;     // per path (candidates: per planner) or NULL: its own number
  double timestep;
  int ignore, edge;               // the definition's two scalars
  // explicit paths
  const double *coeffs;           // [n][6][3]
  const double *t_range;          // planar [2][n]
  // plans
  const afe_plan_output *plans;   // [n]
  // candidates
  int64_t n_planners;
  const double *vel0, *acc0;      // planar [3][n_planners]
  const double *samples;          // [n_tables][n_candidates][4]
  const int32_t *sample_table;    // [n_planners] or NULL
  int n_candidates;
  uint8_t *verdict_out;           // [n]
  double *coeffs_out;             // [n][6][3] or NULL
  // outputs
  afe_image_truth *out;           // [n] or NULL
  unsigned long long *n_free;     // one word or NULL
  unsigned long long *stats;      // counting build: [0] samples examined, [1] pixels tested for s, [2] pixels with s >= 0
};

// the definition's position: the power form, left to right
__device__ __forceinline__ double truth_axis(const double (&c)[18], int a, double t) {
#pragma clang fp contract(off)
  return c[a] * t * t * t * t * t + c[3 + a] * t * t * t * t + c[6 + a] * t * t * t + c[9 + a] * t * t + c[12 + a] * t + c[15 + a];
}

// one axis of the rectangle (file header): pixel coordinates [lo, hi] that hold every pixel whose ray can give s >= 0;
// false: no bound (scan everything).  q = the centre's coordinate on this axis, den = p.z^2 - R^2 > 0, R2 = R^2.
__device__ __forceinline__ bool truth_span(double q, double pz, double den, double R2, double f, double centre, int size, int &lo, int &hi) {
#pragma clang fp contract(off)
  const double root = sqrt(R2) * sqrt(q * q + den);          // R * sqrt(q^2 + p.z^2 - R^2)
  const double e0 = (q * pz - root) / den, e1 = (q * pz + root) / den;
  const double a = e0 * f + centre, b = e1 * f + centre;
  const double xa = floor(fmin(a, b)) - 2.0, xb = ceil(fmax(a, b)) + 2.0;
  if (!(__builtin_isfinite(xa) && __builtin_isfinite(xb))) return false;
  lo = (int)fmin(fmax(xa, 0.0), (double)size);              // clamped in double: the conversions cannot overflow
  hi = (int)fmax(fmin(xb, (double)(size - 1)), -1.0);
  return true;
}

__device__ __forceinline__ unsigned long long truth_wave_sum(unsigned long long x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}

template <int MODE, bool COUNT>
__global__ void __launch_bounds__(kBlock) afe_image_truth_kernel(const TruthArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t path = (int64_t)blockIdx.x * kPathsPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (path >= a.n) return;                // a wave without a path falls through (no barrier below)
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const int W = a.cfg.width, H = a.cfg.height;

  double c[18], tb = 0.0, te = 0.0;
  int64_t owner = path;                   // whose image
  bool judged = true;
  if (MODE == MODE_PATHS) {
    const double *src = a.coeffs + 18 * path;
#pragma unroll
    for (int j = 0; j < 18; j++) c[j] = src[j];
    tb = a.t_range[path]; te = a.t_range[a.n + path];
  } else if (MODE == MODE_PLANS) {
    const afe_plan_output *plan = a.plans + path;
    const double *src = &plan->coeffs[0][0];
#pragma unroll
    for (int j = 0; j < 18; j++) c[j] = src[j];
    te = plan->tf;
    judged = plan->found != 0;
  } else {
    owner = path / a.n_candidates;
    const int cand = (int)(path - owner * a.n_candidates);
    const double *sample = a.samples + ((int64_t)(a.sample_table ? a.sample_table[owner] : 0) * a.n_candidates + cand) * 4;
    Cand k;
    double pf[3];
    for (int ax = 0; ax < 3; ax++) {
      k.v0[ax] = a.vel0[ax * a.n_planners + owner];
      k.a0[ax] = a.acc0[ax * a.n_planners + owner];
      k.grav[ax] = 0.0;                   // (no part of the coefficients)
    }
    deproject(a.cfg, sample[0], sample[1], sample[2], pf);
    c_generate(k, pf, sample[3]);
    Poly p;
    candidate_poly(k, p);
#pragma unroll
    for (int j = 0; j < 18; j++) c[j] = p.c[j / 3][j % 3];
    te = k.tf;
    if (a.coeffs_out && lane == 0) {
      double *dst = a.coeffs_out + 18 * path;
#pragma unroll
      for (int j = 0; j < 18; j++) dst[j] = c[j];
    }
  }
  const uint16_t *img = a.images + (int64_t)(a.image_index ? a.image_index[owner] : owner) * W * H;
  const double f = a.cfg.focal_length, cx = a.cfg.cx, cy = a.cfg.cy, min_dist = a.cfg.min_checking_dist;

  // ---- field of view: one sample per lane, batches of 64 ----
  int K = 0, k_fov = -1;
  double t_fov = nan;
  {
    const double edge = (double)a.edge, right = (double)(W - a.edge), bottom = (double)(H - a.edge);
    double t_run = tb;                    // the time of sample `base`
    for (int base = 0; judged && base < kMaxSamples && t_run < te; base += 64) {
      double my_t = t_run, t = t_run;
      bool mine = false;
      for (int j = 0; j < 64; j++) {      // the serial sum; lane j keeps its own term
        if (lane == j) { my_t = t; mine = t < te; }
        t = t + a.timestep;
      }
      t_run = t;
      const double px = truth_axis(c, 0, my_t), py = truth_axis(c, 1, my_t), pz = truth_axis(c, 2, my_t);
      bool violates = false;
      if (mine && !(pz < min_dist)) {
        const double ix = px * f / pz + cx, iy = py * f / pz + cy;
        violates = ix <= edge || ix > right || iy <= edge || iy > bottom;
      }
      K += __popcll(__ballot(mine));
      const unsigned long long bad = __ballot(violates);
      const int first = bad ? __ffsll((long long)bad) - 1 : 0;
      const double t_at = __shfl(my_t, first);
      if (bad && k_fov < 0) { k_fov = base + first; t_fov = t_at; }
    }
  }

  // ---- pixels: sample by sample, lanes over the pixels of the sphere's rectangle ----
  int k_hit = -1, pixel_hit = -1, n_checked = 0;
  double t_hit = nan;
  unsigned long long n_tested = 0, n_meet = 0;
  if (judged && k_fov < 0) {
    const double r2 = a.cfg.planning_vehicle_radius * a.cfg.planning_vehicle_radius, scale = a.cfg.depth_scale;
    const int ignore = a.ignore;
    double t = tb;
    for (int k = 0; k < K && k_hit < 0; k++, t = t + a.timestep) {       // K <= 4096
      const double px = truth_axis(c, 0, t), py = truth_axis(c, 1, t), pz = truth_axis(c, 2, t);
      if (pz < min_dist) continue;
      n_checked++;
      int x0 = 0, x1 = W - 1, y0 = 0, y1 = H - 1;
      {
        const double pp = px * px + py * py + pz * pz;
        const double R2 = r2 + 0x1p-20 * pp;
        const double den = pz * pz - R2;
        int xa, xb, ya, yb;
        if (pz > 0.0 && den > 0x1p-10 * (pz * pz) && __builtin_isfinite(pp) && truth_span(px, pz, den, R2, f, cx, W, xa, xb) &&
            truth_span(py, pz, den, R2, f, cy, H, ya, yb)) {
          x0 = xa; x1 = xb; y0 = ya; y1 = yb;
        }
      }
      const int rw = x1 - x0 + 1, rh = y1 - y0 + 1;
      const unsigned total = rw > 0 && rh > 0 ? (unsigned)rw * (unsigned)rh : 0u;      // <= W*H < 2^24
      const double pn2 = px * px + py * py + pz * pz;
      for (unsigned idx0 = 0; idx0 < total; idx0 += 64) {
        const unsigned idx = idx0 + (unsigned)lane;
        bool occludes = false;
        int pixel = 0;
        if (idx < total) {
          const unsigned row = idx / (unsigned)rw;
          const int x = x0 + (int)(idx - row * (unsigned)rw), y = y0 + (int)row;
          pixel = y * W + x;
          const int depth = img[pixel];
          if (depth > ignore) {
            const double ex = ((double)x - cx) / f, ey = ((double)y - cy) / f;
            const double n = (double)(float)sqrt(ex * ex + ey * ey + 1.0 * 1.0);
            const double ux = ex / n, uy = ey / n, uz = 1.0 / n;
            const double d = px * ux + py * uy + pz * uz;
            const double s = d * d - pn2 + r2;
            if (COUNT) n_tested++;
            if (s >= 0.0) {
              if (COUNT) n_meet++;
              const double m = (double)depth * scale;
              const double qx = m * ex, qy = m * ey, qz = m * 1.0;
              occludes = sqrt(qx * qx + qy * qy + qz * qz) < d + sqrt(s);
            }
          }
        }
        const unsigned long long hits = __ballot(occludes);
        if (hits) {
          k_hit = k; t_hit = t;
          pixel_hit = __shfl(pixel, __ffsll((long long)hits) - 1);
          break;
        }
      }
    }
  }

  const int verdict = !judged ? -1 : (k_fov >= 0 ? 1 : (k_hit >= 0 ? 2 : 0));
  if (lane == 0) {
    if (a.out) {
      afe_image_truth *r = a.out + path;
      r->verdict = verdict;
      r->k_fov = k_fov; r->t_fov = t_fov;
      r->k_hit = k_hit; r->t_hit = t_hit;
      r->pixel_hit = pixel_hit;
      r->n_samples = K; r->n_checked = n_checked;
    }
    if (MODE == MODE_CANDS) a.verdict_out[path] = (uint8_t)verdict;
    if (a.n_free && verdict == 0) atomicAdd(a.n_free, 1ull);      // one integer vector atomic per free path
  }
  if (COUNT) {
    const unsigned long long s1 = truth_wave_sum(n_tested), s2 = truth_wave_sum(n_meet);
    if (lane < 3) atomicAdd(a.stats + lane, lane == 0 ? (unsigned long long)n_checked : (lane == 1 ? s1 : s2));
  }
}

// MeasureConservativeness' counts: one wave per planner over its candidates; tally[6] summed over the planners
__global__ void __launch_bounds__(64) afe_truth_tally_kernel(const uint8_t *__restrict__ flags, const uint8_t *__restrict__ verdict, int64_t n,
                                                             int n_candidates, unsigned long long *tally, int64_t *per_planner) {
  const int64_t i = blockIdx.x;
  if (i >= n) return;
  const int lane = threadIdx.x;
  int sums[6] = {0, 0, 0, 0, 0, 0};
  for (int base = 0; base < n_candidates; base += 64) {
    const int cnd = base + lane;
    const bool has = cnd < n_candidates;
    const unsigned fl = has ? flags[i * n_candidates + cnd] : 0u;
    const unsigned v = has ? verdict[i * n_candidates + cnd] : 0u;
    const bool checked = (fl & 4u) != 0, pfree = checked && (fl & 8u) != 0, collides = checked && !(fl & 8u);
    sums[0] += __popcll(__ballot(checked));
    sums[1] += __popcll(__ballot(pfree));
    sums[2] += __popcll(__ballot(collides && v != 0));
    sums[3] += __popcll(__ballot(collides && v == 0));
    sums[4] += __popcll(__ballot(pfree && v == 1));
    sums[5] += __popcll(__ballot(pfree && v == 2));
  }
  int mine = 0;
#pragma unroll
  for (int q = 0; q < 6; q++) if (lane == q) mine = sums[q];
  if (lane < 6) {
    if (per_planner) per_planner[i * 6 + lane] = mine;
    if (mine) atomicAdd(tally + lane, (unsigned long long)mine);
  }
}

// the definition's sample count (and times) for one range; false: more than 4096
bool sample_times(double tb, double te, double timestep, int *K, double *t_out) {
#pragma clang fp contract(off)
  int k = 0;
  for (double t = tb; t < te; t = t + timestep) {
    if (k == kMaxSamples) return false;
    if (t_out) t_out[k] = t;
    k++;
  }
  *K = k;
  return true;
}

// what is AFE_ERR_INVALID_ARG about the configuration and the step
bool truth_config_bad(const afe_planner_config *cfg, double timestep) {
  return !cfg || cfg->width <= 0 || cfg->height <= 0 || !(timestep > 0.0) || !std::isfinite(timestep);
}

// what is AFE_ERR_OUT_OF_RANGE about the configuration, and the definition's two scalars
int truth_scalars(const afe_planner_config *cfg, int *ignore, int *edge) {
#pragma clang fp contract(off)
  if ((int64_t)cfg->width * cfg->height > kMaxPixels) return AFE_ERR_OUT_OF_RANGE;      // an image the call cannot take
  if (!(cfg->min_checking_dist > 0.0)) return AFE_ERR_OUT_OF_RANGE;
  const double qi = cfg->true_vehicle_radius / cfg->depth_scale;
  if (!(qi > -1.0 && qi < 65536.0)) return AFE_ERR_OUT_OF_RANGE;                         // uint16(qi) is not defined
  const double qe = cfg->focal_length * cfg->true_vehicle_radius / cfg->min_checking_dist;
  if (!(qe > -1073741824.0 && qe < 1073741824.0)) return AFE_ERR_OUT_OF_RANGE;           // nor int(qe); W - edge stays an int
  *ignore = (int)(uint16_t)qi;
  *edge = (int)qe;
  return AFE_OK;
}

struct ImageSource {
  const void *images;
  int64_t n_images;
  int on_device;
  const int32_t *image_index;
};

// image arguments against `n_owners` owners (paths or planners): what is AFE_ERR_INVALID_ARG, what is AFE_ERR_OUT_OF_RANGE
bool images_bad(const ImageSource &s, int64_t n_owners) {
  return !s.images || s.n_images <= 0 || (s.on_device && ((uintptr_t)s.images & 15u)) || (!s.image_index && s.n_images < n_owners);
}
bool image_index_bad(const ImageSource &s, int64_t n_owners) {
  if (s.image_index)
    for (int64_t i = 0; i < n_owners; i++) if (s.image_index[i] < 0 || s.image_index[i] >= s.n_images) return true;
  return false;
}

bool images_upload(const afe_planner_config *cfg, const ImageSource &s, int64_t n_owners, DevBuf &d_img, DevBuf &d_idx, TruthArgs &g) {
  if (s.on_device) {
    g.images = (const uint16_t *)s.images;
  } else {
    if (!d_img.upload(s.images, (size_t)s.n_images * cfg->width * cfg->height * 2)) return false;
    g.images = (const uint16_t *)d_img.get();
  }
  g.image_index = nullptr;
  if (s.image_index) {
    if (!d_idx.upload(s.image_index, (size_t)n_owners * 4)) return false;
    g.image_index = (const int32_t *)d_idx.get();
  }
  return true;
}

template <int MODE>
int truth_launch(const TruthArgs &g, bool count, hipStream_t stream) {
  const dim3 grid((unsigned)((g.n + kPathsPerBlock - 1) / kPathsPerBlock)), block(kBlock);
  if (count) hipLaunchKernelGGL((afe_image_truth_kernel<MODE, true>), grid, block, 0, stream, g);
  else hipLaunchKernelGGL((afe_image_truth_kernel<MODE, false>), grid, block, 0, stream, g);
  return hipGetLastError() == hipSuccess ? AFE_OK : AFE_ERR_HIP;
}

// explicit paths and plans: records and the free count, or (stats != NULL) the counters of the counting build
int truth_records(int device, const afe_planner_config *cfg, int64_t n, const ImageSource &src, const double *coeffs, const double *t_range,
                  const afe_plan_output *plans, double timestep, afe_image_truth *out, int64_t *n_free, uint64_t *stats, float *kernel_ms) {
  if (truth_config_bad(cfg, timestep) || n < 0 || n > kMaxPaths || (plans ? false : (!coeffs || !t_range)) || (!out && !stats) || images_bad(src, n))
    return AFE_ERR_INVALID_ARG;
  int ignore = 0, edge = 0;
  int rc = truth_scalars(cfg, &ignore, &edge);
  if (rc != AFE_OK) return rc;
  if (image_index_bad(src, n)) return AFE_ERR_OUT_OF_RANGE;
  for (int64_t i = 0; i < n; i++) {
    int K = 0;
    if (plans && !plans[i].found) continue;
    if (!sample_times(plans ? 0.0 : t_range[i], plans ? plans[i].tf : t_range[n + i], timestep, &K, nullptr)) return AFE_ERR_OUT_OF_RANGE;
  }
  if (n == 0) {
    if (n_free) *n_free = 0;
    if (stats) for (int k = 0; k < 4; k++) stats[k] = 0;
    return AFE_OK;
  }
  rc = pick_gfx950(device, &device);
  if (rc != AFE_OK) return rc;

  TruthArgs g;
  std::memset(&g, 0, sizeof(g));
  g.cfg = *cfg; g.n = n; g.timestep = timestep; g.ignore = ignore; g.edge = edge;
  DevBuf d_img, d_idx, d_co, d_tr, d_plans, d_out, d_words;
  if (!images_upload(cfg, src, n, d_img, d_idx, g)) { (void)hipGetLastError(); return AFE_ERR_HIP; }
  bool ok = plans ? d_plans.upload(plans, (size_t)n * sizeof(afe_plan_output)) : (d_co.upload(coeffs, (size_t)n * 144) && d_tr.upload(t_range, (size_t)n * 16));
  ok = ok && (!out || d_out.alloc((size_t)n * sizeof(afe_image_truth))) && d_words.alloc(32) && hipMemset(d_words.get(), 0, 32) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); return AFE_ERR_HIP; }
  g.coeffs = (const double *)d_co.get(); g.t_range = (const double *)d_tr.get(); g.plans = (const afe_plan_output *)d_plans.get();
  g.out = (afe_image_truth *)d_out.get();
  g.n_free = (unsigned long long *)d_words.get();
  g.stats = stats ? (unsigned long long *)d_words.get() + 1 : nullptr;

  float ms = 0;
  StreamTimer timer(nullptr, true);
  if (!timer.ok()) return AFE_ERR_HIP;
  rc = timer.finish(plans ? truth_launch<MODE_PLANS>(g, stats != nullptr, nullptr) : truth_launch<MODE_PATHS>(g, stats != nullptr, nullptr), &ms);
  if (rc != AFE_OK) return rc;
  unsigned long long words[4];
  if (!d_words.download(words, 32) || (out && !d_out.download(out, (size_t)n * sizeof(afe_image_truth)))) return AFE_ERR_HIP;
  if (n_free) *n_free = (int64_t)words[0];
  if (stats) {
    for (int k = 0; k < 3; k++) stats[k] = words[1 + k];
    stats[3] = (uint64_t)cfg->width * (uint64_t)cfg->height * (uint64_t)words[1];
  }
  if (kernel_ms) *kernel_ms = ms;
  return AFE_OK;
}

}  // namespace
}  // namespace afe

using namespace afe;

// the counterpart of afe_device_download: how a host without its own HIP allocator puts depth images into an afe_device_alloc buffer
extern "C" int afe_device_upload(void *dev_dst, const void *host_src, uint64_t bytes) {
  if (!dev_dst || !host_src) return AFE_ERR_INVALID_ARG;
  return hipMemcpy(dev_dst, host_src, bytes, hipMemcpyHostToDevice) == hipSuccess ? AFE_OK : AFE_ERR_HIP;
}

extern "C" int afe_image_truth_sample_times(double t_begin, double t_end, double timestep, int *n_samples, double *t_out) {
  if (!n_samples || !(timestep > 0.0) || !std::isfinite(timestep)) return AFE_ERR_INVALID_ARG;
  int K = 0;
  if (!sample_times(t_begin, t_end, timestep, &K, nullptr)) return AFE_ERR_OUT_OF_RANGE;
  if (t_out) (void)sample_times(t_begin, t_end, timestep, &K, t_out);
  *n_samples = K;
  return AFE_OK;
}

extern "C" int afe_image_truth_paths(int device, const afe_planner_config *cfg, int64_t n_paths, const void *images, int64_t n_images,
                                     int images_on_device, const int32_t *image_index, const double *coeffs, const double *t_range,
                                     double timestep, afe_image_truth *out, int64_t *n_free, float *kernel_ms) {
  if (!out) return AFE_ERR_INVALID_ARG;
  const ImageSource src = {images, n_images, images_on_device, image_index};
  return truth_records(device, cfg, n_paths, src, coeffs, t_range, nullptr, timestep, out, n_free, nullptr, kernel_ms);
}

extern "C" int afe_image_truth_paths_stats(int device, const afe_planner_config *cfg, int64_t n_paths, const void *images, int64_t n_images,
                                           int images_on_device, const int32_t *image_index, const double *coeffs, const double *t_range,
                                           double timestep, uint64_t stats[4], float *kernel_ms) {
  if (!stats) return AFE_ERR_INVALID_ARG;
  const ImageSource src = {images, n_images, images_on_device, image_index};
  return truth_records(device, cfg, n_paths, src, coeffs, t_range, nullptr, timestep, nullptr, nullptr, stats, kernel_ms);
}

extern "C" int afe_image_truth_plans(int device, const afe_planner_config *cfg, int64_t n, const void *images, int64_t n_images,
                                     int images_on_device, const int32_t *image_index, const afe_plan_output *plans, double timestep,
                                     afe_image_truth *out, int64_t *n_free, float *kernel_ms) {
  if (!out || !plans) return AFE_ERR_INVALID_ARG;
  const ImageSource src = {images, n_images, images_on_device, image_index};
  return truth_records(device, cfg, n, src, nullptr, nullptr, plans, timestep, out, n_free, nullptr, kernel_ms);
}

extern "C" int afe_image_truth_candidates(int device, const afe_planner_config *cfg, int64_t n, const void *images, int64_t n_images,
                                          int images_on_device, const int32_t *image_index, const double *vel0, const double *acc0,
                                          const double *samples, int n_tables, const int32_t *sample_table, int n_candidates,
                                          const uint8_t *flags, double timestep, uint8_t *verdict_out, double *coeffs_out,
                                          afe_conservativeness *tally, afe_conservativeness *per_planner, float *kernel_ms) {
  const ImageSource src = {images, n_images, images_on_device, image_index};
  if (truth_config_bad(cfg, timestep) || n < 0 || !vel0 || !acc0 || !samples || n_tables <= 0 || n_candidates <= 0 || !flags || !verdict_out || !tally ||
      n > kMaxPaths / n_candidates || images_bad(src, n))
    return AFE_ERR_INVALID_ARG;
  int ignore = 0, edge = 0;
  int rc = truth_scalars(cfg, &ignore, &edge);
  if (rc != AFE_OK) return rc;
  if (image_index_bad(src, n)) return AFE_ERR_OUT_OF_RANGE;
  if (sample_table)
    for (int64_t i = 0; i < n; i++) if (sample_table[i] < 0 || sample_table[i] >= n_tables) return AFE_ERR_OUT_OF_RANGE;
  for (int64_t k = 0; k < (int64_t)n_tables * n_candidates; k++) {
    int K = 0;
    if (!sample_times(0.0, samples[4 * k + 3], timestep, &K, nullptr)) return AFE_ERR_OUT_OF_RANGE;
  }
  if (n == 0) {
    std::memset(tally, 0, sizeof(*tally));
    return AFE_OK;
  }
  rc = pick_gfx950(device, &device);
  if (rc != AFE_OK) return rc;

  const size_t total = (size_t)n * n_candidates;
  TruthArgs g;
  std::memset(&g, 0, sizeof(g));
  g.cfg = *cfg; g.n = (int64_t)total; g.timestep = timestep; g.ignore = ignore; g.edge = edge;
  g.n_planners = n; g.n_candidates = n_candidates;
  DevBuf d_img, d_idx, d_v, d_a, d_s, d_t, d_flags, d_verdict, d_co, d_tally, d_per;
  if (!images_upload(cfg, src, n, d_img, d_idx, g)) { (void)hipGetLastError(); return AFE_ERR_HIP; }
  if (!d_v.upload(vel0, (size_t)n * 24) || !d_a.upload(acc0, (size_t)n * 24) || !d_s.upload(samples, (size_t)n_tables * n_candidates * 32) ||
      (sample_table && !d_t.upload(sample_table, (size_t)n * 4)) || !d_flags.upload(flags, total) || !d_verdict.alloc(total) ||
      (coeffs_out && !d_co.alloc(total * 144)) || !d_tally.alloc(48) || hipMemset(d_tally.get(), 0, 48) != hipSuccess ||
      (per_planner && !d_per.alloc((size_t)n * 48))) {
    (void)hipGetLastError();
    return AFE_ERR_HIP;
  }
  g.vel0 = (const double *)d_v.get(); g.acc0 = (const double *)d_a.get(); g.samples = (const double *)d_s.get();
  g.sample_table = sample_table ? (const int32_t *)d_t.get() : nullptr;
  g.verdict_out = (uint8_t *)d_verdict.get();
  g.coeffs_out = (double *)d_co.get();

  float ms = 0;
  StreamTimer timer(nullptr, true);
  if (!timer.ok()) return AFE_ERR_HIP;
  rc = truth_launch<MODE_CANDS>(g, false, nullptr);
  if (rc == AFE_OK) {
    hipLaunchKernelGGL(afe_truth_tally_kernel, dim3((unsigned)n), dim3(64), 0, nullptr, (const uint8_t *)d_flags.get(), (const uint8_t *)d_verdict.get(), n,
                       n_candidates, (unsigned long long *)d_tally.get(), (int64_t *)d_per.get());
    rc = hipGetLastError() == hipSuccess ? AFE_OK : AFE_ERR_HIP;
  }
  rc = timer.finish(rc, &ms);
  if (rc != AFE_OK) return rc;
  afe_conservativeness sum;
  if (!d_tally.download(&sum, 48) || !d_verdict.download(verdict_out, total) || (coeffs_out && !d_co.download(coeffs_out, total * 144)) ||
      (per_planner && !d_per.download(per_planner, (size_t)n * 48)))
    return AFE_ERR_HIP;
  *tally = sum;
  if (kernel_ms) *kernel_ms = ms;
  return AFE_OK;
}
