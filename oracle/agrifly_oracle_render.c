/* agrifly_oracle_render.c -- see agrifly_oracle_render.h (TEST INFRASTRUCTURE ONLY). */
#include "agrifly_oracle_render.h"

#include <math.h>

void ora_quat_mul(const double a[4], const double b[4], double out[4]) {
  /* Rotation.hpp:124-131: (this = a) * (r1 = b) */
  const double c0 = b[0] * a[0] - b[1] * a[1] - b[2] * a[2] - b[3] * a[3];
  const double c1 = b[1] * a[0] + b[0] * a[1] + b[3] * a[2] - b[2] * a[3];
  const double c2 = b[2] * a[0] - b[3] * a[1] + b[0] * a[2] + b[1] * a[3];
  const double c3 = b[3] * a[0] + b[2] * a[1] - b[1] * a[2] + b[0] * a[3];
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

void ora_quat_to_matrix(const double q[4], double R[9]) {
  /* Rotation.hpp:196-220 */
  const double r0 = q[0] * q[0], r1 = q[1] * q[1], r2 = q[2] * q[2], r3 = q[3] * q[3];
  R[0] = r0 + r1 - r2 - r3;
  R[1] = 2 * q[1] * q[2] - 2 * q[0] * q[3];
  R[2] = 2 * q[1] * q[3] + 2 * q[0] * q[2];
  R[3] = 2 * q[1] * q[2] + 2 * q[0] * q[3];
  R[4] = r0 - r1 + r2 - r3;
  R[5] = 2 * q[2] * q[3] - 2 * q[0] * q[1];
  R[6] = 2 * q[1] * q[3] - 2 * q[0] * q[2];
  R[7] = 2 * q[2] * q[3] + 2 * q[0] * q[1];
  R[8] = r0 - r1 - r2 + r3;
}

static double dot3(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static void cross3(const double a[3], const double b[3], double o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

/* ray o + t d against one CLOSED triangle; returns t or +inf.  Two-sided, t > 0.
 *
 * Watertight across shared edges.  The barycentric numerators N_u = tv.(d x e2), N_v = d.(tv x e1),
 * N_w = det - N_u - N_v are each a 3x3 determinant of tv / e1, d, e2: six triple products, every one
 * bounded by |a|_1 |b|_1 |c|_1 of its columns and carrying at most 7 roundings (difference that forms
 * tv or e, two products, cross subtraction, dot product and its two additions), and N_w adds those of
 * det, N_u, N_v and its own two subtractions: 9 u (|det| + |N_u| + |N_v|) <= 18 u K with u = 2^-53 and
 *   K = |d|_1 max(|e1|_1, |e2|_1) (|tv|_1 + max(|e1|_1, |e2|_1)).
 * eps = 2^-48 K = 32 u K covers that and the roundings of K itself, so a ray that lies in the closed
 * triangle -- exact numerators >= 0 on the determinant's side -- is always accepted, whichever way the
 * products round: two triangles that share an edge cannot both turn away a ray that runs along it.
 * What is accepted beyond the triangle is at most 2 eps / |det| in barycentric terms (the judge of
 * tests/render_judge.py allows 8 eps / |det|).
 * A determinant within eps of zero has no reliable sign (the triangle is edge-on to the ray as far as
 * fp64 can tell) and hits nothing; one within 2^15 en eps is turned away as well, so that everything
 * accepted lies within 3 (2 eps / |det|) en < 2^-12 m of the triangle itself -- inside the boxes the
 * engine's hierarchy inflates by 3e-4 m.  The cutoff scales with the operands: the earlier absolute
 * 1e-12 did not.  t is computed as before. */
static double ray_triangle(const double o[3], const double d[3], double dn, const float *tri) {
  const double v0[3] = {tri[0], tri[1], tri[2]};
  const double e1[3] = {(double)tri[3] - v0[0], (double)tri[4] - v0[1], (double)tri[5] - v0[2]};
  const double e2[3] = {(double)tri[6] - v0[0], (double)tri[7] - v0[1], (double)tri[8] - v0[2]};
  double p[3], q[3];
  cross3(d, e2, p);
  const double det = dot3(e1, p);
  const double tv[3] = {o[0] - v0[0], o[1] - v0[1], o[2] - v0[2]};
  /* the triangle's factors (the engine keeps them with the triangle) and the ray's dn = |d|_1 (kept with the ray) */
  const double en = fmax(fabs(e1[0]) + fabs(e1[1]) + fabs(e1[2]), fabs(e2[0]) + fabs(e2[1]) + fabs(e2[2]));
  const double k1 = 0x1p-48 * en, cut = fmax(1.0, 32768.0 * en);
  const double tn = fabs(tv[0]) + fabs(tv[1]) + fabs(tv[2]);
  const double eps = (dn * k1) * (tn + en);
  if (!(fabs(det) > eps * cut)) return INFINITY;
  const double s = det > 0.0 ? 1.0 : -1.0;
  const double nu = dot3(tv, p) * s;
  if (nu < -eps) return INFINITY;
  cross3(tv, e1, q);
  const double nv = dot3(d, q) * s;
  if (nv < -eps) return INFINITY;
  if ((fabs(det) - nu) - nv < -eps) return INFINITY;
  const double inv = 1.0 / det;
  const double t = dot3(e2, q) * inv;
  return t > 0.0 ? t : INFINITY;
}

static void camera_frame(const double att[4], const double mount[4], double R[9]) {
  double q[4];
  ora_quat_mul(att, mount, q);
  ora_quat_to_matrix(q, R);
}

static double pixel_depth(const ora_camera *cam, const float *triangles, int64_t n_tri, const double o[3],
                          const double R[9], int px, int py) {
  const double u = (px - cam->cx) / cam->focal_length;
  const double v = (py - cam->cy) / cam->focal_length;
  /* camera-frame ray (u, v, 1): t along it IS the camera-frame z of the hit */
  const double d[3] = {R[0] * u + R[1] * v + R[2], R[3] * u + R[4] * v + R[5], R[6] * u + R[7] * v + R[8]};
  const double dn = fabs(d[0]) + fabs(d[1]) + fabs(d[2]);
  double best = INFINITY;
  for (int64_t k = 0; k < n_tri; k++) {
    const double t = ray_triangle(o, d, dn, triangles + 9 * k);
    if (t < best) best = t;
  }
  return best;
}

static uint16_t quantise(const ora_camera *cam, double z) {
  if (!(z < INFINITY)) return (uint16_t)cam->max_count;
  const double c = floor(z / cam->depth_scale);
  return (uint16_t)(c < cam->max_count ? c : cam->max_count);
}

void ora_render_depth(const ora_camera *cam, const float *triangles, int64_t n_tri, const double cam_pos[3],
                      const double att[4], const double mount[4], uint16_t *out) {
  double R[9];
  camera_frame(att, mount, R);
  /* rows are independent: the same per-pixel arithmetic whatever the thread count */
#pragma omp parallel for schedule(dynamic, 4)
  for (int py = 0; py < cam->height; py++)
    for (int px = 0; px < cam->width; px++)
      out[(int64_t)py * cam->width + px] = quantise(cam, pixel_depth(cam, triangles, n_tri, cam_pos, R, px, py));
}

double ora_render_pixel_depth(const ora_camera *cam, const float *triangles, int64_t n_tri,
                              const double cam_pos[3], const double att[4], const double mount[4], int px,
                              int py) {
  double R[9];
  camera_frame(att, mount, R);
  return pixel_depth(cam, triangles, n_tri, cam_pos, R, px, py);
}
