// Surface sampling and nearest-neighbour distances: the per-element arithmetic shared by the HIP kernels
// (point_metrics.hip) and the host twin (point_metrics_cpu.cpp).  Both include this header and both are compiled with
// -ffp-contract=off, so an area, a weight, a sample and a squared distance are the same IEEE operations in the same
// order on either side (sqrtf, the float and the double divide are correctly rounded on both).
// Contract: corenet_amd/mesh_metrics.py, include/corenet_hip.h and DESIGN section 15.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__)
#define CRN_PM_HD __host__ __device__ inline
#else
#define CRN_PM_HD inline
#endif

// ---------------- random numbers: a counter-based hash of (seed, sample, which) ----------------
CRN_PM_HD uint32_t pm_fmix(uint32_t x) {          // the murmur3 finaliser: a bijection of 32 bits that mixes every bit
  x ^= x >> 16;
  x *= 0x85ebca6bu;
  x ^= x >> 13;
  x *= 0xc2b2ae35u;
  x ^= x >> 16;
  return x;
}

CRN_PM_HD uint32_t pm_hash(uint32_t seed, uint32_t i, uint32_t which) {
  uint32_t h = pm_fmix(seed ^ 0x9e3779b9u);
  h = pm_fmix(h ^ i);
  return pm_fmix(h + which * 0x85ebca6bu + 1u);
}

// uniform in [0, 1): the hash's upper 24 bits as a mantissa (exact in float32)
CRN_PM_HD float pm_uniform(uint32_t seed, uint32_t i, uint32_t which) {
  return (float)(pm_hash(seed, i, which) >> 8) * (1.0f / 16777216.0f);
}

// ---------------- area weights ----------------
// |cross(B - A, C - A)| of the triangle p[9] (twice its area; only ratios are used)
CRN_PM_HD float pm_area(const float* p) {
  const float e1x = p[3] - p[0], e1y = p[4] - p[1], e1z = p[5] - p[2];
  const float e2x = p[6] - p[0], e2y = p[7] - p[1], e2z = p[8] - p[2];
  const float cx = e1y * e2z - e1z * e2y;
  const float cy = e1z * e2x - e1x * e2z;
  const float cz = e1x * e2y - e1y * e2x;
  return sqrtf((cx * cx + cy * cy) + cz * cz);
}

// an area that can carry samples: positive and finite (NaN fails both tests)
CRN_PM_HD bool pm_area_ok(float a) { return a > 0.f && a < INFINITY; }

// Integer weight of area a in an object whose largest eligible area is amax: round(a / amax * 2^24) in [0, 2^24].  The
// maximum does not depend on the order it is taken in and the divide is correctly rounded, so every weight -- and every
// integer sum of weights -- is the same wherever and however it is computed.
#define CRN_PM_WEIGHT_ONE 16777216.0f
CRN_PM_HD int64_t pm_weight(float a, float amax) {
  if (!(pm_area_ok(a) && a <= amax)) return 0;
  return (int64_t)rintf((a / amax) * CRN_PM_WEIGHT_ONE);
}

// Stratified position of sample i of S in [0, total): floor(((i + u) / S) * total), in double (IEEE on both sides)
CRN_PM_HD int64_t pm_target(int64_t i, float u, int64_t S, int64_t total) {
  const double x = ((double)i + (double)u) / (double)S;
  int64_t p = (int64_t)(x * (double)total);
  if (p > total - 1) p = total - 1;
  return p < 0 ? 0 : p;
}

// first k in [lo, hi) with cum[k] > p; cum = inclusive sums of the weights (non-decreasing), cum[hi - 1] > p
CRN_PM_HD int64_t pm_find(const int64_t* cum, int64_t lo, int64_t hi, int64_t p) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (cum[mid] > p) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// square-root warp: (u1, u2) uniform in the unit square -> a point uniform in the triangle p[9]
CRN_PM_HD void pm_point(const float* p, float u1, float u2, float* out) {
  const float r = sqrtf(u1);
  const float b0 = 1.0f - r, b1 = r * (1.0f - u2), b2 = r * u2;
  for (int c = 0; c < 3; ++c) out[c] = (b0 * p[c] + b1 * p[3 + c]) + b2 * p[6 + c];
}

// sample i of an object: its triangles are [t0, t1) of tri, cum their inclusive weight sums (total = cum[t1 - 1] > 0)
CRN_PM_HD void pm_sample(const float* tri, const int64_t* cum, int64_t t0, int64_t t1, int64_t total, int64_t i, int64_t S,
                         uint32_t seed, float* point, int32_t* tri_index) {
  const int64_t p = pm_target(i, pm_uniform(seed, (uint32_t)i, 0u), S, total);
  const int64_t k = pm_find(cum, t0, t1, p);
  pm_point(tri + 9 * k, pm_uniform(seed, (uint32_t)i, 1u), pm_uniform(seed, (uint32_t)i, 2u), point);
  *tri_index = (int32_t)(k - t0);
}

// ---------------- nearest neighbour ----------------
CRN_PM_HD float pm_d2(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

// ---------------- point to triangle ----------------
// A triangle is reduced once to a record of PM_TRI_REC floats: an orthonormal frame at A (u along AB, v in the plane
// towards C, n = u x v) and the triangle in that frame, A = (0, 0), B = (l1, 0), C = l2 * (c2x, c2y), with the unit
// direction and the length of every edge:
//   [0..2] A   [3..5] u   [6..8] v   [9..11] n   [12] l1 = |AB|
//   [13] c2x [14] c2y [15] l2 = |AC|       (unit direction of A -> C in the frame; c2y > 0)
//   [16] c3x [17] c3y [18] l3 = |BC|       (unit direction of B -> C)         [19] 0
// v is made orthogonal to u twice (Gram-Schmidt, then once more on the normalised vector) and n is their cross product,
// so the frame is orthonormal to rounding however thin the triangle is; what a sliver loses is the direction of v about
// its long axis, which moves no point of it by more than rounding.  A triangle that is not eligible
// (pm_area_ok(pm_area) fails), or whose frame is not finite, gives a record of NaNs: every distance to it is NaN or +inf
// and it is never chosen.
#define PM_TRI_REC 20
CRN_PM_HD void pm_tri_record(const float* p, float* r) {
  const float e1x = p[3] - p[0], e1y = p[4] - p[1], e1z = p[5] - p[2];
  const float e2x = p[6] - p[0], e2y = p[7] - p[1], e2z = p[8] - p[2];
  const float l1 = sqrtf((e1x * e1x + e1y * e1y) + e1z * e1z);
  const float ux = e1x / l1, uy = e1y / l1, uz = e1z / l1;
  const float k = (e2x * ux + e2y * uy) + e2z * uz;
  float wx = e2x - k * ux, wy = e2y - k * uy, wz = e2z - k * uz;
  float lw = sqrtf((wx * wx + wy * wy) + wz * wz);
  wx = wx / lw; wy = wy / lw; wz = wz / lw;
  const float k2 = (wx * ux + wy * uy) + wz * uz;                  // what the first pass left of u in w: rounding / sin
  wx = wx - k2 * ux; wy = wy - k2 * uy; wz = wz - k2 * uz;
  lw = sqrtf((wx * wx + wy * wy) + wz * wz);
  const float vx = wx / lw, vy = wy / lw, vz = wz / lw;
  const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  const float cx = (e2x * ux + e2y * uy) + e2z * uz, cy = (e2x * vx + e2y * vy) + e2z * vz;
  const float l2 = sqrtf(cx * cx + cy * cy);
  const float bx = cx - l1;
  const float l3 = sqrtf(bx * bx + cy * cy);
  r[0] = p[0]; r[1] = p[1]; r[2] = p[2];
  r[3] = ux; r[4] = uy; r[5] = uz;
  r[6] = vx; r[7] = vy; r[8] = vz;
  r[9] = nx; r[10] = ny; r[11] = nz;
  r[12] = l1;
  r[13] = cx / l2; r[14] = cy / l2; r[15] = l2;
  r[16] = bx / l3; r[17] = cy / l3; r[18] = l3;
  r[19] = 0.f;
  float sum = 0.f;                                                 // finite exactly when every term is finite
  for (int i = 0; i < PM_TRI_REC; ++i) sum += r[i] * 0.f;
  const bool ok = pm_area_ok(pm_area(p)) && sum == 0.f;
  for (int i = 0; i < PM_TRI_REC; ++i) r[i] = ok ? r[i] : NAN;
}

// squared distance of one edge in the frame: (tx, ty) the query relative to the edge's start, (cx, cy) the edge's unit
// direction, l its length.  s is the signed distance to the edge's line (positive on its left), a what the projection
// lies outside [0, l] by.
CRN_PM_HD float pm_edge_d2(float tx, float ty, float cx, float cy, float l, float* s) {
  const float along = tx * cx + ty * cy;
  *s = cx * ty - cy * tx;
  float c = along < 0.f ? 0.f : along;
  c = c > l ? l : c;
  const float a = along - c;
  return *s * *s + a * a;
}

// Squared distance from (px, py, pz) to the closed triangle of record r: the query in the frame is (x, y, z); the
// distance is z * z plus the squared distance of (x, y) to the triangle in its plane, which is 0 inside (on the left
// of A -> B and B -> C and on the right of A -> C) and the smallest of the three clamped edge distances elsewhere.
// Selects only.  A NaN in the query or the record makes z, and with it the result, NaN.
CRN_PM_HD float pm_tri_d2(float px, float py, float pz, const float* r) {
  const float dx = px - r[0], dy = py - r[1], dz = pz - r[2];
  const float x = (dx * r[3] + dy * r[4]) + dz * r[5];
  const float y = (dx * r[6] + dy * r[7]) + dz * r[8];
  const float z = (dx * r[9] + dy * r[10]) + dz * r[11];
  float c = x < 0.f ? 0.f : x;
  c = c > r[12] ? r[12] : c;
  const float a1 = x - c;
  const float q1 = y * y + a1 * a1;
  float s2, s3;
  const float q2 = pm_edge_d2(x, y, r[13], r[14], r[15], &s2);
  const float q3 = pm_edge_d2(x - r[12], y, r[16], r[17], r[18], &s3);
  float m = q2 < q1 ? q2 : q1;
  m = q3 < m ? q3 : m;
  const bool inside = (y >= 0.f) & (s2 <= 0.f) & (s3 >= 0.f);
  const float in_plane = inside ? 0.f : m;
  return z * z + in_plane;
}
