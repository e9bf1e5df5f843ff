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
