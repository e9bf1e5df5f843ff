// Streaming evaluation labels (crn_eval_labels / crn_eval_labels_cpu): what the HIP kernel and its host twin share.
// Contract: include/corenet_hip.h and DESIGN section 16.
#pragma once
#include <stdint.h>

#include "../../include/corenet_hip.h"

#if defined(__HIP__)
#define EL_HD __host__ __device__ inline
#else
#define EL_HD inline
#endif

// Whether the product of `count` positive factors is at most INT64_MAX.
inline bool el_product_fits(const int64_t* factors, int count) {
  int64_t product = 1;
  for (int i = 0; i < count; ++i) {
    if (product > INT64_MAX / factors[i]) return false;
    product *= factors[i];
  }
  return true;
}

// Every argument rule of the two entry points; nothing is launched or written when this fails.
inline bool el_args_ok(const float* scores, const int32_t* gt, int B, int C, int K, int D, int H, int W, int m, int n,
                       const int32_t* labels, const int64_t* cm, const int32_t* bad) {
  if (!scores || B < 1 || C < 1 || C > CRN_EVAL_MAX_CLASSES || K < 1 || K > CRN_EVAL_MAX_BINS || D < 1 || H < 1 || W < 1) return false;
  if (m < 1 || n < 0) return false;
  // the byte offsets of the score tensor (B * C * S floats) and of the fine grid (B * S * m^3 labels) must fit int64:
  // the index arithmetic of kernel and twin is 64-bit and would wrap beyond that
  const int64_t score_factors[] = {B, C, D, H, W, 4}, fine_factors[] = {B, D, H, W, m, m, m, 4};
  if (!el_product_fits(score_factors, 6) || !el_product_fits(fine_factors, 8)) return false;
  if (n >= (int64_t)m * m * m) return false;                 // (m^3 fits: it is a factor of the product above)
  if (gt && (!cm || !bad)) return false;
  if (!gt && !labels) return false;                          // nothing to compute
  return true;
}

// First maximum over the C scores p[0], p[stride], ...: only a strictly larger score replaces the running best, so a NaN
// never does and a NaN at class 0 stays (argmax_confusion_kernel's rule).
template <int CT>
EL_HD int el_argmax(const float* p, int C, int64_t stride) {
  float best = *p;
  int bi = 0;
#pragma unroll
  for (int c = 1; c < CT; ++c) {
    if (c < C) {
      p += stride;
      const float x = *p;
      if (x > best) { best = x; bi = c; }
    }
  }
  return bi;
}

// Histogram bin of a (ground truth, prediction) pair, both already scaled by the scene class: g * K + pred, or -1 when
// either is outside [0, K) (counted in bad[0]).
EL_HD int el_bin(int64_t g, int64_t pred, int K) {
  return (g >= 0 && g < K && pred >= 0 && pred < K) ? (int)(g * K + pred) : -1;
}
