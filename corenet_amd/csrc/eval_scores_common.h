// Score-level evaluation (crn_eval_scores / crn_eval_scores_cpu, crn_score_softmax): what the HIP kernel and its host
// twin share -- the argument rules, the softmax and every integer formula of an entry.  Contract:
// include/corenet_hip.h and DESIGN section 22.  Both builds compile with -ffp-contract=off and nothing here calls a
// math library: the float operations below are IEEE +, *, / and comparisons, which round alike on host and device.
#pragma once
#include <stdint.h>

#include "../../include/corenet_hip.h"
#include "eval_labels_common.h"

#define ES_HD EL_HD

constexpr int ES_ONE = 1 << 24;                              // q of probability 1

// Every argument rule the two entry points share; nothing is launched or written when this fails.
inline bool es_args_ok(const float* scores, const int32_t* gt, int B, int C, int K, int D, int H, int W, int m, int n, int nbins,
                       const int64_t* table, const int64_t* sq, const int64_t* bad) {
  if (!gt || !table || !sq || !bad) return false;
  if (nbins < 1 || nbins > CRN_SCORE_MAX_NBINS) return false;
  int32_t unused = 0;                                        // el_args_ok's "labels": any non-null pointer
  if (!el_args_ok(scores, gt, B, C, K, D, H, W, m, n, &unused, table, &unused)) return false;
  return (K + 1) * nbins <= CRN_SCORE_MAX_ENTRIES;
}

inline bool es_softmax_args_ok(const float* logits, int B, int C, int64_t S, const float* out) {
  if (!logits || !out || B < 1 || C < 1 || C > CRN_EVAL_MAX_CLASSES || S < 1) return false;
  const int64_t factors[] = {B, C, S, 4};
  return el_product_fits(factors, 4);
}

ES_HD float es_from_bits(uint32_t u) { return __builtin_bit_cast(float, u); }

// exp(t) for t <= 0 (t = x - max of a softmax): 0 below -87, so that no denormal is ever produced; NaN for a NaN (or,
// never reached from es_softmax, a positive t).  n = t * log2(e) rounded to nearest by the 1.5 * 2^23 trick,
// r = t - n * ln2 in two pieces (|r| <= 0.347), the degree-7 Taylor polynomial of exp(r) in Horner form (truncation
// below 6e-9 relative), times 2^n assembled by bits (n >= -126; at n = -126 r is positive, so the product is normal).
ES_HD float es_exp(float t) {
  if (t < -87.f) return 0.f;
  if (!(t <= 0.f)) return es_from_bits(0x7fc00000u);
  const float f = t * 1.44269504088896341f;
  const float nf = (f + 12582912.f) - 12582912.f;
  const float r = (t - nf * 0.693145751953125f) - nf * 1.42860682030941723e-6f;
  float p = 1.98412698412698413e-4f;
  p = p * r + 1.38888888888888894e-3f;
  p = p * r + 8.33333333333333322e-3f;
  p = p * r + 4.16666666666666644e-2f;
  p = p * r + 1.66666666666666657e-1f;
  p = p * r + 0.5f;
  p = p * r + 1.f;
  p = p * r + 1.f;
  return p * es_from_bits((uint32_t)((int)nf + 127) << 23);
}

// The shared softmax, in place over x[0..C): first maximum (el_argmax's rule: a NaN at channel 0 stays, one elsewhere
// never becomes the maximum but poisons the sum), e_c = es_exp(x_c - max), the sum in channel order, one division per
// channel.  A quotient below FLT_MIN becomes 0 (whether the divider keeps denormals does not matter then), a NaN the
// canonical quiet NaN.
template <int CT>
ES_HD void es_softmax(float* x, int C) {
  float best = x[0];
#pragma unroll
  for (int c = 1; c < CT; ++c)
    if (c < C && x[c] > best) best = x[c];
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if (c < C) { x[c] = es_exp(x[c] - best); sum = sum + x[c]; }
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if (c < C) {
      float p = x[c] / sum;
      if (p < 1.17549435e-38f) p = 0.f;
      if (p != p) p = es_from_bits(0x7fc00000u);
      x[c] = p;
    }
}

ES_HD bool es_p_ok(float p) { return p >= 0.f && p <= 1.f; }                     // false for a NaN

// p in [0, 1] -> q in [0, 2^24]: p * 2^24 is exact, the rounding is to nearest even
ES_HD int es_q(float p) { return (int)rintf(p * 16777216.f); }

ES_HD int es_bin(int q, int nbins) {
  const int64_t b = ((int64_t)q * nbins) >> 24;
  return b < nbins - 1 ? (int)b : nbins - 1;
}

// squared error of an entry in units of 2^-24: e = |y - p| in q24, to 16 bits, squared, back to 24 bits
ES_HD uint32_t es_sq(int q, int y) {
  const uint64_t e = (uint64_t)(y ? ES_ONE - q : q), e16 = (e + 128) >> 8;
  return (uint32_t)((e16 * e16 + 128) >> 8);
}
