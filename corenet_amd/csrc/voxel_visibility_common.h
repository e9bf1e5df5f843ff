// Voxel visibility from an eye (crn_voxel_visibility and its host twin): what the HIP kernels and the twin share -- the
// occupancy rule, the integer walk and the argument checks.  Contract: include/corenet_hip.h,
// corenet_amd/voxel_visibility.py and DESIGN section 19.
#pragma once
#include <stdint.h>

#include "../../include/corenet_hip.h"

#if defined(__HIP__)
#define VV_HD __host__ __device__ inline
#else
#define VV_HD inline
#endif

// dtype codes of the grid (those of crn_fill_voxels)
constexpr int VV_U8 = 1, VV_I32 = 2;
constexpr int64_t VV_NEVER = INT64_MAX;          // the crossing term of an axis the segment does not move along

template <typename T>
VV_HD bool vv_occupied(T v) { return v > 0; }

// The walk of one voxel towards its eye.  With t in (0, 1) along the segment from the centre c to the eye e = c + delta,
// the k-th face across axis a is crossed at t = (128 + 256 k) / |delta_a|.  All terms are multiplied by the product of the
// non-zero |delta_b|, so they are integers: T[a] = (128 + 256 k) * prod_{b != a} |delta_b|, the eye lies at t_end = the
// whole product.  |delta_a| <= 2^20 (vv_args_ok), so t_end <= 2^60 and no term exceeds t_end + 2^48 < 2^61.
struct VvWalk {
  int64_t T[3], inc[3], t_end;
  int pos[3], sign[3];
};

// v: the voxel (x, y, z); eye: (x, y, z) in 1/256 voxel.
VV_HD VvWalk vv_start(int x, int y, int z, const int32_t* eye) {
  VvWalk k;
  k.pos[0] = x; k.pos[1] = y; k.pos[2] = z;
  int64_t a[3];
  for (int i = 0; i < 3; ++i) {
    const int delta = eye[i] - (k.pos[i] * CRN_VV_SUBDIVISIONS + CRN_VV_SUBDIVISIONS / 2);
    k.sign[i] = delta > 0 ? 1 : delta < 0 ? -1 : 0;
    a[i] = delta < 0 ? -(int64_t)delta : (int64_t)delta;
  }
  const int64_t f[3] = {a[0] ? a[0] : 1, a[1] ? a[1] : 1, a[2] ? a[2] : 1};
  k.t_end = f[0] * f[1] * f[2];
  for (int i = 0; i < 3; ++i) {
    const int64_t others = f[(i + 1) % 3] * f[(i + 2) % 3];
    k.inc[i] = CRN_VV_SUBDIVISIONS * others;
    k.T[i] = a[i] ? (CRN_VV_SUBDIVISIONS / 2) * others : VV_NEVER;
  }
  return k;
}

// One step: false once the walk reached the eye or left the grid (convex: it does not come back).  Every axis whose term
// equals the minimum moves, so a segment through an edge or a corner enters the voxel diagonally across it.  Each step
// moves one axis or more towards leaving the grid: at most D + H + W steps.
VV_HD bool vv_step(VvWalk& k, int D, int H, int W) {
  int64_t m = k.T[0] < k.T[1] ? k.T[0] : k.T[1];
  m = k.T[2] < m ? k.T[2] : m;
  if (m >= k.t_end) return false;
  for (int i = 0; i < 3; ++i)
    if (k.T[i] == m) { k.pos[i] += k.sign[i]; k.T[i] += k.inc[i]; }
  return (unsigned)k.pos[0] < (unsigned)W && (unsigned)k.pos[1] < (unsigned)H && (unsigned)k.pos[2] < (unsigned)D;
}

// The packed occupancy of a grid: row (z, y) is words64(W) 64-bit words, bit x & 63 of word x >> 6.
VV_HD int vv_words64(int W) { return (W + 63) >> 6; }
VV_HD bool vv_bit(const uint64_t* bits, int words, int H, int x, int y, int z) {
  return (bits[((int64_t)z * H + y) * words + (x >> 6)] >> (x & 63)) & 1;
}

// Every argument rule of crn_voxel_visibility(_cpu); nothing is launched or written when this fails.  N == 0 is valid
// (and nothing is done).  known_flags: the flags of the entry.
inline bool vv_args_ok(const void* grid, const int64_t* strides, int dtype, int N, int D, int H, int W, const int32_t* eye_q,
                       int flags, int known_flags, const uint8_t* occluded) {
  if (N < 0 || D < 1 || H < 1 || W < 1) return false;
  if (D > CRN_VV_MAX_EXTENT || H > CRN_VV_MAX_EXTENT || W > CRN_VV_MAX_EXTENT) return false;
  if ((int64_t)D * H > INT32_MAX / W) return false;                       // `first` is 32-bit per grid
  if (dtype != VV_U8 && dtype != VV_I32) return false;
  if (flags & ~known_flags) return false;
  if (N == 0) return true;
  if (!grid || !strides || !eye_q || !occluded) return false;
  if (strides[3] != 1 || strides[0] < 0 || strides[1] < 0 || strides[2] < 0) return false;
  if ((int64_t)D * H * W > INT64_MAX / 8 / N) return false;               // byte offsets of the outputs fit int64
  for (int64_t i = 0; i < (int64_t)N * 3; ++i)
    if (eye_q[i] > CRN_VV_MAX_EYE || eye_q[i] < -CRN_VV_MAX_EYE) return false;
  return true;
}
