// Exact squared Euclidean distance transform (crn_voxel_distance and its host twin): what the HIP kernels and the twin
// share.  Contract: include/corenet_hip.h, corenet_amd/voxel_distance.py and DESIGN section 18.
#pragma once
#include <stdint.h>

#include "../../include/corenet_hip.h"

#if defined(__HIP__)
#define VD_HD __host__ __device__ inline
#else
#define VD_HD inline
#endif

// dtype codes of the grid (those of crn_fill_voxels)
constexpr int VD_U8 = 1, VD_I32 = 2;

template <typename T>
VD_HD bool vd_fg(T v) { return v > 0; }

// The target rule.  g: the grid (n already applied), element strides sD / sH along d / h, 1 along w.  SURFACE: a foreground
// voxel with one of its 6 neighbours not foreground or outside the grid.
template <typename T>
VD_HD bool vd_target(const T* g, int64_t sD, int64_t sH, int D, int H, int W, int d, int h, int w, int mode) {
  const T* p = g + d * sD + h * sH + w;
  const bool f = vd_fg(*p);
  if (mode == CRN_VD_FOREGROUND) return f;
  if (mode == CRN_VD_BACKGROUND) return !f;
  if (!f) return false;
  if (d == 0 || h == 0 || w == 0 || d == D - 1 || h == H - 1 || w == W - 1) return true;
  return !(vd_fg(p[-1]) && vd_fg(p[1]) && vd_fg(p[-sH]) && vd_fg(p[sH]) && vd_fg(p[-sD]) && vd_fg(p[sD]));
}

// Every argument rule of crn_voxel_distance(_cpu); nothing is launched or written when this fails.  N == 0 is valid (and
// nothing is done).  The largest squared distance of a grid, (D-1)^2 + (H-1)^2 + (W-1)^2, stays below CRN_VD_NO_TARGET.
inline bool vd_args_ok(const void* grid, const int64_t* strides, int dtype, int N, int D, int H, int W, int mode, const int32_t* d2) {
  if (N < 0 || D < 1 || H < 1 || W < 1) return false;
  if (dtype != VD_U8 && dtype != VD_I32) return false;
  if (mode != CRN_VD_FOREGROUND && mode != CRN_VD_BACKGROUND && mode != CRN_VD_SURFACE) return false;
  if ((int64_t)D * H > INT32_MAX / W) return false;                       // the index is 32-bit per grid
  const int64_t e = (int64_t)(D - 1) * (D - 1) + (int64_t)(H - 1) * (H - 1) + (int64_t)(W - 1) * (W - 1);
  if (e >= CRN_VD_NO_TARGET) return false;
  if (N == 0) return true;
  if (!grid || !strides || !d2) return false;
  if (strides[3] != 1 || strides[0] < 0 || strides[1] < 0 || strides[2] < 0) return false;
  if ((int64_t)D * H * W > INT64_MAX / 8 / N) return false;               // byte offsets of the outputs fit int64
  return true;
}
