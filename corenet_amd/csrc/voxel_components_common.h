// Voxel connected components (crn_voxel_components / crn_component_stats and their host twins): what the HIP kernels
// and the twin share.  Contract: include/corenet_hip.h, corenet_amd/voxel_components.py and DESIGN section 17.
#pragma once
#include <stdint.h>

#include "../../include/corenet_hip.h"

#if defined(__HIP__)
#define VC_HD __host__ __device__ inline
#else
#define VC_HD inline
#endif

// dtype codes of the grid (those of crn_fill_voxels)
constexpr int VC_U8 = 1, VC_I32 = 2;

// connectivity 6 / 18 / 26 -> the largest |dd| + |dh| + |dw| of a neighbour offset (1 / 2 / 3); anything else 0
VC_HD int vc_level(int connectivity) { return connectivity == 6 ? 1 : connectivity == 18 ? 2 : connectivity == 26 ? 3 : 0; }

// The key two neighbours compare: 0 on background (v <= 0), else the value (by_value) or 1.
template <typename T>
VC_HD int32_t vc_key(T v, int by_value) { return v > 0 ? (by_value ? (int32_t)v : 1) : 0; }

// Every argument rule of crn_voxel_components(_cpu); nothing is launched or written when this fails.
inline bool vc_args_ok(const void* grid, const int64_t* strides, int dtype, int N, int D, int H, int W, int connectivity,
                       const int32_t* labels, const int64_t* num) {
  if (!grid || !strides || !labels || !num || N < 1 || D < 1 || H < 1 || W < 1) return false;
  if (dtype != VC_U8 && dtype != VC_I32) return false;
  if (!vc_level(connectivity)) return false;
  if (strides[3] != 1 || strides[0] < 0 || strides[1] < 0 || strides[2] < 0) return false;
  if ((int64_t)D * H > INT32_MAX / W) return false;                       // labels and parents are 32-bit per grid
  if ((int64_t)D * H * W > INT64_MAX / 8 / N) return false;               // byte offsets of labels fit int64
  return true;
}

inline bool vc_stats_args_ok(const int32_t* labels, const void* grid, const int64_t* strides, int dtype, int N, int D, int H, int W,
                             const int64_t* offsets, int64_t K, const int64_t* size, const int32_t* bbox, const int64_t* first,
                             const int32_t* value) {
  if (!labels || !offsets || N < 1 || D < 1 || H < 1 || W < 1 || K < 0) return false;
  if (K > 0 && (!size || !bbox || !first)) return false;
  if (grid && (!strides || !value || strides[3] != 1 || (dtype != VC_U8 && dtype != VC_I32))) return false;
  if ((int64_t)D * H > INT32_MAX / W) return false;
  if ((int64_t)D * H * W > INT64_MAX / 8 / N) return false;
  return true;
}
