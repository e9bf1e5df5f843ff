// Configuration histogram of voxel grids (crn_voxel_topology and its host twin): what the HIP kernel and the twin share
// -- the bit order of a cell's code, the rule that turns a voxel value into a label and the argument checks.  Contract:
// include/corenet_hip.h, corenet_amd/voxel_topology.py and DESIGN section 23.
#pragma once
#include <stdint.h>

#include "../../include/corenet_hip.h"

#if defined(__HIP__)
#define VT_HD __host__ __device__ inline
#else
#define VT_HD inline
#endif

// dtype codes of the grids (those of crn_voxel_components)
constexpr int VT_U8 = 1, VT_I32 = 2;

// Cell (d, h, w) holds the voxels (d - 1 + i, h - 1 + j, w - 1 + k); voxel (i, j, k) is bit 4 * i + 2 * j + k of its code.
// The two voxels of one W row of a cell, (w - 1, w), are therefore the bit pair at VT_ROW_SHIFT(i, j).
VT_HD constexpr int vt_row_shift(int i, int j) { return 4 * i + 2 * j; }

// The label of a voxel value: mask grids (mask != 0) have the single label "non-zero"; label grids keep 0 .. L and turn
// every other value into background, which *bad is told about.
VT_HD int32_t vt_label(int32_t v, int32_t L, int mask, bool* bad) {
  *bad = false;
  if (mask) return v != 0;
  if ((uint32_t)v <= (uint32_t)L) return v;
  *bad = true;
  return 0;
}

VT_HD int64_t vt_cells(int D, int H, int W) { return ((int64_t)D + 1) * ((int64_t)H + 1) * ((int64_t)W + 1); }

// Every argument rule of crn_voxel_topology(_cpu); nothing is launched or written when this fails.  N == 0 is valid (and
// nothing is done).
inline bool vt_args_ok(const void* grid, const int64_t* st, int dtype, int N, int D, int H, int W, int num_labels, int mask,
                       const int64_t* table, const int64_t* bad) {
  if (N < 0 || D < 1 || H < 1 || W < 1) return false;
  if ((int64_t)D * H > INT32_MAX / W) return false;
  if (dtype != VT_U8 && dtype != VT_I32) return false;
  if (num_labels < 0 || num_labels > CRN_VT_MAX_LABELS || (mask && num_labels != 0)) return false;
  if (N == 0) return true;
  if (!grid || !st || !table || !bad) return false;
  for (int i = 0; i < 3; ++i)
    if (st[i] < 0) return false;
  return st[3] == 1;
}
