// Label overlaps of two voxel grids (crn_voxel_overlap and its host twin): what the HIP kernel and the twin share -- the
// key of a voxel, the rows a pair of strided grids is read in and the argument checks.  Contract: include/corenet_hip.h,
// corenet_amd/voxel_overlap.py and DESIGN section 20.
#pragma once
#include <stdint.h>

#include "../../include/corenet_hip.h"

#if defined(__HIP__)
#define VO_HD __host__ __device__ inline
#else
#define VO_HD inline
#endif

// dtype codes of the grids (those of crn_voxel_components)
constexpr int VO_U8 = 1, VO_I32 = 2;
constexpr uint32_t VO_BAD = 0xffffffffu;         // the key of a voxel with a label outside its grid's range

// The table entry of a voxel: a * (nb + 1) + b, or VO_BAD.  na, nb >= 0 and (na + 1) * (nb + 1) <= 2^31 - 1 (the caller
// checked), so the key fits 32 bits; key 0 is (background, background).
VO_HD uint32_t vo_key(int32_t a, int32_t b, int32_t na, int32_t nb) {
  return ((uint32_t)a <= (uint32_t)na && (uint32_t)b <= (uint32_t)nb) ? (uint32_t)a * ((uint32_t)nb + 1u) + (uint32_t)b : VO_BAD;
}

// The voxels of one grid pair as R1 * R2 rows of L voxels that are contiguous in both a and b: row r starts at element
// (r / R2) * s1 + (r % R2) * s2 of each grid.  H is merged into the row where both grids have H stride W, and D too where
// both then have D stride H * W: two contiguous grids are a single row of D * H * W voxels.
struct VoRows {
  int R2, L;
  int64_t rows;                // R1 * R2
  int64_t a1, a2, b1, b2;      // strides of a and b, in elements
};

inline VoRows vo_rows(const int64_t* sa, const int64_t* sb, int D, int H, int W) {
  VoRows r;
  if (H == 1 || (sa[2] == W && sb[2] == W)) {
    const int64_t L = (int64_t)H * W;
    r.R2 = 1; r.a2 = 0; r.b2 = 0; r.a1 = sa[1]; r.b1 = sb[1];
    if (D == 1 || (sa[1] == L && sb[1] == L)) { r.L = (int)(L * D); r.rows = 1; }
    else { r.L = (int)L; r.rows = D; }
  } else {
    r.R2 = H; r.L = W; r.rows = (int64_t)D * H;
    r.a1 = sa[1]; r.a2 = sa[2]; r.b1 = sb[1]; r.b2 = sb[2];
  }
  return r;
}

// (na + 1) * (nb + 1) if both are in range and the product is `entries`, else -1: the grid is then counted as bad.
VO_HD int64_t vo_entries_ok(int64_t na, int64_t nb, int64_t entries) {
  if (na < 0 || nb < 0 || na >= INT32_MAX || nb >= INT32_MAX) return -1;
  if (entries < 1 || entries > INT32_MAX || (na + 1) > entries / (nb + 1)) return -1;
  return (na + 1) * (nb + 1) == entries ? entries : -1;
}

inline bool vo_offsets_ok(int N, const int64_t* off) {
  if (N < 0 || (N > 0 && (!off || off[0] != 0))) return false;
  for (int n = 0; n < N; ++n)
    if (off[n + 1] < off[n] || off[n + 1] - off[n] > INT32_MAX || off[n + 1] > INT64_MAX / 8) return false;
  return true;
}

// Every argument rule of crn_voxel_overlap(_cpu); nothing is launched or written when this fails.  N == 0 is valid (and
// nothing is done).
inline bool vo_args_ok(const void* a, const int64_t* sa, int dta, const void* b, const int64_t* sb, int dtb, int N, int D, int H,
                       int W, const int64_t* num_a, const int64_t* num_b, const int64_t* off, const int64_t* table,
                       const int64_t* bad) {
  if (N < 0 || D < 1 || H < 1 || W < 1) return false;
  if ((int64_t)D * H > INT32_MAX / W) return false;
  if ((dta != VO_U8 && dta != VO_I32) || (dtb != VO_U8 && dtb != VO_I32)) return false;
  if (N == 0) return true;
  if (!a || !b || !sa || !sb || !num_a || !num_b || !bad || !vo_offsets_ok(N, off)) return false;
  if (off[N] > 0 && !table) return false;
  for (int i = 0; i < 3; ++i)
    if (sa[i] < 0 || sb[i] < 0) return false;
  return sa[3] == 1 && sb[3] == 1;
}
