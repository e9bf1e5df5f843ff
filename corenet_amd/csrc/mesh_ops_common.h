// Mesh clean-up (crn_mesh_* and their host twins): what the HIP kernels of mesh_ops.hip and the twin mesh_ops_cpu.cpp
// share -- the object lookup, the float32 formulas of a smoothing step and of the normals, the cell / offset / position
// arithmetic of the clustering, its 64-bit cluster key and the hash of its table.  Contract: include/corenet_hip.h,
// corenet_amd/mesh_ops.py and DESIGN section 24.  Both builds use -ffp-contract=off: every formula below is taken as
// written, which is what makes kernel and twin agree bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/corenet_hip.h"

#if defined(__HIP__)
#define MO_HD __host__ __device__ inline
#else
#define MO_HD inline
#endif

constexpr uint64_t MO_EMPTY_KEY = ~0ull;                   // never a cluster key: the object field stops at 2^16 - 2
constexpr int32_t MO_NO_SLOT = -1;

// The object of item i (a global vertex or face id): the n with offsets[n] <= i < offsets[n + 1]; N when there is none.
// offsets is ascending with offsets[0] == 0; empty objects are skipped.
MO_HD int mo_object(const int64_t* offsets, int N, int64_t i) {
  int lo = 0, hi = N;                                      // the first n with offsets[n + 1] > i
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid + 1] > i) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// The three global vertex ids of face f, or false when the face belongs to no object or one of its ids lies outside its
// object (or outside [0, V), for offsets that do not belong to the vertex array); *nbad is the number of such ids.
MO_HD bool mo_face_ids(const int32_t* faces, int64_t f, const int64_t* voff, const int64_t* foff, int N, int64_t V, int64_t g[3],
                       int* nbad) {
  *nbad = 0;
  const int n = mo_object(foff, N, f);
  if (n >= N) { *nbad = 3; return false; }
  const int64_t base = voff[n], nv = voff[n + 1] - base;
  for (int c = 0; c < 3; ++c) {
    const int64_t id = faces[3 * f + c];
    g[c] = base + id;
    if (id < 0 || id >= nv || g[c] >= V) ++*nbad;
  }
  return *nbad == 0;
}

// One smoothing step of one component: v + f * (s / k - v), s the neighbour sum in list order.
MO_HD float mo_smooth(float v, float s, int k, float f) {
  const float m = s / (float)k;
  return v + f * (m - v);
}

// (b - a) x (c - a)
MO_HD void mo_cross(const float* a, const float* b, const float* c, float out[3]) {
  const float u0 = b[0] - a[0], u1 = b[1] - a[1], u2 = b[2] - a[2];
  const float w0 = c[0] - a[0], w1 = c[1] - a[1], w2 = c[2] - a[2];
  out[0] = (u1 * w2) - (u2 * w1);
  out[1] = (u2 * w0) - (u0 * w2);
  out[2] = (u0 * w1) - (u1 * w0);
}

// s / |s|; a zero length gives (0, 0, 0), a NaN stays one.
MO_HD void mo_normalise(const float s[3], float out[3]) {
  const float len = sqrtf((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
  for (int c = 0; c < 3; ++c) out[c] = len == 0.f ? 0.f : s[c] / len;
}

// Cell index and 20-bit offset of one coordinate; false for a non-finite coordinate or a cell outside
// [CRN_MESH_CELL_MIN, CRN_MESH_CELL_MAX].
MO_HD bool mo_cell(float v, float cell, int32_t* c, int64_t* u) {
  const float x = v / cell;
  const float fl = floorf(x);
  if (!(fl >= (float)CRN_MESH_CELL_MIN && fl <= (float)CRN_MESH_CELL_MAX)) return false;      // NaN and infinities fail here
  *c = (int32_t)fl;
  *u = (int64_t)((x - fl) * 1048576.0f);
  return true;
}

MO_HD bool mo_cells(const float* v, float cell, int32_t c[3], int64_t u[3]) {
  bool ok = true;
  for (int a = 0; a < 3; ++a) ok = mo_cell(v[a], cell, c + a, u + a) && ok;
  return ok;
}

// object n < 2^16 - 2 and three cell indices -> the cluster key
MO_HD uint64_t mo_key(int n, const int32_t c[3]) {
  return ((uint64_t)(n + 1) << 48) | ((uint64_t)(uint32_t)(c[0] - CRN_MESH_CELL_MIN) << 32) |
         ((uint64_t)(uint32_t)(c[1] - CRN_MESH_CELL_MIN) << 16) | (uint64_t)(uint32_t)(c[2] - CRN_MESH_CELL_MIN);
}

// first slot of a key in a table of 2^log2 slots (log2 >= 1)
MO_HD uint32_t mo_hash(uint64_t key, int log2) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - log2)); }

// the position of a cluster along one axis
MO_HD float mo_position(int32_t c, int64_t sum_u, int32_t count, float cell) {
  return (float)(((double)c + ((double)sum_u / (double)count) * (1.0 / 1048576.0)) * (double)cell);
}

// the smallest table the clustering of V vertices takes: a power of two >= 2 V (and >= 2)
inline int mo_table_log2(int64_t V) {
  int l = 1;
  while (((int64_t)1 << l) < 2 * V) ++l;
  return l;
}
