// Marching cubes: the per-sample arithmetic shared by the HIP kernels (marching_cubes.hip) and the host twin
// (marching_cubes_cpu.cpp).  Both include this header, so a vertex, a normal and a transform are the same float32
// operations in the same order on either side (both are compiled with -ffp-contract=off).
//
// Index space: the PADDED grid of one object, (D + 2) x (H + 2) x (W + 2) points, sample grid[n, d, h, w] at padded
// (z, y, x) = (d + 1, h + 1, w + 1), zeros on the one-voxel border.  Cells: (D + 1) x (H + 1) x (W + 1), cell (z, y, x)
// has corners (z + dz, y + dy, x + dx), corner id c = dx + 2 dy + 4 dz.  Edge ids: see tools/gen_mc_tables.py.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__)
#define CRN_MC_HD __host__ __device__ inline
#else
#define CRN_MC_HD inline
#endif

struct crnMcGrid {
  const float* p;          // grid[n][d][h][w], W stride 1
  int64_t sN, sD, sH;      // element strides
  int D, H, W;
  float level;
};

// padded sample (zero outside the grid; NaN reads as 0, i.e. outside since level > 0)
CRN_MC_HD float mc_at(const crnMcGrid& g, const float* obj, int z, int y, int x) {
  if (z < 1 || z > g.D || y < 1 || y > g.H || x < 1 || x > g.W) return 0.f;
  const float v = obj[(int64_t)(z - 1) * g.sD + (int64_t)(y - 1) * g.sH + (x - 1)];
  return v == v ? v : 0.f;
}

CRN_MC_HD int mc_inside(float v, float level) { return v > level ? 1 : 0; }

// edge e -> axis and the offsets (dx, dy, dz) of its lower corner in the cell
CRN_MC_HD void mc_edge(int e, int& a, int& dx, int& dy, int& dz) {
  a = e >> 2;
  const int k = e & 3;
  int off[3] = {0, 0, 0};
  off[a == 0 ? 1 : 0] = k & 1;
  off[a == 2 ? 1 : 2] = k >> 1;
  dx = off[0]; dy = off[1]; dz = off[2];
}

// does the edge from padded point (z, y, x) along axis a straddle the level?
CRN_MC_HD int mc_crosses(const crnMcGrid& g, const float* obj, int z, int y, int x, int a) {
  return mc_inside(mc_at(g, obj, z, y, x), g.level) ^
         mc_inside(mc_at(g, obj, z + (a == 2), y + (a == 1), x + (a == 0)), g.level);
}

// bits 0/1/2: the x / y / z edge owned by padded point (z, y, x) crosses
CRN_MC_HD int mc_owned_bits(const crnMcGrid& g, const float* obj, int z, int y, int x) {
  const int i0 = mc_inside(mc_at(g, obj, z, y, x), g.level);
  return (i0 ^ mc_inside(mc_at(g, obj, z, y, x + 1), g.level)) | ((i0 ^ mc_inside(mc_at(g, obj, z, y + 1, x), g.level)) << 1) |
         ((i0 ^ mc_inside(mc_at(g, obj, z + 1, y, x), g.level)) << 2);
}

// owned bits of the cell's own corner 0 from its case
CRN_MC_HD int mc_case_owned_bits(int cs) {
  const int i0 = cs & 1;
  return (i0 ^ ((cs >> 1) & 1)) | ((i0 ^ ((cs >> 2) & 1)) << 1) | ((i0 ^ ((cs >> 4) & 1)) << 2);
}

CRN_MC_HD int mc_popc3(int b) { return (b & 1) + ((b >> 1) & 1) + ((b >> 2) & 1); }

// gradient component along axis c of the padded grid at a point: central difference inside, one-sided on the border
CRN_MC_HD float mc_grad(const crnMcGrid& g, const float* obj, int z, int y, int x, int c) {
  const int dx = c == 0, dy = c == 1, dz = c == 2;
  const int p = c == 0 ? x : (c == 1 ? y : z);
  const int e = (c == 0 ? g.W : (c == 1 ? g.H : g.D)) + 1;       // last padded index
  if (p == 0) return mc_at(g, obj, z + dz, y + dy, x + dx) - mc_at(g, obj, z, y, x);
  if (p == e) return mc_at(g, obj, z, y, x) - mc_at(g, obj, z - dz, y - dy, x - dx);
  return (mc_at(g, obj, z + dz, y + dy, x + dx) - mc_at(g, obj, z - dz, y - dy, x - dx)) * 0.5f;
}

// Vertex of the crossing edge from padded point (z, y, x) along axis a: position (x, y, z order) and unit normal.
// f0 is the sample at the lower end, f1 at the upper; t = (level - f0) / (f1 - f0), coordinate = float(i0) + t.
CRN_MC_HD void mc_vertex(const crnMcGrid& g, const float* obj, int z, int y, int x, int a, float pos[3], float nrm[3]) {
  const int dx = a == 0, dy = a == 1, dz = a == 2;
  const float f0 = mc_at(g, obj, z, y, x), f1 = mc_at(g, obj, z + dz, y + dy, x + dx);
  const float t = (g.level - f0) / (f1 - f0);
  pos[0] = (float)x; pos[1] = (float)y; pos[2] = (float)z;
  pos[a] = pos[a] + t;
  float n[3];
  for (int c = 0; c < 3; ++c) {
    const float g0 = mc_grad(g, obj, z, y, x, c), g1 = mc_grad(g, obj, z + dz, y + dy, x + dx, c);
    n[c] = -(g0 + t * (g1 - g0));
  }
  const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
  for (int c = 0; c < 3; ++c) nrm[c] = len > 0.f ? n[c] / len : 0.f;
}

// m: row-major 4x4.  Positions as points (w = 1, homogeneous divide), normals as vectors (w = 0, not renormalised).
CRN_MC_HD void mc_transform(const float* m, float pos[3], float nrm[3]) {
  float h[4], v[3];
  for (int r = 0; r < 4; ++r) h[r] = ((m[4 * r] * pos[0] + m[4 * r + 1] * pos[1]) + m[4 * r + 2] * pos[2]) + m[4 * r + 3];
  for (int r = 0; r < 3; ++r) v[r] = (m[4 * r] * nrm[0] + m[4 * r + 1] * nrm[1]) + m[4 * r + 2] * nrm[2];
  for (int r = 0; r < 3; ++r) { pos[r] = h[r] / h[3]; nrm[r] = v[r]; }
}

// box filter along one axis of a contiguous [N][D][H][W] output: out = scale * sum_{j < k} in[i - lo + j] (zero outside),
// j ascending from 0.f -- the same order in the kernel and the host twin
CRN_MC_HD float mc_box_tap(const float* in, int64_t base, int64_t stride, int i, int extent, int k, float scale) {
  const int lo = (k - 1) / 2;
  float s = 0.f;
  for (int j = 0; j < k; ++j) {
    const int q = i - lo + j;
    if (q >= 0 && q < extent) s += in[base + (int64_t)q * stride];
  }
  return s * scale;
}
