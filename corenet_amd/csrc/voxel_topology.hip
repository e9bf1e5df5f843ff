// Configuration histogram of voxel grids on gfx950 (corenet_amd.voxel_topology).  Contract: include/corenet_hip.h and
// DESIGN section 23; host twin: voxel_topology_cpu.cpp (identical tables and bad counts: integer adds only).
//
// Two kernels per VT_BATCH grids (blockIdx.y picks the grid), no workgroup waits for another and every loop has a fixed
// or bounded trip count:
//   * vt_kernel: a workgroup owns a brick of CRN_VT_BRICK_D x BRICK_H x CRN_VT_BRICK_W cells.  A lane owns one 16-byte
//     unit of a row (U = 4 int32 or 16 uint8 voxels; SEG = 256 / U lanes side by side cover the brick's W extent, the
//     64 / SEG groups of a wave lie below each other in H) and VT_BH cell rows.  It walks along D: the VT_BH + 1 voxel rows
//     of a plane are loaded first (one 16-byte load each where the unit lies inside the row and is aligned, element by
//     element with bounds checks otherwise), then turned into row records of two registers -- the mask of the labelled
//     voxels of the unit and of the voxel in front of it (from the lane before by a shuffle; the first lane of a group
//     loads it), and the unit's one label or "mixed" -- and the records of the plane before stay in registers.  So a voxel
//     is read once by the workgroup, and the plane and the row in front of a brick are the only voxels two workgroups read.
//   * the cells of a unit: nothing when the four masks are empty (bin 0 is derived); U times code 255 when they are
//     full; else the codes are shifted out of the four masks.  A label grid adds the same codes to the row of the one
//     label its four records agree on; only a unit that sees two or more labels reads the eight voxels of every cell
//     again (from the cache) and loops over their distinct labels.
//     The cell w = W (voxel W - 1 and the border) is counted by the lane whose unit ends at W.
//   * a lane merges equal consecutive keys of row 0, and of the label rows, into runs; a run that ends is added to the
//     u32 rows in LDS.  After one barrier the non-zero entries are added to the grid's table with 64-bit atomics.
//   * vt_finish: bin 0 of every row <- the number of cells minus the row's other bins.
#include <utility>

#include "crn_common.h"
#include "voxel_topology_common.h"

namespace {

constexpr int VT_WAVES = 4;
constexpr int VT_THREADS = VT_WAVES * 64;
constexpr int VT_BH = 8;                                   // cell rows of a lane
constexpr int VT_BD = CRN_VT_BRICK_D;

template <typename T>
struct VtGeo {
  static constexpr int U = 16 / (int)sizeof(T);            // voxels of a unit
  static constexpr int SEG = CRN_VT_BRICK_W / U;           // lanes side by side along W
  static constexpr int HG = 64 / SEG;                      // groups of a wave along H
  static constexpr int BRICK_H = VT_WAVES * HG * VT_BH;
};
static_assert(VtGeo<int32_t>::BRICK_H == CRN_VT_BRICK_H_I32 && VtGeo<uint8_t>::BRICK_H == CRN_VT_BRICK_H_U8, "the header reports the bricks");
static_assert((CRN_VT_MAX_LABELS + 1) * 256 * 4 <= 65536, "the LDS rows need no attribute");

template <typename T>
__device__ __forceinline__ int32_t vt_get(const uint32_t (&w)[4], int i) {
  if (sizeof(T) == 4) return (int32_t)w[i];
  return (int32_t)((w[i >> 2] >> (8 * (i & 3))) & 255u);
}

// The unit [w0, w0 + U) of a row of W voxels at p, element by element; voxels outside the row are 0.
template <typename T>
__device__ __forceinline__ uint4 vt_load_slow(const T* p, int w0, int W) {
  constexpr int U = VtGeo<T>::U;
  uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < U; ++i) {
    const int x = w0 + i;
    uint32_t v = 0;
    if (x >= 0 && x < W) v = sizeof(T) == 4 ? (uint32_t)p[x] : (uint32_t)p[x] & 255u;
    if (sizeof(T) == 4) w[i] = v;
    else w[i >> 2] |= v << (8 * (i & 3));
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// What a lane keeps of one voxel row: bit 0 of m is the voxel in front of the unit, bit 1 + i voxel i, set where the
// voxel carries a label; lab is the one label of those voxels, 0 without any, -1 with several (a mask grid has the one
// label 1).
struct VtRow {
  uint32_t m;
  int32_t lab;
};

__device__ __forceinline__ int32_t vt_same(int32_t a, int32_t b) { return a == 0 ? b : (b == 0 || a == b) ? a : -1; }

template <typename T, bool LABELS>
__device__ __forceinline__ VtRow vt_make(const uint32_t (&w)[4], uint32_t pv, int32_t L, bool own, uint32_t& bad) {
  constexpr int U = VtGeo<T>::U;
  bool b;
  VtRow r;
  r.lab = vt_label((int32_t)pv, L, !LABELS, &b);           // a bad voxel is counted where it is part of the unit
  r.m = r.lab != 0;
  if (w[0] | w[1] | w[2] | w[3]) {
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const int32_t v = vt_label(vt_get<T>(w, i), L, !LABELS, &b);
      if (v) { r.m |= 1u << (i + 1); r.lab = vt_same(r.lab, v); }
      if (LABELS && b && own) ++bad;
    }
  }
  return r;
}

// The counting state of a lane: the open run of row 0 and the open run of the label rows.
struct VtCount {
  uint32_t k0 = 0, n0 = 0, kl = 0, nl = 0;
  uint32_t* lds;
  __device__ __forceinline__ void add0(uint32_t key, uint32_t n) {
    if (key == k0) { n0 += n; return; }
    if (n0) atomicAdd(lds + k0, n0);
    k0 = key; n0 = n;
  }
  __device__ __forceinline__ void addl(uint32_t key, uint32_t n) {
    if (key == kl) { nl += n; return; }
    if (nl) atomicAdd(lds + kl, nl);
    kl = key; nl = n;
  }
  __device__ __forceinline__ void close() {
    if (n0) atomicAdd(lds + k0, n0);
    if (nl) atomicAdd(lds + kl, nl);
    n0 = nl = 0;
  }
};

__device__ __forceinline__ uint32_t vt_code(uint32_t m00, uint32_t m01, uint32_t m10, uint32_t m11, int i) {
  return ((m00 >> i) & 3u) << vt_row_shift(0, 0) | ((m01 >> i) & 3u) << vt_row_shift(0, 1) | ((m10 >> i) & 3u) << vt_row_shift(1, 0) |
         ((m11 >> i) & 3u) << vt_row_shift(1, 1);
}

// One grid as the kernel sees it.
template <typename T>
struct VtGrid {
  const T* g;
  int64_t sD, sH;
  int D, H, W;
  int32_t L;
  // the label of voxel (d, h, w); background outside the grid
  __device__ __forceinline__ int32_t label(int d, int h, int w) const {
    if (d < 0 || d >= D || h < 0 || h >= H || w < 0 || w >= W) return 0;
    bool b;
    return vt_label((int32_t)g[d * sD + h * sH + w], L, 0, &b);
  }
};

// A unit with several labels (rare): the eight voxels of every cell are read again, from the cache.  Cells (d, h, w0 + i).
template <typename T>
__device__ __forceinline__ void vt_mixed(const VtGrid<T>& G, int d, int h, int w0, int cells, VtCount& c) {
#pragma unroll 1
  for (int i = 0; i < cells; ++i) {                        // at most U + 1
    int32_t v[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) v[b] = G.label(d - 1 + (b >> 2), h - 1 + ((b >> 1) & 1), w0 + i - 1 + (b & 1));
    uint32_t code = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) code |= (uint32_t)(v[b] != 0) << b;
    if (!code) continue;
    c.add0(code, 1);
#pragma unroll
    for (int b = 0; b < 8; ++b) {                          // every distinct label once: at its first voxel
      bool first = v[b] != 0;
#pragma unroll
      for (int e = 0; e < b; ++e) first = first && v[e] != v[b];
      if (!first) continue;
      uint32_t lc = 0;
#pragma unroll
      for (int e = b; e < 8; ++e) lc |= (uint32_t)(v[e] == v[b]) << e;
      c.addl(((uint32_t)v[b] << 8) + lc, 1);
    }
  }
}

// The cells (d, h, w0 ..) of one unit: r[i][j] is voxel row (d - 1 + i, h - 1 + j); cell c of the unit holds the voxels c,
// c + 1 of the records.  tail: the unit ends at W and also counts the cell behind it.
template <typename T, bool LABELS>
__device__ __forceinline__ void vt_unit(const VtGrid<T>& G, int d, int h, int w0, const VtRow& r00, const VtRow& r01, const VtRow& r10,
                                        const VtRow& r11, bool tail, VtCount& c) {
  constexpr int U = VtGeo<T>::U;
  constexpr uint32_t FULL = (2u << U) - 1u;
  if ((r00.m | r01.m | r10.m | r11.m) == 0) return;
  const int32_t lab = vt_same(vt_same(r00.lab, r01.lab), vt_same(r10.lab, r11.lab));
  if (LABELS && lab < 0) {
    vt_mixed<T>(G, d, h, w0, tail ? U + 1 : U, c);
    return;
  }
  const uint32_t base = (uint32_t)lab << 8;                // one label: its row gets the codes of row 0
  if ((r00.m & r01.m & r10.m & r11.m) == FULL) {
    c.add0(255, U);
    if (LABELS) c.addl(base + 255, U);
  } else {
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const uint32_t code = vt_code(r00.m, r01.m, r10.m, r11.m, i);
      if (code) {
        c.add0(code, 1);
        if (LABELS) c.addl(base + code, 1);
      }
    }
  }
  if (tail) {
    const uint32_t code = vt_code(r00.m, r01.m, r10.m, r11.m, U);
    if (code) {
      c.add0(code, 1);
      if (LABELS) c.addl(base + code, 1);
    }
  }
}

// The walk of one lane along D.  The steps over the VT_BH + 1 voxel rows of a plane are member templates expanded over an
// index sequence, so every index into the register arrays is a constant.
template <typename T, bool LABELS>
struct VtLane {
  static constexpr int U = VtGeo<T>::U;
  VtGrid<T> G;
  int w0, h0, ul;                                          // first voxel of the unit, first cell row, place in the W group
  bool inside, front, tail;
  VtRow prev[VT_BH + 1], last;                             // voxel rows h0 - 1 .. h0 + VT_BH - 1 of the plane before; row j - 1 of this one
  uint32_t raw[VT_BH + 1][4], pv[VT_BH + 1];

  template <int J>
  __device__ __forceinline__ void load(int dd) {
    const int h = h0 - 1 + J;
    raw[J][0] = raw[J][1] = raw[J][2] = raw[J][3] = 0;
    pv[J] = 0;
    if (dd < 0 || dd >= G.D || h < 0 || h >= G.H) return;
    const T* p = G.g + dd * G.sD + h * G.sH;
    uint4 q;
    if (inside && ((uintptr_t)(p + w0) & 15) == 0) q = *reinterpret_cast<const uint4*>(p + w0);
    else q = vt_load_slow<T>(p, w0, G.W);
    raw[J][0] = q.x; raw[J][1] = q.y; raw[J][2] = q.z; raw[J][3] = q.w;
    if (ul == 0 && front) pv[J] = sizeof(T) == 4 ? (uint32_t)p[w0 - 1] : (uint32_t)p[w0 - 1] & 255u;
  }

  template <int J>
  __device__ __forceinline__ void step(int dd, bool proc, VtCount& c, uint32_t& nbad) {
    const uint32_t up = (uint32_t)__shfl_up((int)vt_get<T>(raw[J], U - 1), 1, 64);
    if (ul != 0) pv[J] = front ? up : 0u;
    const VtRow cur = vt_make<T, LABELS>(raw[J], pv[J], G.L, proc && J >= 1, nbad);
    if constexpr (J >= 1) {
      if (proc) vt_unit<T, LABELS>(G, dd, h0 - 1 + J, w0, prev[J - 1], prev[J], last, cur, tail, c);
      prev[J - 1] = last;
    }
    last = cur;
  }

  template <int... J>
  __device__ __forceinline__ void plane(int dd, bool proc, VtCount& c, uint32_t& nbad, std::integer_sequence<int, J...>) {
    (load<J>(dd), ...);                                    // all loads of the plane first
    (step<J>(dd, proc, c, nbad), ...);
    prev[VT_BH] = last;
  }

  __device__ __forceinline__ void run(int d0, int d1, VtCount& c, uint32_t& nbad) {
#pragma unroll
    for (int j = 0; j <= VT_BH; ++j) { prev[j].m = 0; prev[j].lab = 0; }
    last.m = 0; last.lab = 0;
#pragma unroll 1
    for (int dd = d0 - 1; dd < d1; ++dd)                   // at most CRN_VT_BRICK_D + 1 planes
      plane(dd, dd >= d0, c, nbad, std::make_integer_sequence<int, VT_BH + 1>());
  }
};

__device__ __forceinline__ uint32_t vt_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// LABELS == false counts a mask grid (value != 0, L == 0, nothing is bad).
template <typename T, bool LABELS>
__global__ __launch_bounds__(VT_THREADS) void vt_kernel(const T* __restrict__ grid, int64_t sN, int64_t sD, int64_t sH, int D, int H, int W,
                                                        int32_t L, int segs, int hbricks, int64_t* table, int64_t* bad) {
  using G = VtGeo<T>;
  constexpr int U = G::U;
  extern __shared__ __attribute__((aligned(16))) uint32_t vt_lds[];
  const int entries = (L + 1) * 256;
  for (int i = threadIdx.x; i < entries; i += VT_THREADS) vt_lds[i] = 0;
  __syncthreads();                                         // every thread of the workgroup arrives: no return above
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ul = lane % G::SEG, hg = lane / G::SEG;
  const int n = blockIdx.y;
  const T* g = grid + n * sN;
  const int a = (int)(((uintptr_t)g / sizeof(T)) % U);     // units start where row (0, 0) of the grid is 16-byte aligned
  uint32_t bx = blockIdx.x;
  const int seg = (int)(bx % (uint32_t)segs); bx /= (uint32_t)segs;
  const int hb = (int)(bx % (uint32_t)hbricks), db = (int)(bx / (uint32_t)hbricks);
  const int64_t w0l = ((int64_t)seg * G::SEG + ul) * U - a;
  const int64_t h0l = (int64_t)hb * G::BRICK_H + (wave * G::HG + hg) * VT_BH;
  const int d0 = db * VT_BD;
  const int d1 = d0 + VT_BD < D + 1 ? d0 + VT_BD : D + 1;  // the brick's cell planes are d0 .. d1 - 1
  VtCount c;
  c.lds = vt_lds;
  uint32_t nbad = 0;
  if (w0l < W && h0l <= H) {                               // else the lane has no cell; the lane before an active one is active
    const int w0 = (int)w0l, h0 = (int)h0l;
    const bool inside = w0 >= 0 && w0 + U <= W;
    const bool front = w0 >= 1 && w0 < W;                  // the voxel in front of the unit exists and the unit has cells of its own
    const bool tail = w0 + U == W;
    VtLane<T, LABELS> ln;
    ln.G = VtGrid<T>{g, sD, sH, D, H, W, L};
    ln.w0 = w0; ln.h0 = h0; ln.ul = ul; ln.inside = inside; ln.front = front; ln.tail = tail;
    ln.run(d0, d1, c, nbad);
    c.close();
  }
  nbad = vt_wave_sum(nbad);
  if (lane == 0 && nbad) atomicAdd(reinterpret_cast<unsigned long long*>(bad + n), (unsigned long long)nbad);
  __syncthreads();
  unsigned long long* tab = reinterpret_cast<unsigned long long*>(table + (int64_t)n * entries);
  for (int i = threadIdx.x; i < entries; i += VT_THREADS) {
    const uint32_t k = vt_lds[i];
    if (k && (i & 255)) atomicAdd(tab + i, (unsigned long long)k);
  }
}

// Bin 0 of row blockIdx.x <- cells minus the row's other bins.  One workgroup of 256 threads per row.
__global__ __launch_bounds__(256) void vt_finish(int64_t* table, int64_t cells) {
  __shared__ int64_t part[4];
  int64_t* row = table + (int64_t)blockIdx.x * 256;
  int64_t v = threadIdx.x ? row[threadIdx.x] : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) row[0] = cells - (part[0] + part[1] + part[2] + part[3]);
}

template <typename T, bool LABELS>
int vt_launch(const void* grid, const int64_t* st, int nb, int D, int H, int W, int L, int64_t* table, int64_t* bad, hipStream_t s) {
  using G = VtGeo<T>;
  // a grid's units start up to U - 1 voxels in front of its rows (the kernel's `a`); the same for all grids when N stride keeps alignment
  const int shift = (nb == 1 || st[0] % G::U == 0) ? (int)(((uintptr_t)grid / sizeof(T)) % G::U) : G::U - 1;
  const int segs = (int)(((int64_t)W + shift + CRN_VT_BRICK_W - 1) / CRN_VT_BRICK_W);
  const int hbricks = (int)(((int64_t)H + 1 + G::BRICK_H - 1) / G::BRICK_H);
  const int dbricks = (int)(((int64_t)D + 1 + VT_BD - 1) / VT_BD);
  const int64_t bricks = (int64_t)segs * hbricks * dbricks;
  if (bricks > INT32_MAX) return CRN_EINVAL;               // unreachable for D*H*W <= 2^31 - 1; kept as the launch's own check
  const dim3 g((unsigned)bricks, (unsigned)nb), blk(VT_THREADS);
  return crn_launch(vt_kernel<T, LABELS>, g, blk, (size_t)(L + 1) * 1024, s, (const T*)grid, st[0], st[1], st[2], D, H, W, (int32_t)L, segs,
                    hbricks, table, bad);
}

}  // namespace

extern "C" int crn_voxel_topology_tiles(int32_t* out6) {
  if (!out6) return CRN_EINVAL;
  out6[0] = CRN_VT_BRICK_D; out6[1] = CRN_VT_BRICK_H_I32; out6[2] = CRN_VT_BRICK_H_U8; out6[3] = CRN_VT_BRICK_W;
  out6[4] = CRN_VT_MAX_LABELS; out6[5] = CRN_VT_BATCH;
  return CRN_OK;
}

extern "C" int crn_voxel_topology(const void* grid, const int64_t* strides, int dtype, int N, int D, int H, int W, int num_labels,
                                  int mask, int64_t* table, int64_t* bad, crnStream stream) {
  if (!vt_args_ok(grid, strides, dtype, N, D, H, W, num_labels, mask, table, bad)) return CRN_EINVAL;
  if (N == 0) return CRN_OK;
  CRN_ENTRY(stream);
  hipStream_t st = (hipStream_t)stream;
  const int64_t entries = ((int64_t)num_labels + 1) * 256;
  CRN_HIP(hipMemsetAsync(table, 0, (size_t)N * entries * 8, st));
  CRN_HIP(hipMemsetAsync(bad, 0, (size_t)N * 8, st));
  const size_t es = dtype == VT_U8 ? 1 : 4;
  const int64_t cells = vt_cells(D, H, W);
  for (int n0 = 0; n0 < N; n0 += CRN_VT_BATCH) {
    const int nb = N - n0 < CRN_VT_BATCH ? N - n0 : CRN_VT_BATCH;
    const void* g = (const char*)grid + (size_t)n0 * strides[0] * es;
    int64_t* tab = table + n0 * entries;
    int rc;
    if (dtype == VT_U8)
      rc = mask ? vt_launch<uint8_t, false>(g, strides, nb, D, H, W, num_labels, tab, bad + n0, st)
                : vt_launch<uint8_t, true>(g, strides, nb, D, H, W, num_labels, tab, bad + n0, st);
    else
      rc = mask ? vt_launch<int32_t, false>(g, strides, nb, D, H, W, num_labels, tab, bad + n0, st)
                : vt_launch<int32_t, true>(g, strides, nb, D, H, W, num_labels, tab, bad + n0, st);
    if (rc != CRN_OK) return rc;
    rc = crn_launch(vt_finish, dim3((unsigned)(nb * (num_labels + 1))), dim3(256), 0, st, tab, cells);
    if (rc != CRN_OK) return rc;
  }
  return CRN_OK;
}
