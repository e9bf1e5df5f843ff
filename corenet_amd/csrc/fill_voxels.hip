// fill_inside_voxels: flood fill of the empty region connected to the
// x==0 / y==0 / z==0 faces; everything else becomes 1.
// Reference: cc/fill_voxels_gpu.cu:96-171 (lock-free union-find, 2 kernels,
// 16 B/voxel parent array), cc/fill_voxels_cpu.cc:74-183.  Semantics kept
// bit-exact: 6-connectivity, the virtual background node touches
// only the LOW faces, output strictly {0,1}.
//
// MI355X design: not a union-find.  The grid is bit-packed (1 bit/voxel: a
// 128^3 grid is 256 KiB), so a z-slab of the "empty" and "reached" bitmaps lives
// entirely in the 160 KiB LDS of one CU.  Propagation along x is word-parallel
// carry arithmetic (64 voxels per add), along y/z it is a bitwise AND/OR of
// neighbouring rows.  Slabs exchange halo planes through HBM between rounds;
// the propagation is a monotone closure, so any interleaving converges to the
// same fixed point = the reference's connected-component answer.
// HBM traffic: read grid once, write result once (+ 2 bits/voxel of bitmaps).
#include "crn_common.h"
#include <cstring>
#include <algorithm>
#include <mutex>
#include <vector>

namespace {

typedef unsigned long long u64;

// Element strides of a [N][D][H][W] tensor (crn_fill_voxels_strided: the reference op takes packed accessors with
// strides, fill_voxels_gpu.cu:146-163).  SV = false instantiations never read it (contiguous grids, 16-byte paths).
struct FillView { long long sN, sD, sH, sW; };
template <bool SV> __device__ __forceinline__ long long fv_grid(const FillView& v, long long n, long long DHW) {
  return SV ? n * v.sN : n * DHW;
}
// element offset of (row = z*H + y, x) inside a grid
template <bool SV> __device__ __forceinline__ long long fv_at(const FillView& v, long long row, int x, int H, int W) {
  if (SV) { const long long z = row / H, y = row - z * H; return z * v.sD + y * v.sH + (long long)x * v.sW; }
  return row * W + x;
}

template <typename T>
__global__ __launch_bounds__(256) void fill_pack_kernel(const T* grid, u64* E, u64* R, int D, int H, int W,
                                                        int WX, int64_t nwords) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t wi = wave0; wi < nwords; wi += nwaves) {
    const int k = (int)(wi % WX);
    const int64_t row = wi / WX;              // (n*D + z)*H + y
    const int y = (int)(row % H);
    const int z = (int)((row / H) % D);
    const int x = k * 64 + lane;
    bool empty = false;
    if (x < W) empty = !(grid[row * W + x] > (T)0);
    const u64 e = __ballot(empty);
    if (lane == 0) {
      E[wi] = e;
      R[wi] = (y == 0 || z == 0) ? e : (k == 0 ? (e & 1ull) : 0ull);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void fill_unpack_kernel(const u64* E, const u64* R, T* out, int W, int WX,
                                                          int64_t nwords) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t wi = wave0; wi < nwords; wi += nwaves) {
    const int k = (int)(wi % WX);
    const int64_t row = wi / WX;
    const int x = k * 64 + lane;
    const u64 outside = E[wi] & R[wi];
    if (x < W) out[row * W + x] = ((outside >> lane) & 1ull) ? (T)0 : (T)1;
  }
}

// bits of r (subset of e) spread towards higher bit positions through runs of 1s in e
__device__ __forceinline__ u64 fill_up(u64 e, u64 r) { return (((e + r) ^ e) & e) | r; }

// Grids of ANY size (the reference op has no size limit, fill_voxels_gpu.cu:136-171): rows wider than 512 voxels, or
// planes whose bitmaps do not fit the LDS budget of the kernels below.  One workgroup per grid, bitmaps in the global
// workspace (words of 64 voxels, WX words per row, WX unbounded): pack, then relax rows in place -- neighbours in y / z
// are ORed in, the closure along x is the same carry arithmetic, a forward and a backward pass over the row's words --
// until a whole sweep changes nothing, then unpack.  Every update only sets bits (monotone closure), words are written
// with single 8-byte stores, and the workgroup barrier between sweeps orders them: any interleaving inside a sweep
// reads valid lower bounds and the fixed point is the reference's connected components.  No host round trip.
template <typename T, bool SV>
__global__ __launch_bounds__(1024) void fill_global_kernel(const T* grid, T* out, u64* E, u64* R, int D, int H, int W, int WX,
                                                          FillView vi, FillView vo) {
  const int n = blockIdx.x;
  const int64_t rows = (int64_t)D * H, nw = rows * WX;
  const T* g = grid + fv_grid<SV>(vi, n, rows * W);
  T* o = out + fv_grid<SV>(vo, n, rows * W);
  u64* e = E + (int64_t)n * nw;
  u64* r = R + (int64_t)n * nw;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  for (int64_t wi = wave; wi < nw; wi += nwaves) {             // pack: one wave per word
    const int k = (int)(wi % WX);
    const int64_t row = wi / WX;
    const int y = (int)(row % H), z = (int)(row / H);
    const int x = k * 64 + lane;
    const bool empty = x < W && !(g[fv_at<SV>(vi, row, x, H, W)] > (T)0);
    const u64 eb = __ballot(empty);
    if (lane == 0) { e[wi] = eb; r[wi] = (y == 0 || z == 0) ? eb : (k == 0 ? (eb & 1ull) : 0ull); }
  }
  __syncthreads();
  for (int sweep = 0; sweep < (1 << 24); ++sweep) {
    int changed = 0;
    for (int64_t row = threadIdx.x; row < rows; row += blockDim.x) {
      const int y = (int)(row % H), z = (int)(row / H);
      u64* rr = r + row * WX;
      const u64* er = e + row * WX;
      u64 carry = 0;
      for (int k = 0; k < WX; ++k) {                           // neighbours + closure towards +x
        const u64 ek = er[k], old = rr[k];
        u64 nb = carry & 1ull;
        if (y > 0) nb |= rr[k - WX];
        if (y + 1 < H) nb |= rr[k + WX];
        if (z > 0) nb |= rr[k - (int64_t)H * WX];
        if (z + 1 < D) nb |= rr[k + (int64_t)H * WX];
        u64 v = fill_up(ek, old | (nb & ek));
        carry = v >> 63;
        if (v != old) { rr[k] = v; changed = 1; }
      }
      carry = 0;
      for (int k = WX - 1; k >= 0; --k) {                      // closure towards -x
        const u64 eb = __brevll(er[k]), old = rr[k];
        u64 v = fill_up(eb, __brevll(old) | (carry & eb & 1ull));
        carry = v >> 63;
        v = __brevll(v);
        if (v != old) { rr[k] = v; changed = 1; }
      }
    }
    if (!__syncthreads_or(changed)) break;
  }
  for (int64_t wi = wave; wi < nw; wi += nwaves) {             // unpack
    const int k = (int)(wi % WX);
    const int64_t row = wi / WX;
    const int x = k * 64 + lane;
    const u64 outside = e[wi] & r[wi];
    if (x < W) o[fv_at<SV>(vo, row, x, H, W)] = ((outside >> lane) & 1ull) ? (T)0 : (T)1;
  }
}

template <int WX>
__device__ __forceinline__ bool relax_row(const u64* e, u64* r) {
  // r |= x-closure of r inside e, both directions, with carries across the row's words
  bool changed = false;
  u64 carry = 0;
#pragma unroll
  for (int k = 0; k < WX; ++k) {
    u64 v = r[k] | (carry & e[k] & 1ull);
    v = fill_up(e[k], v);
    carry = v >> 63;
    if (v != r[k]) { r[k] = v; changed = true; }
  }
  carry = 0;
#pragma unroll
  for (int k = WX - 1; k >= 0; --k) {
    const u64 eb = __brevll(e[k]);
    u64 v = __brevll(r[k]) | (carry & eb & 1ull);
    v = fill_up(eb, v);
    carry = v >> 63;
    v = __brevll(v);
    if (v != r[k]) { r[k] = v; changed = true; }
  }
  return changed;
}

constexpr int STRIP = 8;

// Relaxes one slab held in LDS to its local fixed point.  El [nz][H][WX], Rl [nz+2][H][WX] with halo
// planes 0 and nz+1.  Returns (block-uniform) whether anything changed.
template <int WX>
__device__ int relax_slab(const u64* El, u64* Rl, int nz, int H) {
  const int rowsz = H * WX;
  const int nstrips = (H + STRIP - 1) / STRIP;
  const int units = nz * nstrips;
  int any = 0;
  for (int iter = 0; iter < 100000; ++iter) {
    int changed = 0;
    for (int u = threadIdx.x; u < units; u += blockDim.x) {
      const int p = u / nstrips, y0 = (u % nstrips) * STRIP, y1 = min(H, y0 + STRIP);
      const u64* el = El + (size_t)p * rowsz;
      u64* rc = Rl + (size_t)(p + 1) * rowsz;
      const u64* rlo = Rl + (size_t)p * rowsz;
      const u64* rhi = Rl + (size_t)(p + 2) * rowsz;
      u64 prev[WX], e[WX], r[WX];
      // +y sweep
#pragma unroll
      for (int k = 0; k < WX; ++k) prev[k] = y0 > 0 ? rc[(y0 - 1) * WX + k] : 0ull;
      for (int y = y0; y < y1; ++y) {
        bool ch = false;
#pragma unroll
        for (int k = 0; k < WX; ++k) {
          e[k] = el[y * WX + k];
          const u64 old = rc[y * WX + k];
          const u64 nb = prev[k] | rlo[y * WX + k] | rhi[y * WX + k] | (y + 1 < H ? rc[(y + 1) * WX + k] : 0ull);
          r[k] = old | (nb & e[k]);
          ch |= (r[k] != old);
        }
        ch |= relax_row<WX>(e, r);
        if (ch) {
#pragma unroll
          for (int k = 0; k < WX; ++k) rc[y * WX + k] = r[k];
          changed = 1;
        }
#pragma unroll
        for (int k = 0; k < WX; ++k) prev[k] = r[k];
      }
      // -y sweep
#pragma unroll
      for (int k = 0; k < WX; ++k) prev[k] = y1 < H ? rc[y1 * WX + k] : 0ull;
      for (int y = y1 - 1; y >= y0; --y) {
        bool ch = false;
#pragma unroll
        for (int k = 0; k < WX; ++k) {
          e[k] = el[y * WX + k];
          const u64 old = rc[y * WX + k];
          const u64 nb = prev[k] | rlo[y * WX + k] | rhi[y * WX + k] | (y > 0 ? rc[(y - 1) * WX + k] : 0ull);
          r[k] = old | (nb & e[k]);
          ch |= (r[k] != old);
        }
        ch |= relax_row<WX>(e, r);
        if (ch) {
#pragma unroll
          for (int k = 0; k < WX; ++k) rc[y * WX + k] = r[k];
          changed = 1;
        }
#pragma unroll
        for (int k = 0; k < WX; ++k) prev[k] = r[k];
      }
    }
    if (!__syncthreads_or(changed)) break;
    any = 1;
  }
  return any;
}

// Control block of one grid for the single-launch kernel (fill_fused_kernel): one word per exchange round -- arrivals
// in the low 16 bits, "my slab changed" votes in the high 16 -- and one departure counter per round.  The block is
// all zeros between calls: the last slab to LEAVE a round clears that round's two words (everybody else has read the
// final value by then), so no memset precedes a call; after a failed launch the rescue kernel clears the blocks
// (and the status words behind them).  The blocks live in a buffer owned by the library (zeroed once, when it is
// allocated), keyed by the caller's workspace pointer -- the caller's workspace may hold anything.
constexpr int kFusedIters = 64;
struct FusedCtl { unsigned word[kFusedIters]; unsigned depart[kFusedIters]; unsigned exits, raised, pad[2]; };   // per grid
// exits / raised: used in the block of a launch's FIRST grid -- workgroups that have left the launch, and "a workgroup
// gave up" (a partner never arrived, or the round limit): the last workgroup out then redoes the launch's grids itself.

// ---- device-side rescue path ---------------------------------------------------------------------
// Runs inside the single-launch kernel when one of its workgroups gave up (a partner workgroup was not resident within
// the spin bound, or more slab exchanges were needed than the round limit) -- see the end of fill_fused_kernel -- and
// as a kernel of its own for tests (CRN_FILL_RESCUE=1).
// One grid, one workgroup (any size): pack -> sweep the slabs of the grid through LDS until a whole pass changes
// nothing -> unpack.  sm: (2 * zs + 2) planes of LDS.
template <typename T, int WX, bool SV>
__device__ void rescue_grid(const T* gsrc, T* gdst, u64* Eg, u64* Rg, int D, int H, int W, int zs, int nslabs, u64* sm,
                            const FillView& vi, const FillView& vo) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int rowsz = H * WX;
  const int64_t gwords = (int64_t)D * rowsz;
  for (int64_t wi = wave; wi < gwords; wi += nwaves) {          // fill_pack_kernel for this grid
    const int k = (int)(wi % WX);
    const int64_t row = wi / WX;                                // z*H + y
    const int y = (int)(row % H), z = (int)(row / H);
    const int x = k * 64 + lane;
    bool empty = false;
    if (x < W) empty = !(gsrc[fv_at<SV>(vi, row, x, H, W)] > (T)0);
    const u64 e = __ballot(empty);
    if (lane == 0) {
      Eg[wi] = e;
      Rg[wi] = (y == 0 || z == 0) ? e : (k == 0 ? (e & 1ull) : 0ull);
    }
  }
  __threadfence_block();
  __syncthreads();
  u64* El = sm;                          // [zs][H][WX]
  u64* Rl = sm + (size_t)zs * rowsz;     // [zs+2][H][WX]
  for (int round = 0; round < (1 << 20); ++round) {
    int pass_changed = 0;
    for (int slab = 0; slab < nslabs; ++slab) {
      const int z0 = slab * zs, nz = min(zs, D - z0);
      const u64* Es = Eg + (int64_t)z0 * rowsz;
      u64* Rs = Rg + (int64_t)z0 * rowsz;
      for (int i = threadIdx.x; i < nz * rowsz; i += blockDim.x) { El[i] = Es[i]; Rl[rowsz + i] = Rs[i]; }
      for (int i = threadIdx.x; i < rowsz; i += blockDim.x) {
        Rl[i] = z0 > 0 ? Rs[i - rowsz] : 0ull;
        Rl[(nz + 1) * rowsz + i] = (z0 + nz < D) ? Rs[nz * rowsz + i] : 0ull;
      }
      __syncthreads();
      const int any = relax_slab<WX>(El, Rl, nz, H);
      if (any) {
        for (int i = threadIdx.x; i < nz * rowsz; i += blockDim.x) Rs[i] = Rl[rowsz + i];
        pass_changed = 1;
      }
      __threadfence_block();
      __syncthreads();
    }
    if (!pass_changed || nslabs == 1) break;
  }
  for (int64_t wi = wave; wi < gwords; wi += nwaves) {          // fill_unpack_kernel for this grid
    const int k = (int)(wi % WX);
    const int64_t row = wi / WX;
    const int x = k * 64 + lane;
    const u64 outside = Eg[wi] & Rg[wi];
    if (x < W) gdst[fv_at<SV>(vo, row, x, H, W)] = ((outside >> lane) & 1ull) ? (T)0 : (T)1;
  }
  __syncthreads();
}

template <typename T, int WX, bool SV>
__global__ __launch_bounds__(512) void fill_rescue_kernel(const T* grid, T* out, u64* E, u64* R, int D, int H, int W,
                                                          int zs, int nslabs, FillView vi, FillView vo) {
  extern __shared__ __attribute__((aligned(16))) u64 sm[];
  const int n = blockIdx.x;
  const int64_t gwords = (int64_t)D * H * WX;
  rescue_grid<T, WX, SV>(grid + fv_grid<SV>(vi, n, (int64_t)D * H * W), out + fv_grid<SV>(vo, n, (int64_t)D * H * W),
                         E + n * gwords, R + n * gwords, D, H, W, zs, nslabs, sm, vi, vo);
}

// ---- wave-level plane closure (single-launch path) --------------------------------------------
// One wavefront owns a z-plane: lane = row y (64 rows per group).  Along x the closure is the carry
// trick per row; along y it is a segmented OR-scan over the lanes (Kogge-Stone on (reach, empty)
// pairs with wavefront shuffles), so a plane converges in a few passes instead of one row step per
// iteration.  Returns wave-uniform "changed".
__device__ __forceinline__ u64 shfl_up64(u64 v, int d) { return (u64)__shfl_up((long long)v, d, 64); }
__device__ __forceinline__ u64 shfl_dn64(u64 v, int d) { return (u64)__shfl_down((long long)v, d, 64); }

template <int WX>
__device__ bool plane_close(const u64* e_pl, u64* r_pl, const u64* r_lo, const u64* r_hi, int H) {
  const int lane = threadIdx.x & 63;
  const int ngrp = (H + 63) >> 6;
  bool changed = false;
  // z neighbours, then x closure (row parallel)
  for (int grp = 0; grp < ngrp; ++grp) {
    const int y = grp * 64 + lane;
    if (y < H) {
      u64 e[WX], r[WX];
      bool ch = false;
#pragma unroll
      for (int k = 0; k < WX; ++k) {
        e[k] = e_pl[y * WX + k];
        const u64 old = r_pl[y * WX + k];
        r[k] = old | ((r_lo[y * WX + k] | r_hi[y * WX + k]) & e[k]);
        ch |= r[k] != old;
      }
      ch |= relax_row<WX>(e, r);
      if (ch) {
#pragma unroll
        for (int k = 0; k < WX; ++k) r_pl[y * WX + k] = r[k];
        changed = true;
      }
    }
  }
  for (int pass = 0; pass < 4096; ++pass) {
    bool ch_pass = false;
    // +y: reach flows to higher rows through runs of empty voxels
    u64 carry[WX];
#pragma unroll
    for (int k = 0; k < WX; ++k) carry[k] = 0ull;
    for (int grp = 0; grp < ngrp; ++grp) {
      const int y = grp * 64 + lane;
#pragma unroll
      for (int k = 0; k < WX; ++k) {
        const u64 p0 = y < H ? e_pl[y * WX + k] : 0ull, g0 = y < H ? r_pl[y * WX + k] : 0ull;
        u64 G = g0, P = p0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          u64 gs = shfl_up64(G, d), ps = shfl_up64(P, d);
          if (lane < d) { gs = 0ull; ps = ~0ull; }
          G |= P & gs; P &= ps;
        }
        u64 gin = shfl_up64(G, 1), pin = shfl_up64(P, 1);          // exclusive prefix
        if (lane == 0) { gin = 0ull; pin = ~0ull; }
        const u64 cin = gin | (pin & carry[k]);
        const u64 v = g0 | (p0 & cin);
        if (v != g0) { r_pl[y * WX + k] = v; ch_pass = true; }
        carry[k] = __shfl((long long)v, 63, 64);
      }
    }
    // -y
#pragma unroll
    for (int k = 0; k < WX; ++k) carry[k] = 0ull;
    for (int grp = ngrp - 1; grp >= 0; --grp) {
      const int y = grp * 64 + lane;
#pragma unroll
      for (int k = 0; k < WX; ++k) {
        const u64 p0 = y < H ? e_pl[y * WX + k] : 0ull, g0 = y < H ? r_pl[y * WX + k] : 0ull;
        u64 G = g0, P = p0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          u64 gs = shfl_dn64(G, d), ps = shfl_dn64(P, d);
          if (lane + d > 63) { gs = 0ull; ps = ~0ull; }
          G |= P & gs; P &= ps;
        }
        u64 gin = shfl_dn64(G, 1), pin = shfl_dn64(P, 1);
        if (lane == 63) { gin = 0ull; pin = ~0ull; }
        const u64 cin = gin | (pin & carry[k]);
        const u64 v = g0 | (p0 & cin);
        if (v != g0) { r_pl[y * WX + k] = v; ch_pass = true; }
        carry[k] = __shfl((long long)v, 0, 64);
      }
    }
    if (!__any(ch_pass)) break;
    changed = true;
    // new reach spreads along x
    bool ch_x = false;
    for (int grp = 0; grp < ngrp; ++grp) {
      const int y = grp * 64 + lane;
      if (y < H) {
        u64 e[WX], r[WX];
#pragma unroll
        for (int k = 0; k < WX; ++k) { e[k] = e_pl[y * WX + k]; r[k] = r_pl[y * WX + k]; }
        if (relax_row<WX>(e, r)) {
#pragma unroll
          for (int k = 0; k < WX; ++k) r_pl[y * WX + k] = r[k];
          ch_x = true;
        }
      }
    }
    if (!__any(ch_x)) break;
  }
  return __any(changed);
}

// slab held in LDS: one wavefront per plane for the in-plane closure, then one thread per (row, word)
// column for the closure along z; block-uniform "changed"
template <int WX>
__device__ int relax_slab_waves(const u64* El, u64* Rl, int nz, int H) {
  const int rowsz = H * WX;
  const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  int any = 0;
  for (int iter = 0; iter < 100000; ++iter) {
    int changed = 0;
    for (int p = wave; p < nz; p += nwaves)
      changed |= plane_close<WX>(El + (size_t)p * rowsz, Rl + (size_t)(p + 1) * rowsz, Rl + (size_t)p * rowsz,
                                 Rl + (size_t)(p + 2) * rowsz, H) ? 1 : 0;
    const int c1 = __syncthreads_or(changed);
    int zch = 0;
    for (int i = threadIdx.x; i < rowsz; i += blockDim.x) {
      u64 carry = Rl[i];                                    // halo below
      for (int p = 0; p < nz; ++p) {
        const u64 e = El[(size_t)p * rowsz + i], old = Rl[(size_t)(p + 1) * rowsz + i];
        const u64 v = old | (carry & e);
        if (v != old) { Rl[(size_t)(p + 1) * rowsz + i] = v; zch = 1; }
        carry = v;
      }
      carry = Rl[(size_t)(nz + 1) * rowsz + i];             // halo above
      for (int p = nz - 1; p >= 0; --p) {
        const u64 e = El[(size_t)p * rowsz + i], old = Rl[(size_t)(p + 1) * rowsz + i];
        const u64 v = old | (carry & e);
        if (v != old) { Rl[(size_t)(p + 1) * rowsz + i] = v; zch = 1; }
        carry = v;
      }
    }
    const int c2 = __syncthreads_or(zch);
    if (c1 | c2) any = 1;
    if (!c2) break;          // every plane is closed in-plane and nothing moves along z: fixed point
  }
  return any;
}

// ---- single-launch path -------------------------------------------------------------------------
// One workgroup per z-slab reads its part of the input grid straight into LDS bitmaps (ballot),
// relaxes, exchanges boundary planes with the neighbouring slabs of the same grid through HBM, and
// writes the {0,1} result from LDS: 8 B/voxel of HBM traffic for fp32, no bitmap round trip, no host
// synchronisation.  The slabs of one grid meet at a counter barrier once per exchange; the host
// launches at most as many workgroups as are co-resident (<= 1 per CU), so the spin-wait cannot
// starve a workgroup that has not started.  A bounded spin plus a round limit turn any surprise into the launch's
// `raised` flag, and the last workgroup to leave the launch redoes its grids alone (rescue_grid).


template <typename T, int WX, bool SV>
__global__ __launch_bounds__(1024) void fill_fused_kernel(const T* grid, T* out, int D, int H, int W, int zs,
                                                         int nslabs, u64* halo, FusedCtl* ctl, u64* E, u64* R,
                                                         int max_rounds, int fused_relaxed, FillView vi, FillView vo) {
  extern __shared__ __attribute__((aligned(16))) u64 sm[];
  const int slab = blockIdx.x % nslabs, n = blockIdx.x / nslabs;
  const int z0 = slab * zs, nz = min(zs, D - z0);
  const int rowsz = H * WX;
  u64* El = sm;                          // [nz][H][WX]
  u64* Rl = sm + (size_t)zs * rowsz;     // [nz+2][H][WX], plane 0 / nz+1 = halos
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const T* gsrc = SV ? grid + n * vi.sN + z0 * vi.sD : grid + ((int64_t)n * D + z0) * H * W;
  const int nrows = nz * H;
  // load + pack, 16-byte path (4-byte voxels, W a multiple of 64, aligned slab): the slab is one flat array; a lane
  // loads 4 consecutive voxels, 8 lanes = 32 voxels = one 32-bit piece of a row bitmap, assembled with three DPP
  // OR steps -- a quarter of the load instructions of the one-voxel-per-lane path below, whose load phase was
  // bound by the rate of (coalesced) dword load instructions, not by HBM (33 us for 100 MB)
  const bool vec4 = !SV && sizeof(T) == 4 && (W & 63) == 0 && ((reinterpret_cast<uintptr_t>(gsrc) & 15) == 0);
  if (vec4) {
    constexpr int NV = 8;
    typedef T __attribute__((ext_vector_type(4))) T4;
    const T4* g4 = reinterpret_cast<const T4*>(gsrc);
    const int total = nrows * (W / 4);
    unsigned* El32 = reinterpret_cast<unsigned*>(El);
    unsigned* Rl32 = reinterpret_cast<unsigned*>(Rl + rowsz);
    for (int u0 = wave * NV * 64; u0 < total; u0 += nwaves * NV * 64) {
      T4 vals[NV];
#pragma unroll
      for (int j = 0; j < NV; ++j) vals[j] = g4[min(u0 + j * 64 + lane, total - 1)];
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const int u = u0 + j * 64 + lane;
        unsigned nib = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) nib |= (!(vals[j][i] > (T)0) ? 1u : 0u) << i;
        int v = (int)(nib << (4 * (lane & 7)));
        v |= __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);    // quad_perm [1,0,3,2]
        v |= __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);    // quad_perm [2,3,0,1]
        v |= __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false);   // row_half_mirror: the other quad of the 8
        if ((lane & 7) == 0 && u < total) {
          const int f = u * 4, row = f / W, p = (f - row * W) >> 5;       // 32-bit piece p of the row
          const int y = row % H, z = z0 + row / H;
          const unsigned e = (unsigned)v;
          El32[row * (WX * 2) + p] = e;
          Rl32[row * (WX * 2) + p] = (y == 0 || z == 0) ? e : (p == 0 ? (e & 1u) : 0u);
        }
      }
    }
  }
  // one wave per row, RW rows (RW*WX loads per lane) in flight
  constexpr int RW = WX <= 2 ? 8 : 4;
  for (int r0 = vec4 ? nrows : wave * RW; r0 < nrows; r0 += nwaves * RW) {
    // branch-free: every load is issued (clamped address) before the first value is used
    T vals[RW][WX];
#pragma unroll
    for (int j = 0; j < RW; ++j)
#pragma unroll
      for (int k = 0; k < WX; ++k)
        vals[j][k] = gsrc[fv_at<SV>(vi, min(r0 + j, nrows - 1), min(k * 64 + lane, W - 1), H, W)];
    bool emp[RW][WX];
#pragma unroll
    for (int j = 0; j < RW; ++j)
#pragma unroll
      for (int k = 0; k < WX; ++k) emp[j][k] = (r0 + j < nrows && k * 64 + lane < W) && !(vals[j][k] > (T)0);
#pragma unroll
    for (int j = 0; j < RW; ++j)
#pragma unroll
      for (int k = 0; k < WX; ++k) {
        const u64 e = __ballot(emp[j][k]);
        const int row = r0 + j;
        if (lane == 0 && row < nrows) {
          const int y = row % H, z = z0 + row / H;
          El[row * WX + k] = e;
          Rl[rowsz + row * WX + k] = (y == 0 || z == 0) ? e : (k == 0 ? (e & 1ull) : 0ull);
        }
      }
  }
  for (int i = threadIdx.x; i < rowsz; i += blockDim.x) { Rl[i] = 0ull; Rl[(nz + 1) * rowsz + i] = 0ull; }
  __syncthreads();

  FusedCtl* c = ctl + n;
  u64* hb = halo + (int64_t)n * nslabs * 2 * 2 * rowsz;       // [parity][slab][lo/hi][rowsz]
  T* gdst = SV ? out + n * vo.sN + z0 * vo.sD : out + ((int64_t)n * D + z0) * H * W;
  // unpack + store from the LDS bitmaps (an in-place call overwrites its input only here)
  auto store_slab = [&]() {
    // 16-byte path (same condition as the load): the slab is one flat array of 64-voxel words, word w = El[w]; 16 lanes
    // write the 64 voxels of a word as float4s, a wave 4 words per instruction -- a quarter of the store instructions
    // of the one-voxel-per-lane path below (the store phase was bound by their rate, like the load phase before it)
    if (vec4 && (reinterpret_cast<uintptr_t>(gdst) & 15) == 0) {
      typedef T __attribute__((ext_vector_type(4))) T4;
      T4* d4 = reinterpret_cast<T4*>(gdst);
      const int nwords = nrows * WX, sub = lane >> 4, q4 = lane & 15;
      constexpr int NU = 4;
      for (int w0 = wave * 4 * NU; w0 < nwords; w0 += nwaves * 4 * NU) {
#pragma unroll
        for (int j = 0; j < NU; ++j) {
          const int w = w0 + j * 4 + sub;
          if (w < nwords) {
            const u64 outside = El[w] & Rl[rowsz + w];
            const unsigned nib = (unsigned)(outside >> (4 * q4)) & 15u;
            T4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = ((nib >> i) & 1u) ? (T)0 : (T)1;
            // written through (sc0 sc1): the result is not read again by this launch, and lines left dirty in the L2s are
            // written back at the end of the kernel, when nothing else runs (52.6 -> 50.3 us per call against nt stores)
            if constexpr (sizeof(T) == 4)
              asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" :: "v"(d4 + (int64_t)w * 16 + q4), "v"(v) : "memory");
          }
        }
      }
      return;
    }
    for (int r0 = wave; r0 < nrows; r0 += nwaves) {
#pragma unroll
      for (int k = 0; k < WX; ++k) {
        const int x = k * 64 + lane;
        const u64 outside = El[r0 * WX + k] & Rl[rowsz + r0 * WX + k];
        if (x < W) gdst[fv_at<SV>(vo, r0, x, H, W)] = ((outside >> lane) & 1ull) ? (T)0 : (T)1;
      }
    }
  };
  bool ok = true;
  int pend = 0;
  // the departure from a round (which clears its words) is issued by lane 0 of wave 1 and looked at one round later,
  // when the counter's old value has long arrived: off the critical path of the round
  const bool janitor = threadIdx.x == 64;
  unsigned dep_old = 0; int dep_it = -1;
  auto dep_finish = [&]() {
    if (janitor && dep_it >= 0) {
      if (dep_old == (unsigned)nslabs - 1u) {
        __hip_atomic_store(&c->word[dep_it], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&c->depart[dep_it], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      dep_it = -1;
    }
  };
  for (int it = 0; it < max_rounds; ++it) {
    const int any = (it == 0 || pend) ? relax_slab_waves<WX>(El, Rl, nz, H) : 0;
    if (nslabs == 1) break;
    dep_finish();
    // publish my boundary planes, then meet the other slabs of this grid
    u64* mine = hb + ((int64_t)(it & 1) * nslabs + slab) * 2 * rowsz;
    for (int i = threadIdx.x; i < rowsz; i += blockDim.x) {
      __hip_atomic_store(mine + i, Rl[rowsz + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(mine + rowsz + i, Rl[(size_t)nz * rowsz + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // The exchange never touches the caches' maintenance instructions.  Plane words are agent-scope atomic stores (written
    // through to the agent's coherence point) and agent-scope atomic loads (which bypass the non-coherent caches); every
    // wave waits for its own stores to be acknowledged, the workgroup barrier collects the waves, and only then does
    // thread 0 announce the slab with ONE relaxed read-modify-write (arrival + vote in one word; separate count / flag words
    // cost two more memory round trips per round) and poll with relaxed loads.  The release / acquire form of the same
    // protocol (other devices: buffer_wbl2 + buffer_inv at agent scope) writes back every dirty line this XCD's L2
    // holds -- the previous call's output, other kernels' data -- before the arrival counts: 3.4 us per round against
    // 0.8 us, 62-64 us per call against 54-58 (12 x 128^3).
    // The words of round `it` are those of round it - kFusedIters, cleared long ago by that round's last leaver.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    __shared__ int s_go;
    unsigned* wp = &c->word[it & (kFusedIters - 1)];
    if (threadIdx.x == 0) {
      const unsigned before = __hip_atomic_fetch_add(wp, 1u + ((any || it == 0) ? 0x10000u : 0u),
                                                     fused_relaxed ? __ATOMIC_RELAXED : __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      int spins = 0;
      unsigned v;
      while (((v = __hip_atomic_load(wp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) & 0xFFFFu) < (unsigned)nslabs &&
             ++spins < (1 << 22))
        __builtin_amdgcn_s_sleep(2);
      if (!fused_relaxed) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      // an arrival count that was not below nslabs BEFORE this slab arrived, or that ends above it, is not of this round: words
      // left behind by a launch that did not end (a fault killed it).  Give up like for a missing partner: the flag goes up, the
      // last workgroup out redoes the grids alone and clears every control word of the launch.
      const bool stale = (before & 0xFFFFu) >= (unsigned)nslabs || (v & 0xFFFFu) > (unsigned)nslabs;
      s_go = ((v & 0xFFFFu) < (unsigned)nslabs || stale) ? -1 : (int)(v >> 16);
    }
    __syncthreads();
    const int go = s_go;
    __syncthreads();
    if (janitor && go >= 0) {
      dep_old = __hip_atomic_fetch_add(&c->depart[it & (kFusedIters - 1)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      dep_it = it & (kFusedIters - 1);
    }
    if (go < 0) { ok = false; break; }          // a partner never arrived (should not happen)
    if (go == 0) break;                         // no slab of this grid changed: fixed point
    if (it + 1 == max_rounds) { ok = false; break; }
    // neighbours' boundary planes -> halos
    const u64* par = hb + (int64_t)(it & 1) * nslabs * 2 * rowsz;
    for (int i = threadIdx.x; i < rowsz; i += blockDim.x) {
      if (slab > 0) Rl[i] = __hip_atomic_load(par + ((int64_t)(slab - 1) * 2 + 1) * rowsz + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (slab + 1 < nslabs) Rl[(size_t)(nz + 1) * rowsz + i] = __hip_atomic_load(par + ((int64_t)(slab + 1) * 2) * rowsz + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    // does a halo reach an empty, not yet reached voxel of my boundary planes?  If not, this slab is at its fixed
    // point for these halos and the next relaxation is skipped (it could only report "no change")
    int pnd = 0;
    for (int i = threadIdx.x; i < rowsz; i += blockDim.x) {
      pnd |= (Rl[i] & El[i] & ~Rl[rowsz + i]) != 0ull;
      pnd |= (Rl[(size_t)(nz + 1) * rowsz + i] & El[(size_t)(nz - 1) * rowsz + i] & ~Rl[(size_t)nz * rowsz + i]) != 0ull;
    }
    pend = __syncthreads_or(pnd);
  }
  // A workgroup that gave up writes nothing and raises the launch's flag.  Every workgroup, once its own stores are
  // acknowledged, counts itself out; the last one out looks at the flag and, if it is up, redoes the launch's grids
  // alone (rescue_grid: no inter-workgroup dependency, so it always terminates; the host never has to look, i.e.
  // crn_fill_voxels stays asynchronous like the reference op, fill_voxels_gpu.cu:158-165).  It reads `grid` again: a
  // failed launch leaves each grid either untouched or (in place, some slabs) already at the final answer, and the fill
  // is idempotent on such a mix (empties only shrink to the reached set), so the result is the same fixed point.
  // The control blocks are all zeros again when the launch ends, whatever happened.
  FusedCtl* L = ctl;                                        // the launch's words live in its first grid's block
  if (ok) { store_slab(); dep_finish(); }
  else if (threadIdx.x == 0) __hip_atomic_store(&L->raised, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  __shared__ int s_last;
  if (threadIdx.x == 0) {
    const unsigned left = __hip_atomic_fetch_add(&L->exits, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int last = left == gridDim.x - 1u, redo = 0;
    if (last) {
      redo = __hip_atomic_load(&L->raised, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
      if (!redo) __hip_atomic_store(&L->exits, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    s_last = last && redo;
  }
  __syncthreads();
  if (!s_last) return;
  const int G = gridDim.x / nslabs;
  const int64_t gwords = (int64_t)D * rowsz;
  const int nsl = (D + zs - 1) / zs;
  for (int g = 0; g < G; ++g)
    rescue_grid<T, WX, SV>(grid + fv_grid<SV>(vi, g, (int64_t)D * H * W), out + fv_grid<SV>(vo, g, (int64_t)D * H * W),
                           E + g * gwords, R + g * gwords, D, H, W, zs, nsl, sm, vi, vo);
  unsigned* cw = reinterpret_cast<unsigned*>(ctl);
  for (int i = threadIdx.x; i < (int)(G * sizeof(FusedCtl) / 4); i += blockDim.x)
    __hip_atomic_store(cw + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}



constexpr int CRN_EAGAIN = -1000;     // internal: use the multi-launch path

// Control buffer of the single-launch path for one caller workspace: allocated and zeroed (on the call's stream) the
// first time that workspace is seen or when it has to grow -- that call cannot be part of a stream capture, every
// later one can.  Calls that share a workspace are ordered by the caller anyway (they share its bitmaps and halos).
// A control buffer is NEVER freed while the process lives: a captured HIP graph keeps the address it saw, so a
// workspace that grows gets a new buffer and the outgrown one stays allocated, and no entry is ever evicted (64 KiB per
// distinct workspace address; torch's caching allocator hands the same few addresses out again and again).
struct FillControl { const void* ws; char* buf; size_t bytes; };
std::mutex g_fill_mu;
std::vector<FillControl> g_fill_controls;
char* fill_control(const void* ws, size_t bytes, hipStream_t st) {
  std::lock_guard<std::mutex> lock(g_fill_mu);
  FillControl* slot = nullptr;
  for (auto& f : g_fill_controls) if (f.ws == ws && f.bytes >= bytes) slot = &f;
  if (slot) return slot->buf;
  const size_t want = std::max(bytes, (size_t)64 * 1024);
  char* buf = nullptr;
  if (hipMalloc(&buf, want) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  if (hipMemsetAsync(buf, 0, want, st) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(buf); return nullptr; }
  g_fill_controls.push_back({ws, buf, want});          // (an outgrown entry of the same workspace stays: a graph may replay it)
  return buf;
}
// The cache-maintenance-free exchange (write-through stores, acknowledged, relaxed arrival) is outside what the HIP / LLVM memory
// model promises; it rests on how gfx950 implements agent-scope atomics (written through / cache-bypassing) and on vmcnt covering
// stores.  It is measured and tested on MI355X (bit-exact on every fixture incl. the serpentine grid's hundreds of rounds); on any
// other device name the release / acquire form is used.
int fill_relaxed_default() {
  static const int v = [] {
    int dev = 0; hipDeviceProp_t p;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess) return 0;
    return strncmp(p.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
  }();
  return v;
}
constexpr size_t kSweepLds = 144 * 1024;
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t fused_offset(int64_t nwords) { return 2 * align256((size_t)nwords * 8) + 4096 * sizeof(int) + 256; }

template <typename T, int WX, bool SV>
int launch_fused(const T* grid, T* out, int G, int D, int H, int W, int zs, int nslabs, size_t lds, u64* halo,
                 FusedCtl* ctl, u64* E, u64* R, int max_rounds, int relaxed, hipStream_t st, FillView vi, FillView vo) {
  return crn_launch(fill_fused_kernel<T, WX, SV>, dim3(G * nslabs), dim3(1024), lds, st, grid, out, D, H, W, zs, nslabs, halo, ctl, E, R,
                    max_rounds, relaxed, vi, vo);
}

template <typename T, int WX, bool SV>
int launch_rescue(const T* grid, T* out, u64* E, u64* R, int N, int D, int H, int W, hipStream_t st, FillView vi, FillView vo) {
  const size_t plane = (size_t)H * WX * 8;
  int zs = (int)std::min<size_t>((size_t)D, (kSweepLds / plane - 2) / 2);
  if (zs < 1) return CRN_EINVAL;
  const int nslabs = (D + zs - 1) / zs;
  zs = (D + nslabs - 1) / nslabs;
  const size_t lds = (size_t)(2 * zs + 2) * plane;
  return crn_launch(fill_rescue_kernel<T, WX, SV>, dim3(N), dim3(512), lds, st, grid, out, E, R, D, H, W, zs, nslabs, vi, vo);
}

// ONE launch per call (per G grids): the single-launch kernel carries its own rescue path (its last workgroup out);
// nothing here waits for the GPU.  CRN_FILL_RESCUE=1 (tests): run the rescue body alone, one workgroup per grid.
template <typename T, bool SV>
int run_fill_fused(const T* grid, T* out, int N, int D, int H, int W, int WX, void* ws, hipStream_t st, FillView vi, FillView vo) {
  static const bool off = getenv("CRN_FILL_MULTI") != nullptr;
  static const bool rescue_only = getenv("CRN_FILL_RESCUE") != nullptr;
  if (off) return CRN_EAGAIN;
  const size_t plane = (size_t)H * WX * 8;
  const int zs_max = (int)std::min<size_t>((size_t)D, (kSweepLds / plane - 2) / 2);
  if (zs_max < 1) return CRN_EAGAIN;
  const int nslabs_min = (D + zs_max - 1) / zs_max;
  static const int kResident = [] {                    // workgroups guaranteed co-resident: one per CU
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
    return cus;
  }();
  if (kResident < 1) return CRN_EAGAIN;
  if (nslabs_min > kResident) return CRN_EAGAIN;
  const int G = std::min(N, kResident / nslabs_min);   // grids per launch
  // at least 4 planes per slab (when the LDS allows it): every slab boundary is a potential exchange round
  int nslabs = std::min(std::max(nslabs_min, (D + 3) / 4), std::max(nslabs_min, kResident / G));
  int zs = (D + nslabs - 1) / nslabs;
  nslabs = (D + zs - 1) / zs;
  const size_t lds = (size_t)(2 * zs + 2) * plane;
  const int64_t nwords = (int64_t)N * D * H * WX;
  u64* E = reinterpret_cast<u64*>(ws);
  u64* R = reinterpret_cast<u64*>(reinterpret_cast<char*>(ws) + align256((size_t)nwords * 8));
  char* base = reinterpret_cast<char*>(ws) + fused_offset(nwords);
  // control blocks: library-owned, all zeros between calls (see FusedCtl) -- no memset in front of the launch
  char* cbase = fill_control(ws, align256((size_t)N * sizeof(FusedCtl)), st);
  if (!cbase) return CRN_ENOMEM;
  FusedCtl* ctl = reinterpret_cast<FusedCtl*>(cbase);
  u64* halo = reinterpret_cast<u64*>(base + align256((size_t)N * sizeof(FusedCtl)) + 256);
  // rounds: bounded only to bound a launch's run time (tests: CRN_FILL_MAXROUNDS forces the failure path)
  static const int max_rounds = getenv("CRN_FILL_MAXROUNDS") ? std::max(2, atoi(getenv("CRN_FILL_MAXROUNDS"))) : (1 << 16);
  const int relaxed = fill_relaxed_default();
  const int64_t gstride = SV ? vi.sN : (int64_t)D * H * W, ostride = SV ? vo.sN : (int64_t)D * H * W;
  const int64_t hstride = (int64_t)nslabs * 2 * 2 * H * WX;
  for (int g0 = 0; g0 < N && !rescue_only; g0 += G) {
    const int Gn = std::min(G, N - g0);
    int rc = CRN_EINVAL;
#define CRN_FUSED(K) case K: rc = launch_fused<T, K, SV>(grid + g0 * gstride, out + g0 * ostride, Gn, D, H, W, zs, nslabs, lds, \
                                                     halo + g0 * hstride, ctl + g0, E + g0 * (int64_t)D * H * WX, R + g0 * (int64_t)D * H * WX, max_rounds, relaxed, st, vi, vo); break;
    switch (WX) { CRN_FUSED(1) CRN_FUSED(2) CRN_FUSED(3) CRN_FUSED(4) CRN_FUSED(5) CRN_FUSED(6) CRN_FUSED(7) CRN_FUSED(8) }
#undef CRN_FUSED
    if (rc != CRN_OK) return rc;
  }
  if (!rescue_only) return CRN_OK;
  int rc = CRN_EINVAL;
#define CRN_RESCUE(K) case K: rc = launch_rescue<T, K, SV>(grid, out, E, R, N, D, H, W, st, vi, vo); break;
  switch (WX) { CRN_RESCUE(1) CRN_RESCUE(2) CRN_RESCUE(3) CRN_RESCUE(4) CRN_RESCUE(5) CRN_RESCUE(6) CRN_RESCUE(7) CRN_RESCUE(8) }
#undef CRN_RESCUE
  return rc;
}

template <typename T, bool SV>
int run_fill(const T* grid, T* out, int N, int D, int H, int W, void* ws, hipStream_t st, FillView vi = FillView{},
             FillView vo = FillView{}) {
  const int WX = (W + 63) / 64;
  const int64_t nwords = (int64_t)N * D * H * WX;
  if (WX <= 8) {
    const int rc = run_fill_fused<T, SV>(grid, out, N, D, H, W, WX, ws, st, vi, vo);
    if (rc != CRN_EAGAIN) return rc;
  }
  // any other size (rows wider than 512 voxels, planes beyond the LDS budget, CRN_FILL_MULTI=1): one persistent
  // workgroup per grid on bitmaps in the workspace -- still a single asynchronous launch, no host wait
  u64* E = reinterpret_cast<u64*>(ws);
  u64* R = reinterpret_cast<u64*>(reinterpret_cast<char*>(ws) + align256((size_t)nwords * 8));
  hipLaunchKernelGGL((fill_global_kernel<T, SV>), dim3(N), dim3(1024), 0, st, grid, out, E, R, D, H, W, WX, vi, vo);
  CRN_CHECK_LAUNCH();
  return CRN_OK;
}

}  // namespace

extern "C" size_t crn_fill_voxels_workspace_bytes(int N, int D, int H, int W) {
  const int WX = (W + 63) / 64;
  const size_t nwords = (size_t)N * D * H * WX;
  const size_t multi = fused_offset((int64_t)nwords);      // the two bitmaps (any-size and rescue kernels) + slack
  // single-launch path: control blocks + status + halo planes (2 parities x 2 planes per slab, <= D slabs)
  const size_t fused = align256((size_t)N * sizeof(FusedCtl)) + 256 + (size_t)N * D * 4 * H * WX * 8 + 256;
  return multi + fused;
}

extern "C" int crn_fill_voxels(const void* grid, void* out, int dtype, int N, int D, int H, int W,
                               void* workspace, size_t workspace_bytes, crnStream stream) {
  CRN_ENTRY(stream);
  hipStream_t st = (hipStream_t)stream;
  if (!grid || !out || N < 1 || D < 1 || H < 1 || W < 1) return CRN_EINVAL;
  if (workspace_bytes < crn_fill_voxels_workspace_bytes(N, D, H, W)) return CRN_ENOMEM;
  switch (dtype) {
    case 0: return run_fill<float, false>((const float*)grid, (float*)out, N, D, H, W, workspace, st);
    case 1: return run_fill<uint8_t, false>((const uint8_t*)grid, (uint8_t*)out, N, D, H, W, workspace, st);
    case 2: return run_fill<int32_t, false>((const int32_t*)grid, (int32_t*)out, N, D, H, W, workspace, st);
    case 3: return run_fill<double, false>((const double*)grid, (double*)out, N, D, H, W, workspace, st);
    case 4: return run_fill<int64_t, false>((const int64_t*)grid, (int64_t*)out, N, D, H, W, workspace, st);
    case 5: return run_fill<int16_t, false>((const int16_t*)grid, (int16_t*)out, N, D, H, W, workspace, st);
    case 6: return run_fill<int8_t, false>((const int8_t*)grid, (int8_t*)out, N, D, H, W, workspace, st);
  }
  return CRN_EINVAL;
}

// Strided views of both tensors (element strides, any sign-free layout torch can produce): the reference op reads and
// writes through packed accessors (fill_voxels_gpu.cu:146-163), so `fill_inside_voxels_gpu(grid[:, ::2], inplace=True)`
// mutates the caller's view.  One launch like the contiguous entry; voxels move one per lane (no 16-byte paths).
extern "C" int crn_fill_voxels_strided(const void* grid, const int64_t* grid_strides, void* out, const int64_t* out_strides,
                                       int dtype, int N, int D, int H, int W, void* workspace, size_t workspace_bytes,
                                       crnStream stream) {
  CRN_ENTRY(stream);
  hipStream_t st = (hipStream_t)stream;
  if (!grid || !out || !grid_strides || !out_strides || N < 1 || D < 1 || H < 1 || W < 1) return CRN_EINVAL;
  for (int i = 0; i < 4; ++i) if (grid_strides[i] < 0 || out_strides[i] < 0) return CRN_EINVAL;
  if (workspace_bytes < crn_fill_voxels_workspace_bytes(N, D, H, W)) return CRN_ENOMEM;
  const FillView vi{grid_strides[0], grid_strides[1], grid_strides[2], grid_strides[3]};
  const FillView vo{out_strides[0], out_strides[1], out_strides[2], out_strides[3]};
  switch (dtype) {
    case 0: return run_fill<float, true>((const float*)grid, (float*)out, N, D, H, W, workspace, st, vi, vo);
    case 1: return run_fill<uint8_t, true>((const uint8_t*)grid, (uint8_t*)out, N, D, H, W, workspace, st, vi, vo);
    case 2: return run_fill<int32_t, true>((const int32_t*)grid, (int32_t*)out, N, D, H, W, workspace, st, vi, vo);
    case 3: return run_fill<double, true>((const double*)grid, (double*)out, N, D, H, W, workspace, st, vi, vo);
    case 4: return run_fill<int64_t, true>((const int64_t*)grid, (int64_t*)out, N, D, H, W, workspace, st, vi, vo);
    case 5: return run_fill<int16_t, true>((const int16_t*)grid, (int16_t*)out, N, D, H, W, workspace, st, vi, vo);
    case 6: return run_fill<int8_t, true>((const int8_t*)grid, (int8_t*)out, N, D, H, W, workspace, st, vi, vo);
  }
  return CRN_EINVAL;
}
