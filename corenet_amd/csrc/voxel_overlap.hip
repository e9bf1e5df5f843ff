// Label overlaps of two voxel grids on gfx950 (corenet_amd.voxel_overlap).  Contract: include/corenet_hip.h and DESIGN
// section 20; host twin: voxel_overlap_cpu.cpp (identical tables and bad counts: integer adds only).
//
// One kernel, one launch per VO_BATCH grids (their table offsets are kernel arguments; blockIdx.y picks the grid), no
// workgroup waits for another and every loop has a fixed or bounded trip count:
//   * a workgroup owns CRN_VO_CHUNK consecutive voxels of a grid, each of its VO_WAVES waves an equal share, which the
//     wave walks row by row (vo_rows: two contiguous grids are one row).
//   * a row piece is read as a scalar head up to the first voxel at which the rows of a and b are both 16-byte aligned,
//     a body of 16-byte loads -- a lane owns VO_UNIT consecutive voxels per round: 4 when both grids are int32 (one
//     load each), else 16 (one load of uint8, four of int32) -- and a scalar tail.  Rows whose alignments never agree
//     (the head search ends without a hit) are all head.
//   * a lane turns every voxel into its key a * (nb + 1) + b, merges equal consecutive keys into a run, and only a run
//     that ends is counted: key 0 and bad voxels in registers (summed over the wave at the end, one atomic per wave),
//     every other key by one atomic.  A unit whose words are all zero skips the keys altogether.
//   * LDS path (table of at most CRN_VO_LDS_ENTRIES entries, workgroup-uniform): runs go to a u32 table in LDS; after
//     one barrier its non-zero entries are added to the grid's table with 64-bit atomics.  Global path: runs go to
//     the grid's table with 64-bit atomics; no LDS, no barrier.
// A grid whose num_a / num_b do not give the table length the host passed is counted as bad altogether, so no key ever
// lies outside the table the host allocated.
#include "crn_common.h"
#include "voxel_overlap_common.h"

namespace {

constexpr int VO_WAVES = 8;
constexpr int VO_THREADS = VO_WAVES * 64;
constexpr int VO_SHARE = CRN_VO_CHUNK / VO_WAVES;          // voxels of a wave
constexpr int VO_BATCH = 64;                               // grids per launch
static_assert(CRN_VO_CHUNK % VO_WAVES == 0, "every wave owns the same share of a chunk");
static_assert(CRN_VO_LDS_ENTRIES * 4 <= 65536, "the LDS table needs no attribute and lets two workgroups share a CU");

struct VoBatch {
  int64_t off[VO_BATCH];       // first entry of the grid's table in the flat buffer
  int32_t entries[VO_BATCH];   // its length as the host sized it
};

// VO_UNIT consecutive voxels of one grid in registers, read with 16-byte loads from a 16-byte aligned address.
template <typename T, int U>
struct VoVec {
  static constexpr int WORDS = U * (int)sizeof(T) / 4;
  static_assert(WORDS % 4 == 0, "whole 16-byte loads");
  uint32_t w[WORDS];
  __device__ __forceinline__ void load(const T* p) {
#pragma unroll
    for (int k = 0; k < WORDS / 4; ++k) {
      const uint4 q = reinterpret_cast<const uint4*>(p)[k];
      w[4 * k] = q.x; w[4 * k + 1] = q.y; w[4 * k + 2] = q.z; w[4 * k + 3] = q.w;
    }
  }
  __device__ __forceinline__ int32_t get(int i) const {
    if (sizeof(T) == 4) return (int32_t)w[i];
    return (int32_t)((w[i >> 2] >> (8 * (i & 3))) & 255u);
  }
  __device__ __forceinline__ uint32_t any() const {
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < WORDS; ++k) r |= w[k];
    return r;
  }
};

__device__ __forceinline__ uint32_t vo_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The counting state of a lane: the open run, and the counts kept in registers.
template <bool LDS>
struct VoCount {
  uint32_t key = 0, run = 0, zero = 0, bad = 0;
  uint32_t* lds;
  unsigned long long* tab;
  __device__ __forceinline__ void close() {
    if (key == 0) zero += run;
    else if (key == VO_BAD) bad += run;
    else if (LDS) atomicAdd(lds + key, run);
    else atomicAdd(tab + key, (unsigned long long)run);
  }
  __device__ __forceinline__ void add(uint32_t k, uint32_t n) {
    if (k == key) { run += n; return; }
    if (run) close();
    key = k; run = n;
  }
};

template <typename TA, typename TB, bool LDS>
__device__ __forceinline__ void vo_walk(const TA* __restrict__ a, const TB* __restrict__ b, const VoRows& rw, int64_t v, int64_t v1,
                                        int32_t na, int32_t nb, int lane, VoCount<LDS>& c) {
  constexpr int U = (sizeof(TA) == 4 && sizeof(TB) == 4) ? 4 : 16;
  constexpr int UNR = U * (int)(sizeof(TA) + sizeof(TB)) <= 32 ? 4 : 2;      // units in flight per lane
  if (v >= v1) return;                                       // wave-uniform
  int64_t r = v / rw.L;
  int x = (int)(v - r * rw.L);
  while (v < v1) {                                           // at most the rows of the share
    const int64_t left = v1 - v;
    const int len = left < rw.L - x ? (int)left : rw.L - x;
    const int64_t r1 = r / rw.R2, r2 = r - r1 * rw.R2;
    const TA* pa = a + r1 * rw.a1 + r2 * rw.a2 + x;
    const TB* pb = b + r1 * rw.b1 + r2 * rw.b2 + x;
    int head = len;
    for (int h = 0; h < 16 && h < len; ++h)
      if ((((uintptr_t)(pa + h) | (uintptr_t)(pb + h)) & 15) == 0) { head = h; break; }
    for (int i = lane; i < head; i += 64) c.add(vo_key((int32_t)pa[i], (int32_t)pb[i], na, nb), 1);
    const int units = (len - head) / U;
    const TA* qa = pa + head;
    const TB* qb = pb + head;
    int u = lane;
    for (; u + 64 * (UNR - 1) < units; u += 64 * UNR) {      // UNR units of the lane, all loads first
      VoVec<TA, U> va[UNR];
      VoVec<TB, U> vb[UNR];
#pragma unroll
      for (int k = 0; k < UNR; ++k) { va[k].load(qa + (int64_t)(u + 64 * k) * U); vb[k].load(qb + (int64_t)(u + 64 * k) * U); }
#pragma unroll
      for (int k = 0; k < UNR; ++k) {
        if ((va[k].any() | vb[k].any()) == 0) { c.add(0, U); continue; }
#pragma unroll
        for (int i = 0; i < U; ++i) c.add(vo_key(va[k].get(i), vb[k].get(i), na, nb), 1);
      }
    }
    for (; u < units; u += 64) {
      VoVec<TA, U> va;
      VoVec<TB, U> vb;
      va.load(qa + (int64_t)u * U); vb.load(qb + (int64_t)u * U);
      if ((va.any() | vb.any()) == 0) { c.add(0, U); continue; }
#pragma unroll
      for (int i = 0; i < U; ++i) c.add(vo_key(va.get(i), vb.get(i), na, nb), 1);
    }
    for (int i = head + units * U + lane; i < len; i += 64) c.add(vo_key((int32_t)pa[i], (int32_t)pb[i], na, nb), 1);
    v += len; ++r; x = 0;
  }
}

template <typename TA, typename TB>
__global__ __launch_bounds__(VO_THREADS) void vo_kernel(const TA* __restrict__ a, int64_t aN, const TB* __restrict__ b, int64_t bN, VoRows rw,
                                                        int64_t S, const int64_t* __restrict__ num_a,
                                                        const int64_t* __restrict__ num_b, VoBatch bt, int64_t* table, int64_t* bad) {
  extern __shared__ __attribute__((aligned(16))) uint32_t vo_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.y;
  const int64_t c0 = (int64_t)blockIdx.x * CRN_VO_CHUNK;
  const int64_t c1 = c0 + CRN_VO_CHUNK < S ? c0 + CRN_VO_CHUNK : S;
  const int64_t entries = vo_entries_ok(num_a[n], num_b[n], bt.entries[n]);  // workgroup-uniform, like all that follows from it
  unsigned long long* badn = reinterpret_cast<unsigned long long*>(bad + n);
  if (entries < 0) {                                         // no table to count into: the chunk is bad
    if (threadIdx.x == 0) atomicAdd(badn, (unsigned long long)(c1 - c0));
    return;
  }
  const int32_t na = (int32_t)num_a[n], nb = (int32_t)num_b[n];
  unsigned long long* tab = reinterpret_cast<unsigned long long*>(table + bt.off[n]);
  const int64_t v = c0 + (int64_t)wave * VO_SHARE;
  const int64_t v1 = v + VO_SHARE < c1 ? v + VO_SHARE : c1;
  a += n * aN;
  b += n * bN;
  if (entries <= CRN_VO_LDS_ENTRIES) {
    for (int i = threadIdx.x; i < (int)entries; i += VO_THREADS) vo_lds[i] = 0;
    __syncthreads();                                         // every thread of the workgroup arrives: no return above on this path
    VoCount<true> c;
    c.lds = vo_lds; c.tab = tab;
    vo_walk<TA, TB, true>(a, b, rw, v, v1, na, nb, lane, c);
    if (c.run) c.close();
    const uint32_t zero = vo_wave_sum(c.zero), nbad = vo_wave_sum(c.bad);
    if (lane == 0 && zero) atomicAdd(vo_lds, zero);
    if (lane == 0 && nbad) atomicAdd(badn, (unsigned long long)nbad);
    __syncthreads();
    for (int i = threadIdx.x; i < (int)entries; i += VO_THREADS) {
      const uint32_t k = vo_lds[i];
      if (k) atomicAdd(tab + i, (unsigned long long)k);
    }
  } else {
    VoCount<false> c;
    c.lds = nullptr; c.tab = tab;
    vo_walk<TA, TB, false>(a, b, rw, v, v1, na, nb, lane, c);
    if (c.run) c.close();
    const uint32_t zero = vo_wave_sum(c.zero), nbad = vo_wave_sum(c.bad);
    if (lane == 0 && zero) atomicAdd(tab, (unsigned long long)zero);
    if (lane == 0 && nbad) atomicAdd(badn, (unsigned long long)nbad);
  }
}

template <typename TA, typename TB>
int vo_launch(const void* a, int64_t aN, const void* b, int64_t bN, const VoRows& rw, int64_t S, const int64_t* num_a,
              const int64_t* num_b, const VoBatch& bt, int nb, size_t lds, int64_t* table, int64_t* bad, hipStream_t st) {
  const dim3 g((unsigned)((S + CRN_VO_CHUNK - 1) / CRN_VO_CHUNK), (unsigned)nb), blk(VO_THREADS);
  return crn_launch(vo_kernel<TA, TB>, g, blk, lds, st, (const TA*)a, aN, (const TB*)b, bN, rw, S, num_a, num_b, bt, table, bad);
}

}  // namespace

extern "C" int crn_voxel_overlap_tiles(int32_t* out3) {
  if (!out3) return CRN_EINVAL;
  out3[0] = CRN_VO_CHUNK; out3[1] = CRN_VO_LDS_ENTRIES; out3[2] = CRN_VO_MAX_TABLE_ENTRIES;
  return CRN_OK;
}

extern "C" size_t crn_voxel_overlap_workspace_bytes(int N, const int64_t* table_offsets) {
  if (N < 1 || !vo_offsets_ok(N, table_offsets)) return 0;
  return table_offsets[N] > 0 ? (size_t)table_offsets[N] * 8 : 8;
}

extern "C" int crn_voxel_overlap(const void* a, const int64_t* strides_a, int dtype_a, const void* b, const int64_t* strides_b,
                                 int dtype_b, int N, int D, int H, int W, const int64_t* num_a, const int64_t* num_b,
                                 const int64_t* table_offsets, int64_t* table, size_t table_bytes, int64_t* bad, crnStream stream) {
  if (!vo_args_ok(a, strides_a, dtype_a, b, strides_b, dtype_b, N, D, H, W, num_a, num_b, table_offsets, table, bad)) return CRN_EINVAL;
  if (N == 0) return CRN_OK;
  if (table_offsets[N] > CRN_VO_MAX_TABLE_ENTRIES) return CRN_EINVAL;
  if (table_bytes < crn_voxel_overlap_workspace_bytes(N, table_offsets)) return CRN_ENOMEM;
  CRN_ENTRY(stream);
  hipStream_t st = (hipStream_t)stream;
  if (table_offsets[N] > 0) CRN_HIP(hipMemsetAsync(table, 0, (size_t)table_offsets[N] * 8, st));
  CRN_HIP(hipMemsetAsync(bad, 0, (size_t)N * 8, st));
  const VoRows rw = vo_rows(strides_a, strides_b, D, H, W);
  const int64_t S = (int64_t)D * H * W;
  const size_t ea = dtype_a == VO_U8 ? 1 : 4, eb = dtype_b == VO_U8 ? 1 : 4;
  for (int n0 = 0; n0 < N; n0 += VO_BATCH) {
    const int nb = N - n0 < VO_BATCH ? N - n0 : VO_BATCH;
    VoBatch bt = {};
    int64_t lds_entries = 0;
    for (int i = 0; i < nb; ++i) {
      const int64_t e = table_offsets[n0 + i + 1] - table_offsets[n0 + i];
      bt.off[i] = table_offsets[n0 + i];
      bt.entries[i] = (int32_t)e;
      if (e <= CRN_VO_LDS_ENTRIES && e > lds_entries) lds_entries = e;
    }
    const void* pa = (const char*)a + (size_t)n0 * strides_a[0] * ea;
    const void* pb = (const char*)b + (size_t)n0 * strides_b[0] * eb;
    const size_t lds = (size_t)lds_entries * 4;
    int rc;
    if (dtype_a == VO_U8)
      rc = dtype_b == VO_U8 ? vo_launch<uint8_t, uint8_t>(pa, strides_a[0], pb, strides_b[0], rw, S, num_a + n0, num_b + n0, bt, nb, lds, table, bad + n0, st)
                            : vo_launch<uint8_t, int32_t>(pa, strides_a[0], pb, strides_b[0], rw, S, num_a + n0, num_b + n0, bt, nb, lds, table, bad + n0, st);
    else
      rc = dtype_b == VO_U8 ? vo_launch<int32_t, uint8_t>(pa, strides_a[0], pb, strides_b[0], rw, S, num_a + n0, num_b + n0, bt, nb, lds, table, bad + n0, st)
                            : vo_launch<int32_t, int32_t>(pa, strides_a[0], pb, strides_b[0], rw, S, num_a + n0, num_b + n0, bt, nb, lds, table, bad + n0, st);
    if (rc != CRN_OK) return rc;
  }
  return CRN_OK;
}
