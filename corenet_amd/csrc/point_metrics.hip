// Surface sampling and brute-force nearest neighbours on gfx950 (corenet_amd.mesh_metrics: Chamfer distance and F-score
// of predicted against ground-truth surfaces).  Contract: include/corenet_hip.h and DESIGN section 15; the per-element
// arithmetic is point_metrics_common.h, shared with the host twin (point_metrics_cpu.cpp), which returns the same arrays.
//
// sample_surface, two launches:
//   weights  one workgroup per object: the largest eligible area (a maximum: exact in any order), then the inclusive
//            64-bit scan of the integer weights round(area / max * 2^24), 1024 triangles per round -> workspace
//   sample   one thread per (object, sample): hash -> stratified position in the integer total -> binary search of the
//            scanned weights -> square-root warp inside the triangle
// nearest, one launch (three when the candidates of an object are split):
//   a workgroup holds 1024 queries of one object in registers (4 per lane) and walks the object's candidates (or its
//   share of them) in tiles of 1024, staged in LDS as three arrays x / y / z; every lane of a wave reads the same LDS
//   address (a broadcast: no bank conflicts), four candidates per ds_read_b128.  The inner loop is VALU only: two
//   candidates per packed subtract / multiply / add, then a compare and two selects per pair keep (d2, index); candidates
//   come in ascending index and only a strictly smaller d2 replaces the best, so ties go to the lowest index.
//   When objects x query tiles cannot fill the chip the candidate range is cut into `splits` shares; every share merges
//   its (d2, index) with a 64-bit atomicMin on (bits(d2) << 32) | index (d2 >= 0, so the bits order like the value; the
//   minimum commutes, so the result does not depend on which workgroup finishes first).
// point_triangle, two launches (four when the triangles of an object are split):
//   records  one thread per triangle: pm_tri_record -> 20 floats in the workspace (NaNs for a triangle that is not eligible)
//   pt       nn_kernel's layout with triangle records in place of points: 1024 queries of one object in registers, tiles
//            of 256 records in LDS (20 KiB), five broadcast ds_read_b128 per record, then pm_tri_d2 for each of the lane's
//            four queries: selects only, no bounds test (NaN padding), strict < in ascending order.  Split and merge as above.
#include "crn_common.h"
#include "point_metrics_common.h"

namespace {

constexpr int PM_SCAN_THREADS = 1024;
constexpr int PM_SCAN_WAVES = PM_SCAN_THREADS / 64;
constexpr int PM_SAMPLE_THREADS = 256;
constexpr int NN_THREADS = 256;
constexpr int NN_QPT = 4;                              // queries per lane
constexpr int NN_QTILE = NN_THREADS * NN_QPT;          // queries per workgroup
constexpr int NN_TB = 1024;                            // candidates per LDS tile (3 x 4 KiB)
constexpr int NN_TARGET_WGS = 1024;                    // 256 CUs x 4 workgroups of 4 waves
constexpr unsigned long long NN_KEY_NONE = 0x7f800000ffffffffull;     // (+inf, -1)

typedef float f32x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(PM_SCAN_THREADS) void pm_weights_kernel(const float* __restrict__ tri, const int64_t* __restrict__ off,
                                                                     int64_t* __restrict__ cum, int64_t* __restrict__ total,
                                                                     uint8_t* __restrict__ valid) {
  __shared__ float smax[PM_SCAN_WAVES];
  __shared__ long long ssum[PM_SCAN_WAVES];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t t0 = off[n], t1 = off[n + 1];
  float m = 0.f;
  for (int64_t k = t0 + tid; k < t1; k += PM_SCAN_THREADS) {
    const float a = pm_area(tri + 9 * k);
    if (pm_area_ok(a) && a > m) m = a;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (lane == 0) smax[wid] = m;
  __syncthreads();
  float amax = smax[0];
#pragma unroll
  for (int w = 1; w < PM_SCAN_WAVES; ++w) amax = fmaxf(amax, smax[w]);
  if (!(amax > 0.f)) {                                   // uniform: no triangle of the object can carry a sample
    if (tid == 0) { valid[n] = 0; total[n] = 0; }
    return;
  }
  long long carry = 0;
  for (int64_t base = t0; base < t1; base += PM_SCAN_THREADS) {
    const int64_t k = base + tid;
    long long v = k < t1 ? (long long)pm_weight(pm_area(tri + 9 * k), amax) : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long u = __shfl_up(v, o, 64);
      if (lane >= o) v += u;
    }
    if (lane == 63) ssum[wid] = v;
    __syncthreads();
    long long pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < PM_SCAN_WAVES; ++w) {
      const long long x = ssum[w];
      if (w < wid) pre += x;
      tot += x;
    }
    if (k < t1) cum[k] = carry + pre + v;
    carry += tot;
    __syncthreads();
  }
  if (tid == 0) { valid[n] = 1; total[n] = carry; }
}

__global__ __launch_bounds__(PM_SAMPLE_THREADS) void pm_sample_kernel(const float* __restrict__ tri, const int64_t* __restrict__ off,
                                                                      const int64_t* __restrict__ cum, const int64_t* __restrict__ total,
                                                                      int bps, int64_t S, uint32_t seed, float* __restrict__ points,
                                                                      int32_t* __restrict__ tri_index) {
  const int n = blockIdx.x / bps;
  const int64_t i = (int64_t)(blockIdx.x - n * bps) * PM_SAMPLE_THREADS + threadIdx.x;
  if (i >= S) return;
  const int64_t o = (int64_t)n * S + i, tot = total[n];
  float p[3] = {0.f, 0.f, 0.f};
  int32_t k = -1;
  if (tot > 0) pm_sample(tri, cum, off[n], off[n + 1], tot, i, S, seed, p, &k);
  points[3 * o] = p[0];
  points[3 * o + 1] = p[1];
  points[3 * o + 2] = p[2];
  tri_index[o] = k;
}

__global__ void nn_keys_init_kernel(unsigned long long* __restrict__ keys, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) keys[i] = NN_KEY_NONE;
}

__global__ void nn_keys_final_kernel(const unsigned long long* __restrict__ keys, int64_t n, float* __restrict__ dist2,
                                     int32_t* __restrict__ index) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = keys[i];
  dist2[i] = __uint_as_float((unsigned)(k >> 32));
  index[i] = (int32_t)(unsigned)(k & 0xffffffffu);
}

// grid (query tiles, splits, objects of this launch).  SPLIT: merge through keys; else write dist2 / index directly.
template <bool SPLIT>
__global__ __launch_bounds__(NN_THREADS) void nn_kernel(const float* __restrict__ a, const int64_t* __restrict__ a_off,
                                                        const float* __restrict__ b, const int64_t* __restrict__ b_off, int n0,
                                                        float* __restrict__ dist2, int32_t* __restrict__ index,
                                                        unsigned long long* __restrict__ keys) {
  __shared__ __attribute__((aligned(16))) float sb[3][NN_TB];
  const int n = n0 + blockIdx.z, tid = threadIdx.x;
  const int64_t a0 = a_off[n], na = a_off[n + 1] - a0;
  const int64_t q0 = (int64_t)blockIdx.x * NN_QTILE;
  if (q0 >= na) return;                                                   // uniform
  const int64_t b0 = b_off[n], nb = b_off[n + 1] - b0;
  const int64_t tiles = (nb + NN_TB - 1) / NN_TB;
  const int64_t per = ((tiles + gridDim.y - 1) / gridDim.y) * NN_TB;      // candidates per share, whole tiles
  const int64_t c_begin = (int64_t)blockIdx.y * per;
  const int64_t c_end = c_begin + per < nb ? c_begin + per : nb;
  if (SPLIT && c_begin >= c_end) return;                                  // uniform; the keys are initialised

  float ax[NN_QPT], ay[NN_QPT], az[NN_QPT], best[NN_QPT];
  int32_t bi[NN_QPT];
#pragma unroll
  for (int k = 0; k < NN_QPT; ++k) {
    const int64_t q = q0 + k * NN_THREADS + tid;
    const bool in = q < na;
    ax[k] = in ? a[3 * (a0 + q)] : NAN;                                   // a query past the end never finds anything
    ay[k] = in ? a[3 * (a0 + q) + 1] : NAN;
    az[k] = in ? a[3 * (a0 + q) + 2] : NAN;
    best[k] = INFINITY;
    bi[k] = -1;
  }
  const float* bo = b + 3 * b0;
  for (int64_t c0 = c_begin; c0 < c_end; c0 += NN_TB) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 3 * NN_TB / NN_THREADS; ++r) {                    // the tile's 3 * NN_TB floats, coalesced
      const int f = r * NN_THREADS + tid, j = f / 3, c = f - 3 * j;
      sb[c][j] = c0 + j < c_end ? bo[3 * c0 + f] : NAN;                   // NaN padding: never chosen, no bounds test below
    }
    __syncthreads();
    const int32_t cbase = (int32_t)c0;
#pragma unroll 2
    for (int j = 0; j < NN_TB; j += 4) {
      const f32x4 X = *reinterpret_cast<const f32x4*>(&sb[0][j]);
      const f32x4 Y = *reinterpret_cast<const f32x4*>(&sb[1][j]);
      const f32x4 Z = *reinterpret_cast<const f32x4*>(&sb[2][j]);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f32x2 bx = h ? X.zw : X.xy, by = h ? Y.zw : Y.xy, bz = h ? Z.zw : Z.xy;
#pragma unroll
        for (int k = 0; k < NN_QPT; ++k) {
          const f32x2 dx = ax[k] - bx, dy = ay[k] - by, dz = az[k] - bz;
          const f32x2 d2 = (dx * dx + dy * dy) + dz * dz;
          if (d2.x < best[k]) { best[k] = d2.x; bi[k] = cbase + j + 2 * h; }
          if (d2.y < best[k]) { best[k] = d2.y; bi[k] = cbase + j + 2 * h + 1; }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NN_QPT; ++k) {
    const int64_t q = q0 + k * NN_THREADS + tid;
    if (q >= na) continue;
    if (bi[k] < 0 && ax[k] == ax[k] && ay[k] == ay[k] && az[k] == az[k]) {
      // nothing was strictly below +inf: the first candidate at +inf (an overflow, not a NaN) is the (d2, index) minimum
      for (int64_t j = c_begin; j < c_end; ++j) {
        const float d2 = pm_d2(ax[k], ay[k], az[k], bo[3 * j], bo[3 * j + 1], bo[3 * j + 2]);
        if (d2 == d2) { bi[k] = (int32_t)j; break; }
      }
    }
    if (SPLIT) {
      atomicMin(&keys[a0 + q], ((unsigned long long)__float_as_uint(best[k]) << 32) | (unsigned)bi[k]);
    } else {
      dist2[a0 + q] = best[k];
      index[a0 + q] = bi[k];
    }
  }
}

// ---------------- point to triangle ----------------
constexpr int PT_THREADS = 256;
constexpr int PT_QPT = 4;                              // queries per lane
constexpr int PT_QTILE = PT_THREADS * PT_QPT;          // queries per workgroup
constexpr int PT_TB = 256;                             // triangle records per LDS tile (256 x 80 B = 20 KiB)
constexpr int PT_REC4 = PM_TRI_REC / 4;                // 16-byte reads per record
static_assert(PM_TRI_REC % 4 == 0 && (PT_TB * PT_REC4) % PT_THREADS == 0, "a tile is whole float4 rounds of the workgroup");
static_assert(CRN_PT_QUERY_TILE == PT_QTILE && CRN_PT_TRIANGLE_TILE == PT_TB, "the header states the tiles");

// one thread per triangle of the whole soup: its record, or NaNs when it is not eligible
__global__ __launch_bounds__(256) void pt_records_kernel(const float* __restrict__ tri, int64_t T, float* __restrict__ rec) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= T) return;
  float r[PM_TRI_REC];
  pm_tri_record(tri + 9 * k, r);
  f32x4* out = reinterpret_cast<f32x4*>(rec + PM_TRI_REC * k);
#pragma unroll
  for (int i = 0; i < PT_REC4; ++i) out[i] = f32x4{r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]};
}

// grid (query tiles, splits, objects of this launch), as nn_kernel.  rec: the records of the whole soup.
template <bool SPLIT>
__global__ __launch_bounds__(PT_THREADS) void pt_kernel(const float* __restrict__ p, const int64_t* __restrict__ p_off,
                                                        const float* __restrict__ rec, const int64_t* __restrict__ t_off, int n0,
                                                        float* __restrict__ dist2, int32_t* __restrict__ index,
                                                        unsigned long long* __restrict__ keys) {
  __shared__ f32x4 sr[PT_TB * PT_REC4];
  const int n = n0 + blockIdx.z, tid = threadIdx.x;
  const int64_t p0 = p_off[n], np = p_off[n + 1] - p0;
  const int64_t q0 = (int64_t)blockIdx.x * PT_QTILE;
  if (q0 >= np) return;                                                   // uniform
  const int64_t t0 = t_off[n], nt = t_off[n + 1] - t0;
  const int64_t tiles = (nt + PT_TB - 1) / PT_TB;
  const int64_t per = ((tiles + gridDim.y - 1) / gridDim.y) * PT_TB;      // triangles per share, whole tiles
  const int64_t c_begin = (int64_t)blockIdx.y * per;
  const int64_t c_end = c_begin + per < nt ? c_begin + per : nt;
  if (SPLIT && c_begin >= c_end) return;                                  // uniform; the keys are initialised

  float ax[PT_QPT], ay[PT_QPT], az[PT_QPT], best[PT_QPT];
  int32_t bi[PT_QPT];
#pragma unroll
  for (int k = 0; k < PT_QPT; ++k) {
    const int64_t q = q0 + k * PT_THREADS + tid;
    const bool in = q < np;
    ax[k] = in ? p[3 * (p0 + q)] : NAN;                                   // a query past the end never finds anything
    ay[k] = in ? p[3 * (p0 + q) + 1] : NAN;
    az[k] = in ? p[3 * (p0 + q) + 2] : NAN;
    best[k] = INFINITY;
    bi[k] = -1;
  }
  const f32x4* ro = reinterpret_cast<const f32x4*>(rec + PM_TRI_REC * t0);
  const f32x4 nan4 = {NAN, NAN, NAN, NAN};
  for (int64_t c0 = c_begin; c0 < c_end; c0 += PT_TB) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < PT_TB * PT_REC4 / PT_THREADS; ++r) {              // the tile's records, coalesced 16-byte reads
      const int f = r * PT_THREADS + tid;
      sr[f] = c0 + f / PT_REC4 < c_end ? ro[c0 * PT_REC4 + f] : nan4;     // NaN padding: never chosen, no bounds test below
    }
    __syncthreads();
    const int32_t cbase = (int32_t)c0;
#pragma unroll 2
    for (int j = 0; j < PT_TB; ++j) {
      float r[PM_TRI_REC];
#pragma unroll
      for (int i = 0; i < PT_REC4; ++i) {                                 // every lane reads the same address: a broadcast
        const f32x4 v = sr[j * PT_REC4 + i];
        r[4 * i] = v.x; r[4 * i + 1] = v.y; r[4 * i + 2] = v.z; r[4 * i + 3] = v.w;
      }
#pragma unroll
      for (int k = 0; k < PT_QPT; ++k) {
        const float d2 = pm_tri_d2(ax[k], ay[k], az[k], r);
        const bool less = d2 < best[k];                                   // strict, ascending j: ties keep the lowest index
        best[k] = less ? d2 : best[k];
        bi[k] = less ? cbase + j : bi[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < PT_QPT; ++k) {
    const int64_t q = q0 + k * PT_THREADS + tid;
    if (q >= np) continue;
    if (SPLIT) {
      atomicMin(&keys[p0 + q], ((unsigned long long)__float_as_uint(best[k]) << 32) | (unsigned)bi[k]);
    } else {
      dist2[p0 + q] = best[k];
      index[p0 + q] = bi[k];
    }
  }
}

struct PtLayout {
  size_t o_rec, o_keys, bytes;
};

PtLayout pt_layout(int64_t Np, int64_t T) {
  PtLayout L;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  L.o_rec = 0;                                           // float [T][PM_TRI_REC]
  L.o_keys = al((size_t)T * PM_TRI_REC * 4);             // uint64 [Np]
  L.bytes = al(L.o_keys + (size_t)Np * 8);
  return L;
}

// shares the triangles of an object are cut into: enough for NN_TARGET_WGS workgroups, at most one per tile
int64_t pt_splits(int N, int64_t max_np, int64_t max_nt) {
  const int64_t qtiles = (max_np + PT_QTILE - 1) / PT_QTILE;
  const int64_t ctiles = (max_nt + PT_TB - 1) / PT_TB;
  if (N < 1 || qtiles < 1) return 1;
  int64_t splits = (NN_TARGET_WGS + N * qtiles - 1) / (N * qtiles);
  if (splits > ctiles) splits = ctiles;
  if (splits > 65535) splits = 65535;
  return splits < 1 ? 1 : splits;
}

struct PmLayout {
  size_t o_cum, o_total, bytes;
};

PmLayout pm_layout(int64_t T, int N) {
  PmLayout L;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  L.o_cum = 0;                                           // int64 [T]
  L.o_total = al((size_t)T * 8);                         // int64 [N]
  L.bytes = al(L.o_total + (size_t)N * 8);
  return L;
}

}  // namespace

extern "C" size_t crn_sample_surface_workspace_bytes(int64_t T, int N) {
  if (T < 0 || N < 1) return 0;
  return pm_layout(T, N).bytes;
}

extern "C" int crn_sample_surface(const float* triangles, const int64_t* tri_offsets, int N, int64_t T, int64_t S, uint32_t seed,
                                  void* workspace, size_t workspace_bytes, float* points, int32_t* tri_index, uint8_t* valid,
                                  crnStream s) {
  if (N < 1 || T < 0 || S < 1 || S > CRN_PM_MAX_SAMPLES || !tri_offsets || !workspace || !points || !tri_index || !valid)
    return CRN_EINVAL;
  if (T > 0 && !triangles) return CRN_EINVAL;
  const PmLayout L = pm_layout(T, N);
  const int64_t bps = (S + PM_SAMPLE_THREADS - 1) / PM_SAMPLE_THREADS;
  if (workspace_bytes < L.bytes || (int64_t)N * bps >= ((int64_t)1 << 31)) return CRN_EINVAL;
  int64_t* cum = (int64_t*)((char*)workspace + L.o_cum);
  int64_t* total = (int64_t*)((char*)workspace + L.o_total);
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(pm_weights_kernel, dim3((unsigned)N), dim3(PM_SCAN_THREADS), 0, st, triangles, tri_offsets, cum, total, valid);
  CRN_CHECK_LAUNCH();
  hipLaunchKernelGGL(pm_sample_kernel, dim3((unsigned)((int64_t)N * bps)), dim3(PM_SAMPLE_THREADS), 0, st, triangles, tri_offsets,
                     (const int64_t*)cum, (const int64_t*)total, (int)bps, S, seed, points, tri_index);
  CRN_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t crn_nearest_workspace_bytes(int64_t Na) { return Na > 0 ? (size_t)Na * 8 : 0; }

extern "C" int crn_nearest(const float* a, const int64_t* a_offsets, const float* b, const int64_t* b_offsets, int N, int64_t Na,
                           int64_t max_na, int64_t max_nb, void* workspace, size_t workspace_bytes, float* dist2,
                           int32_t* index, crnStream s) {
  if (N < 1 || Na < 0 || max_na < 0 || max_na > Na || max_nb < 0 || max_nb > CRN_PM_MAX_CANDIDATES || !a_offsets || !b_offsets)
    return CRN_EINVAL;
  if (Na == 0 || max_na == 0) return 0;
  if (!a || !dist2 || !index || (max_nb > 0 && !b)) return CRN_EINVAL;
  const int64_t qtiles = (max_na + NN_QTILE - 1) / NN_QTILE;
  const int64_t ctiles = (max_nb + NN_TB - 1) / NN_TB;
  int64_t splits = (NN_TARGET_WGS + N * qtiles - 1) / (N * qtiles);
  if (splits > ctiles) splits = ctiles;
  if (splits > 65535) splits = 65535;
  if (splits < 1) splits = 1;
  if (qtiles >= ((int64_t)1 << 31)) return CRN_EINVAL;
  hipStream_t st = (hipStream_t)s;
  unsigned long long* keys = (unsigned long long*)workspace;
  const unsigned kb = (unsigned)((Na + 255) / 256);
  if (splits > 1) {
    if (!workspace || workspace_bytes < (size_t)Na * 8 || (Na + 255) / 256 >= ((int64_t)1 << 31)) return CRN_EINVAL;
    hipLaunchKernelGGL(nn_keys_init_kernel, dim3(kb), dim3(256), 0, st, keys, Na);
    CRN_CHECK_LAUNCH();
  }
  for (int n0 = 0; n0 < N; n0 += 65535) {
    const unsigned nz = (unsigned)(N - n0 < 65535 ? N - n0 : 65535);
    const dim3 grid((unsigned)qtiles, (unsigned)splits, nz);
    if (splits > 1)
      hipLaunchKernelGGL(nn_kernel<true>, grid, dim3(NN_THREADS), 0, st, a, a_offsets, b, b_offsets, n0, dist2, index, keys);
    else
      hipLaunchKernelGGL(nn_kernel<false>, grid, dim3(NN_THREADS), 0, st, a, a_offsets, b, b_offsets, n0, dist2, index, keys);
    CRN_CHECK_LAUNCH();
  }
  if (splits > 1) {
    hipLaunchKernelGGL(nn_keys_final_kernel, dim3(kb), dim3(256), 0, st, (const unsigned long long*)keys, Na, dist2, index);
    CRN_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" size_t crn_point_triangle_workspace_bytes(int64_t Np, int64_t T) {
  if (Np < 0 || T < 0) return 0;
  return pt_layout(Np, T).bytes;
}

extern "C" size_t crn_point_triangle_tile(int which) { return which == 0 ? PT_QTILE : which == 1 ? PT_TB : 0; }

extern "C" size_t crn_point_triangle_splits(int N, int64_t max_np, int64_t max_nt) {
  if (N < 1 || max_np < 0 || max_nt < 0) return 0;
  return (size_t)pt_splits(N, max_np, max_nt);
}

extern "C" int crn_point_triangle(const float* p, const int64_t* p_offsets, const float* triangles, const int64_t* t_offsets,
                                  int N, int64_t Np, int64_t T, int64_t max_np, int64_t max_nt, void* workspace,
                                  size_t workspace_bytes, float* dist2, int32_t* index, crnStream s) {
  if (N < 1 || Np < 0 || T < 0 || max_np < 0 || max_np > Np || max_nt < 0 || max_nt > T || max_nt > CRN_PM_MAX_CANDIDATES ||
      !p_offsets || !t_offsets)
    return CRN_EINVAL;
  if (Np == 0 || max_np == 0) return 0;
  if (!p || !dist2 || !index || (T > 0 && !triangles)) return CRN_EINVAL;
  const PtLayout L = pt_layout(Np, T);
  if (!workspace || workspace_bytes < L.bytes) return CRN_EINVAL;
  const int64_t qtiles = (max_np + PT_QTILE - 1) / PT_QTILE;
  const int64_t splits = pt_splits(N, max_np, max_nt);
  const int64_t rb = (T + 255) / 256, kb64 = (Np + 255) / 256;
  if (qtiles >= ((int64_t)1 << 31) || rb >= ((int64_t)1 << 31) || kb64 >= ((int64_t)1 << 31)) return CRN_EINVAL;
  hipStream_t st = (hipStream_t)s;
  float* rec = (float*)((char*)workspace + L.o_rec);
  unsigned long long* keys = (unsigned long long*)((char*)workspace + L.o_keys);
  const unsigned kb = (unsigned)kb64;
  if (T > 0) {
    hipLaunchKernelGGL(pt_records_kernel, dim3((unsigned)rb), dim3(256), 0, st, triangles, T, rec);
    CRN_CHECK_LAUNCH();
  }
  if (splits > 1) {
    hipLaunchKernelGGL(nn_keys_init_kernel, dim3(kb), dim3(256), 0, st, keys, Np);
    CRN_CHECK_LAUNCH();
  }
  for (int n0 = 0; n0 < N; n0 += 65535) {
    const unsigned nz = (unsigned)(N - n0 < 65535 ? N - n0 : 65535);
    const dim3 grid((unsigned)qtiles, (unsigned)splits, nz);
    if (splits > 1)
      hipLaunchKernelGGL(pt_kernel<true>, grid, dim3(PT_THREADS), 0, st, p, p_offsets, (const float*)rec, t_offsets, n0, dist2,
                         index, keys);
    else
      hipLaunchKernelGGL(pt_kernel<false>, grid, dim3(PT_THREADS), 0, st, p, p_offsets, (const float*)rec, t_offsets, n0, dist2,
                         index, keys);
    CRN_CHECK_LAUNCH();
  }
  if (splits > 1) {
    hipLaunchKernelGGL(nn_keys_final_kernel, dim3(kb), dim3(256), 0, st, (const unsigned long long*)keys, Np, dist2, index);
    CRN_CHECK_LAUNCH();
  }
  return 0;
}
