// Score-level evaluation epilogue on gfx950 (corenet_amd.score_metrics.score_histogram, CoreNet.multi_offset_score_histogram):
// the scores of ONE native pass of a multi-offset inference, binned per class against that pass's sub-lattice of the x m
// label grid into table / sq / bad.  Contract: include/corenet_hip.h and DESIGN section 22; shared arithmetic:
// eval_scores_common.h; host twin: eval_scores_cpu.cpp (identical table, sq and bad: every sum is an integer sum).
//
// One launch, grid (chunks, B), 256 threads, eval_labels_kernel's structure: a workgroup owns CRN_SCORE_CHUNK = 8192
// consecutive coarse voxels of sample b, a thread V consecutive ones per round (V = 4 with 16-byte loads when W is a
// multiple of 4, the scores are 16-byte aligned and C <= 16, else 1: with 17..32 channels four voxels' scores and the 33
// pending entries do not fit 256 registers and V = 4 would spill), lanes along W; gt is read first at the fine voxels, then
// the C class planes one after the other (pointer += S), and with from_logits the shared softmax runs in registers.
//
// Counting.  A voxel makes C + 1 entries, and real grids are dominated by two keys per row ("void, p ~ 1" and "absent
// class, p ~ 0"): per-lane LDS atomics would serialise on a handful of addresses.  So
//   * a thread keeps, per channel (unrolled over CT, plus the foreground row), the last key (bin, y) with its pending
//     count and sum of q in registers and adds to LDS only when the key changes; the squared errors, which depend on
//     y alone, pend under y and are added only when y changes;
//   * what is still pending when the chunk is done is merged across the wave first: the lanes that share the first
//     lane's key are summed by a butterfly and added once, the others add on their own;
//   * count and sum of an entry share one 64-bit LDS word (count << 40 | sum): one LDS atomic per flush.
// A thread sees at most 8192 / 256 = 32 voxels, so its 32-bit pending sums stay below 32 * 2^24 = 2^29; a workgroup sees
// 8192, so an LDS word holds a sum below 2^37 < 2^40 and a count below 2^14, and nothing can wrap whatever the input.
// The workgroup then adds its non-zero words to the global table with 64-bit atomics.
#include "crn_common.h"
#include "eval_scores_common.h"

#include <algorithm>

namespace {

constexpr int ES_THREADS = 256;
constexpr int ES_SUM_BITS = 40;
constexpr unsigned long long ES_SUM_MASK = (1ull << ES_SUM_BITS) - 1;
typedef unsigned long long es_u64;

__device__ __forceinline__ es_u64 es_wave_sum(es_u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// vec_io: m == 1, V == 4 and gt 16-byte aligned -> its four voxels go as one int4
template <int CT, int V>
__global__ __launch_bounds__(ES_THREADS) void eval_scores_kernel(const float* __restrict__ scores, int from_logits,
                                                                 const int32_t* __restrict__ gt,
                                                                 const int32_t* __restrict__ scene_class, int C, int K, int H, int W,
                                                                 int64_t S, int m, int iz, int iy, int ix, int small, int vec_io,
                                                                 int nbins, es_u64* __restrict__ table, es_u64* __restrict__ sq,
                                                                 es_u64* __restrict__ bad) {
  extern __shared__ es_u64 es_lds[];
  const int E2 = (K + 1) * nbins * 2, R2 = (K + 1) * 2;
  es_u64* ent = es_lds;                                             // [K+1][nbins][2]: count << 40 | sum of q
  es_u64* sqs = es_lds + E2;                                        // [K+1][2]
  es_u64* nbd = sqs + R2;                                           // [1]
  const int tid = threadIdx.x, lane = tid & 63;
  const int b = blockIdx.y;
  for (int i = tid; i < E2 + R2 + 1; i += ES_THREADS) es_lds[i] = 0;
  __syncthreads();
  const float* sb = scores + (int64_t)b * C * S;
  const int64_t sc = scene_class ? (int64_t)scene_class[b] : 1;
  const bool sample_ok = sc >= 1 && (int64_t)(C - 1) * sc < K;
  const int isc = sample_ok ? (int)sc : 0;                          // rows c * isc stay inside [0, K)
  const int64_t mW = (int64_t)W * m, mH = (int64_t)H * m;
  const int64_t fine_b = (int64_t)b * S * m * m * m;
  const int64_t v0 = (int64_t)blockIdx.x * CRN_SCORE_CHUNK, v1 = v0 + CRN_SCORE_CHUNK < S ? v0 + CRN_SCORE_CHUNK : S;

  int pk[CT + 1], py[CT + 1];                                       // pending key (bin * 2 + y) and y of the pending sq; -1: none
  unsigned int pc[CT + 1], ps[CT + 1], pq[CT + 1];
#pragma unroll
  for (int c = 0; c <= CT; ++c) { pk[c] = -1; py[c] = -1; pc[c] = 0; ps[c] = 0; pq[c] = 0; }
  unsigned int nbad = 0;

  // V divides W, S and the chunk: an item never straddles a row, the chunk or the sample
  for (int64_t v = v0 + (int64_t)tid * V; v < v1; v += ES_THREADS * V) {
    int64_t f = v;
    if (m > 1) {
      int64_t x, y, z;
      if (small) {                                                  // S < 2^31: 32-bit divisions
        const unsigned int vv = (unsigned int)v, row = vv / (unsigned int)W;
        x = vv - row * (unsigned int)W; z = row / (unsigned int)H; y = row - (unsigned int)z * (unsigned int)H;
      } else {
        const int64_t row = v / W;
        x = v - row * W; z = row / H; y = row - z * H;
      }
      f = ((z * m + iz) * mH + (y * m + iy)) * mW + (x * m + ix);
    }
    f += fine_b;
    if (!sample_ok) { nbad += V; continue; }
    int64_t g[V];
    {
      bool done = false;
      if constexpr (V == 4) {
        if (vec_io) {
          const int4 gv = *reinterpret_cast<const int4*>(gt + f);
          g[0] = gv.x; g[1] = gv.y; g[2] = gv.z; g[3] = gv.w;
          done = true;
        }
      }
      if (!done) {
#pragma unroll
        for (int u = 0; u < V; ++u) g[u] = gt[f + (int64_t)u * m];
      }
    }
    float xs[V][CT];
    {
      const float* p = sb + v;
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        if (c < C) {
          if constexpr (V == 4) {
            const float4 s4 = *reinterpret_cast<const float4*>(p);
            xs[0][c] = s4.x; xs[1][c] = s4.y; xs[2][c] = s4.z; xs[3][c] = s4.w;
          } else {
            xs[0][c] = *p;
          }
          p += S;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < V; ++u) {
      if (from_logits) es_softmax<CT>(xs[u], C);
      const int64_t gg = g[u] * sc;
      bool ok = gg >= 0 && gg < K;
#pragma unroll
      for (int c = 0; c < CT; ++c)
        if (c < C) ok = ok && es_p_ok(xs[u][c]);
      if (!ok) { ++nbad; continue; }
      const int gi = (int)gg;
      int q0 = 0;
#pragma unroll
      for (int c = 0; c <= CT; ++c) {
        if (c < C || c == CT) {
          int q, y, row;
          if (c < CT) {
            q = es_q(xs[u][c]); row = c * isc; y = gi == row;
            if (c == 0) q0 = q;
          } else {
            q = ES_ONE - q0; row = K; y = gi != 0;
          }
          const int key = es_bin(q, nbins) * 2 + y;
          if (key != pk[c]) {
            if (pk[c] >= 0) atomicAdd(&ent[row * nbins * 2 + pk[c]], ((es_u64)pc[c] << ES_SUM_BITS) | ps[c]);
            pk[c] = key; pc[c] = 0; ps[c] = 0;
          }
          pc[c] += 1; ps[c] += (unsigned int)q;
          if (y != py[c]) {
            if (py[c] >= 0) atomicAdd(&sqs[row * 2 + py[c]], (es_u64)pq[c]);
            py[c] = y; pq[c] = 0;
          }
          pq[c] += es_sq(q, y);
        }
      }
    }
  }

  // what is still pending: every lane of the wave is here (C is kernel-uniform)
#pragma unroll
  for (int c = 0; c <= CT; ++c) {
    if (c < C || c == CT) {
      const int row = c < CT ? c * isc : K;
      int key = pk[c];
      const es_u64 todo = __ballot(key >= 0);
      if (todo) {                                                   // wave-uniform
        const int leader = __ffsll((long long)todo) - 1;
        const int lkey = __builtin_amdgcn_readlane(key, leader);
        const bool same = key == lkey;
        const es_u64 sum = es_wave_sum(same ? (((es_u64)pc[c] << ES_SUM_BITS) | ps[c]) : 0ull);
        if (lane == leader) atomicAdd(&ent[row * nbins * 2 + lkey], sum);
        if (same) key = -1;
      }
      if (key >= 0) atomicAdd(&ent[row * nbins * 2 + key], ((es_u64)pc[c] << ES_SUM_BITS) | ps[c]);
#pragma unroll
      for (int y = 0; y < 2; ++y) {
        const es_u64 sum = es_wave_sum(py[c] == y ? (es_u64)pq[c] : 0ull);
        if (lane == 0 && sum) atomicAdd(&sqs[row * 2 + y], sum);
      }
    }
  }
  if (nbad) atomicAdd(nbd, (es_u64)nbad);
  __syncthreads();
  for (int i = tid; i < E2; i += ES_THREADS) {
    const es_u64 w = ent[i];
    if (w) {
      atomicAdd(&table[2 * i], w >> ES_SUM_BITS);
      if (w & ES_SUM_MASK) atomicAdd(&table[2 * i + 1], w & ES_SUM_MASK);
    }
  }
  for (int i = tid; i < R2; i += ES_THREADS)
    if (sqs[i]) atomicAdd(&sq[i], sqs[i]);
  if (tid == 0 && nbd[0]) atomicAdd(bad, nbd[0]);
}

template <int CT>
__global__ __launch_bounds__(ES_THREADS) void score_softmax_kernel(const float* __restrict__ in, int C, int64_t S,
                                                                   float* __restrict__ out) {
  const int64_t base = (int64_t)blockIdx.y * C * S;
  for (int64_t v = blockIdx.x * (int64_t)ES_THREADS + threadIdx.x; v < S; v += (int64_t)gridDim.x * ES_THREADS) {
    float x[CT];
    const float* p = in + base + v;
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C) { x[c] = *p; p += S; }
    es_softmax<CT>(x, C);
    float* o = out + base + v;
#pragma unroll
    for (int c = 0; c < CT; ++c)
      if (c < C) { *o = x[c]; o += S; }
  }
}

inline bool es_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int crn_eval_scores_tiles(int32_t* out3) {
  if (!out3) return CRN_EINVAL;
  out3[0] = CRN_SCORE_CHUNK; out3[1] = CRN_SCORE_MAX_ENTRIES; out3[2] = CRN_SCORE_MAX_NBINS;
  return CRN_OK;
}

extern "C" int crn_eval_scores(const float* scores, int from_logits, const int32_t* gt, const int32_t* scene_class, int B, int C,
                               int K, int D, int H, int W, int m, int n, int nbins, int64_t* table, int64_t* sq, int64_t* bad,
                               crnStream stream) {
  if (!es_args_ok(scores, gt, B, C, K, D, H, W, m, n, nbins, table, sq, bad) || B > 65535) return CRN_EINVAL;
  const int64_t S = (int64_t)D * H * W;
  const int64_t chunks = (S + CRN_SCORE_CHUNK - 1) / CRN_SCORE_CHUNK;
  if (chunks >= (1 << 24)) return CRN_EINVAL;                       // grid.x * 256 threads must stay below 2^32
  CRN_ENTRY(stream);
  hipStream_t st = (hipStream_t)stream;
  const int ix = n % m, iy = (n / m) % m, iz = (int)(n / ((int64_t)m * m));
  const int small = S < ((int64_t)1 << 31);
  const bool vec = W % 4 == 0 && es_aligned16(scores) && C <= 16;
  const int vec_io = vec && m == 1 && es_aligned16(gt);
  dim3 grid((unsigned int)chunks, B);
  const size_t sh = ((size_t)(K + 1) * nbins * 2 + (size_t)(K + 1) * 2 + 1) * sizeof(es_u64);      // at most 33 816 bytes
#define CRN_ES2(CT, V) hipLaunchKernelGGL((eval_scores_kernel<CT, V>), grid, dim3(ES_THREADS), sh, st, scores, from_logits, gt, scene_class, C, K, H, W, S, m, iz, iy, ix, small, vec_io, nbins, reinterpret_cast<es_u64*>(table), reinterpret_cast<es_u64*>(sq), reinterpret_cast<es_u64*>(bad))
#define CRN_ES(CT) do { if (vec) CRN_ES2(CT, 4); else CRN_ES2(CT, 1); } while (0)
  if (C <= 2) CRN_ES(2); else if (C <= 4) CRN_ES(4); else if (C <= 8) CRN_ES(8);
  else if (C <= 16) CRN_ES(16); else CRN_ES2(32, 1);
#undef CRN_ES
#undef CRN_ES2
  CRN_CHECK_LAUNCH();
  return CRN_OK;
}

extern "C" int crn_score_softmax(const float* logits, int B, int C, int64_t S, float* out, crnStream stream) {
  if (!es_softmax_args_ok(logits, B, C, S, out) || B > 65535) return CRN_EINVAL;
  CRN_ENTRY(stream);
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned int)std::min<int64_t>((S + ES_THREADS - 1) / ES_THREADS, 1 << 20), B);
#define CRN_ES(CT) hipLaunchKernelGGL((score_softmax_kernel<CT>), grid, dim3(ES_THREADS), 0, st, logits, C, S, out)
  if (C <= 2) CRN_ES(2); else if (C <= 4) CRN_ES(4); else if (C <= 8) CRN_ES(8);
  else if (C <= 16) CRN_ES(16); else CRN_ES(32);
#undef CRN_ES
  CRN_CHECK_LAUNCH();
  return CRN_OK;
}
