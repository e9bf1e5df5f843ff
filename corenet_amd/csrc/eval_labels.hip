// Streaming evaluation epilogue on gfx950 (corenet_amd.voxel_metrics.label_confusion, CoreNet.multi_offset_labels):
// argmax of ONE native pass of a multi-offset inference, scattered to that pass's sub-lattice of the x m label grid and
// counted into a K x K confusion matrix over the dataset's classes.  Contract: include/corenet_hip.h and DESIGN
// section 16; host twin: eval_labels_cpu.cpp (identical labels, cm and bad: every sum is an integer sum).
//
// One launch, grid (blocks, B), 256 threads.  A thread owns V consecutive coarse voxels of a row of sample b per round
// (V = 4 when W is a multiple of 4 and the scores are 16-byte aligned, else 1), lanes along W:
//   gt       read first, at the fine voxels ((z*m+iz) * mH + y*m+iy) * mW + x*m+ix: stride m between voxels (m = 1 and
//            V = 4: one 16-byte read)
//   scores   C reads of V * 256 B per wave, one class plane after the other (pointer += S: no 64-bit multiply per class)
//   labels   written at the same addresses as gt
//   counts   per-workgroup LDS histogram of K*K bins, then one 64-bit global atomic per non-zero bin and workgroup and one
//            32-bit add of each wave's rejected voxels.  With two logits (fg_bg: a sample hits at most four bins) a wave
//            first merges the lanes that share a bin -- ballot of the lanes whose bin equals the leader's, one LDS add of
//            the popcount, up to EL_ROUNDS distinct bins, the lanes left after that add on their own.  With more logits
//            every lane adds on its own.
#include "crn_common.h"
#include "eval_labels_common.h"

#include <algorithm>

namespace {

constexpr int EL_THREADS = 256;
constexpr int EL_ROUNDS = 4;

template <int AGG>
__device__ __forceinline__ void el_count(unsigned int* hist, int bin, int lane) {
  if (AGG > 0) {                                                    // every lane of the wave is here
    unsigned long long todo = __ballot(bin >= 0);
    for (int r = 0; r < AGG && todo; ++r) {                         // wave-uniform
      const int leader = __ffsll((long long)todo) - 1;
      const int lbin = __builtin_amdgcn_readlane(bin, leader);
      const unsigned long long same = __ballot(bin == lbin);
      if (lane == leader) atomicAdd(&hist[lbin], (unsigned int)__popcll(same));
      if (bin == lbin) bin = -1;
      todo &= ~same;
    }
  }
  if (bin >= 0) atomicAdd(&hist[bin], 1u);
}

// vec_io: m == 1, V == 4 and gt / labels 16-byte aligned -> their four voxels go as one int4
template <int CT, int V>
__global__ __launch_bounds__(EL_THREADS) void eval_labels_kernel(const float* __restrict__ scores, const int32_t* __restrict__ gt,
                                                                 const int32_t* __restrict__ scene_class, int C, int K, int H, int W,
                                                                 int64_t S, int m, int iz, int iy, int ix, int small, int vec_io,
                                                                 int32_t* __restrict__ labels, unsigned long long* __restrict__ cm,
                                                                 int32_t* __restrict__ bad) {
  constexpr int AGG = CT == 2 ? EL_ROUNDS : 0;
  extern __shared__ unsigned int el_hist[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int b = blockIdx.y;
  if (gt) {
    for (int i = tid; i < K * K; i += EL_THREADS) el_hist[i] = 0;
    __syncthreads();
  }
  const float* sb = scores + (int64_t)b * C * S;
  const int64_t sc = scene_class ? (int64_t)scene_class[b] : 1;
  const int64_t mW = (int64_t)W * m, mH = (int64_t)H * m;
  const int64_t fine_b = (int64_t)b * S * m * m * m;
  const int64_t items = S / V;                                      // V divides W
  unsigned int nbad = 0;                                            // lane 0 of each wave counts for its wave
  // block-uniform trip count: every lane of a wave takes part in the ballots below
  for (int64_t base = blockIdx.x * (int64_t)EL_THREADS; base < items; base += (int64_t)gridDim.x * EL_THREADS) {
    const int64_t q = base + tid;
    const bool in = q < items;
    int64_t pred[V], g[V];
#pragma unroll
    for (int u = 0; u < V; ++u) { pred[u] = 0; g[u] = 0; }
    if (in) {
      const int64_t v = q * V;
      int64_t f = v;
      if (m > 1) {
        int64_t x, y, z;
        if (small) {                                                // S < 2^31: 32-bit divisions
          const unsigned int vv = (unsigned int)v, row = vv / (unsigned int)W;
          x = vv - row * (unsigned int)W; z = row / (unsigned int)H; y = row - (unsigned int)z * (unsigned int)H;
        } else {
          const int64_t row = v / W;
          x = v - row * W; z = row / H; y = row - z * H;
        }
        f = ((z * m + iz) * mH + (y * m + iy)) * mW + (x * m + ix);
      }
      f += fine_b;
      if (gt) {
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
      if constexpr (V == 4) {
        const float* p = sb + v;
        float4 best = *reinterpret_cast<const float4*>(p);
        int4 bi = make_int4(0, 0, 0, 0);
#pragma unroll
        for (int c = 1; c < CT; ++c) {
          if (c < C) {
            p += S;
            const float4 s4 = *reinterpret_cast<const float4*>(p);
            if (s4.x > best.x) { best.x = s4.x; bi.x = c; }         // el_argmax's rule, four voxels at a time
            if (s4.y > best.y) { best.y = s4.y; bi.y = c; }
            if (s4.z > best.z) { best.z = s4.z; bi.z = c; }
            if (s4.w > best.w) { best.w = s4.w; bi.w = c; }
          }
        }
        pred[0] = bi.x * sc; pred[1] = bi.y * sc; pred[2] = bi.z * sc; pred[3] = bi.w * sc;
      } else {
        pred[0] = (int64_t)el_argmax<CT>(sb + v, C, S) * sc;
      }
      if (labels) {
        bool done = false;
        if constexpr (V == 4) {
          if (vec_io) {
            *reinterpret_cast<int4*>(labels + f) = make_int4((int32_t)pred[0], (int32_t)pred[1], (int32_t)pred[2], (int32_t)pred[3]);
            done = true;
          }
        }
        if (!done) {
#pragma unroll
          for (int u = 0; u < V; ++u) labels[f + (int64_t)u * m] = (int32_t)pred[u];
        }
      }
    }
    if (gt) {                                                       // kernel-uniform
#pragma unroll
      for (int u = 0; u < V; ++u) {
        const int bin = in ? el_bin(g[u] * sc, pred[u], K) : -1;
        const unsigned long long rej = __ballot(in && bin < 0);
        if (lane == 0) nbad += (unsigned int)__popcll(rej);
        el_count<AGG>(el_hist, bin, lane);
      }
    }
  }
  if (gt) {
    __syncthreads();
    for (int i = tid; i < K * K; i += EL_THREADS)
      if (el_hist[i]) atomicAdd(&cm[i], (unsigned long long)el_hist[i]);
    if (nbad) atomicAdd(bad, (int)nbad);
  }
}

// 8 rounds per thread, at most 512 workgroups per sample (argmax_confusion_kernel's launch shape): a workgroup's 32-bit
// LDS counts cannot overflow below S = 2^40 voxels per sample
inline int el_blocks(int64_t items) { return (int)std::min<int64_t>(std::max<int64_t>(1, (items + EL_THREADS * 8 - 1) / (EL_THREADS * 8)), 512); }

inline bool el_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int crn_eval_labels(const float* scores, const int32_t* gt, const int32_t* scene_class, int B, int C, int K, int D,
                               int H, int W, int m, int n, int32_t* labels, int64_t* cm, int32_t* bad, crnStream stream) {
  if (!el_args_ok(scores, gt, B, C, K, D, H, W, m, n, labels, cm, bad) || B > 65535) return CRN_EINVAL;
  CRN_ENTRY(stream);
  hipStream_t st = (hipStream_t)stream;
  const int64_t S = (int64_t)D * H * W;
  const int ix = n % m, iy = (n / m) % m, iz = (int)(n / ((int64_t)m * m));
  const int small = S < ((int64_t)1 << 31);
  const bool vec = W % 4 == 0 && el_aligned16(scores);
  const int vec_io = vec && m == 1 && el_aligned16(gt) && el_aligned16(labels);
  dim3 grid(el_blocks(vec ? S / 4 : S), B);
  const size_t sh = gt ? (size_t)K * K * sizeof(unsigned int) : 0;
#define CRN_EL2(CT, V) hipLaunchKernelGGL((eval_labels_kernel<CT, V>), grid, dim3(EL_THREADS), sh, st, scores, gt, scene_class, C, K, H, W, S, m, iz, iy, ix, small, vec_io, labels, reinterpret_cast<unsigned long long*>(cm), bad)
#define CRN_EL(CT) do { if (vec) CRN_EL2(CT, 4); else CRN_EL2(CT, 1); } while (0)
  if (C <= 2) CRN_EL(2); else if (C <= 4) CRN_EL(4); else if (C <= 8) CRN_EL(8);
  else if (C <= 16) CRN_EL(16); else CRN_EL(32);
#undef CRN_EL
#undef CRN_EL2
  CRN_CHECK_LAUNCH();
  return CRN_OK;
}
