// Batched 3-D connected-component labelling on gfx950 (corenet_amd.voxel_components).  Contract: include/corenet_hip.h
// and DESIGN section 17; host twin: voxel_components_cpu.cpp (identical labels, counts and stats: they are a function of
// the partition alone).
//
// Six launches per call, none of which waits for another workgroup; every loop is a union-find walk over strictly
// decreasing indices or has a fixed trip count:
//   brick    one workgroup per CRN_VC_BRICK_D x _H x _W brick, parents and keys of the brick in LDS (64 KiB).  A wave owns
//            a row (lanes along w): a ballot of the run starts gives every voxel its run's first index without atomics;
//            runs of neighbouring rows are united in LDS (find with path splitting, hook the larger root under the smaller
//            with atomicMin); every voxel then writes its brick-local root as a per-grid linear index (background -1).
//   seam     one thread per voxel on the low faces of the bricks: unites it with its equal-keyed neighbours in other
//            bricks on the global parent array -- find both roots, atomicMin the larger root's parent to the smaller, and
//            when the returned value shows that the root had been hooked meanwhile, go on from that value.
//   flatten  every voxel finds its root and writes root + 1 into labels; a voxel is a root iff it is its set's lowest
//            index; roots are counted per chunk of VC_CHUNK voxels.
//   scan     one workgroup per grid: exclusive prefix sum of the chunk counts (fixed trip count), num_components.
//   number   every root takes its raster-order number (chunk offset + rank in the chunk) into parent[root].
//   relabel  labels[v] = parent[labels[v] - 1].
// p[x] <= x always holds, so every walk ends; while unions run (brick, seam) parents only ever decrease, in flatten a
// parent is only replaced by another ancestor.  Whatever the interleaving, when a launch has ended the unions it was given
// are all made, and the root of a set is its lowest index.  crn_component_stats: three more launches (see vc_stats_kernel).
#include "crn_common.h"
#include "voxel_components_common.h"

#include <algorithm>

namespace {

constexpr int BD = CRN_VC_BRICK_D, BH = CRN_VC_BRICK_H, BW = CRN_VC_BRICK_W;
constexpr int ROWS = BD * BH, BV = ROWS * BW;
constexpr int VC_BRICK_THREADS = 512, VC_BRICK_WAVES = VC_BRICK_THREADS / 64;
constexpr int VC_CHUNK = 1024;                   // voxels per chunk of the root count = threads of flatten / number / scan
constexpr int VC_THREADS = 256;
static_assert(BW == 64, "a wave owns a row of a brick");
static_assert(ROWS % VC_BRICK_WAVES == 0, "every wave owns the same number of rows");
static_assert(2 * BV * sizeof(int) <= 65536, "the brick's parents and keys fit 64 KiB of LDS");

// ---- union-find on an int array p with p[x] <= x; WG: LDS of one workgroup, else global memory shared by the launch ----
template <bool WG>
__device__ __forceinline__ int vc_load(const int* p) {
  if (WG) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Root of x.  Path splitting: a visited node is re-pointed at its grandparent -- with atomicMin (ATOMIC: other threads
// hook roots at the same time, a parent must never grow) or a plain store (no hooks are running: any ancestor is valid).
// x strictly decreases from one round to the next.
template <bool WG, bool ATOMIC>
__device__ __forceinline__ int vc_find(int* p, int x) {
  for (;;) {
    const int q = vc_load<WG>(p + x);
    if (q == x) return x;
    const int g = vc_load<WG>(p + q);
    if (g == q) return q;
    if (ATOMIC) atomicMin(p + x, g);
    else __hip_atomic_store(p + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = q;
  }
}

// Unite the sets of a and b.  A root once hooked never becomes a root again, and a round that does not end the loop was
// caused by another thread's hook, so the loop ends.
template <bool WG>
__device__ __forceinline__ void vc_union(int* p, int a, int b) {
  for (;;) {
    a = vc_find<WG, true>(p, a);
    b = vc_find<WG, true>(p, b);
    if (a == b) return;
    if (a < b) { const int s = a; a = b; b = s; }
    const int old = atomicMin(p + a, b);                    // a > b
    if (old == a) return;                                    // a was still a root: hooked
    a = old;                                                 // a had been hooked under `old`: p[a] = min(old, b), go on with the other
  }
}

// ---- brick pass ----
template <typename T>
__global__ __launch_bounds__(VC_BRICK_THREADS) void vc_brick_kernel(const T* __restrict__ grid, int64_t sN, int64_t sD, int64_t sH,
                                                                    int D, int H, int W, int nbh, int nbw, int64_t nb,
                                                                    int level, int by_value, int32_t* __restrict__ parent) {
  extern __shared__ int vc_lds[];
  int* par = vc_lds;
  int* key = vc_lds + BV;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t n = blockIdx.x / (unsigned)nb;                                   // nb * N fits 31 bits
  const int rem = (int)(blockIdx.x - n * nb);
  const int d0 = (rem / (nbw * nbh)) * BD, h0 = ((rem / nbw) % nbh) * BH, w0 = (rem % nbw) * BW;
  const int64_t S = (int64_t)D * H * W;
  const T* g = grid + n * sN;
  const int w = w0 + lane;

  constexpr int RPW = ROWS / VC_BRICK_WAVES;                                     // rows per wave: all loads in flight at once
  T val[RPW];
#pragma unroll
  for (int i = 0; i < RPW; ++i) {
    const int r = wave + i * VC_BRICK_WAVES;
    const int d = d0 + r / BH, h = h0 + r % BH;
    val[i] = 0;
    if (d < D && h < H && w < W) val[i] = g[d * sD + h * sH + w];
  }
  int any = 0;
#pragma unroll
  for (int i = 0; i < RPW; ++i) any |= vc_key(val[i], by_value);
  if (!__syncthreads_or(any)) {                                                  // a brick of background (workgroup-uniform)
    for (int r = wave; r < ROWS; r += VC_BRICK_WAVES) {
      const int d = d0 + r / BH, h = h0 + r % BH;
      if (d < D && h < H && w < W) parent[n * S + ((int64_t)d * H + h) * W + w] = -1;
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < RPW; ++i) {
    const int r = wave + i * VC_BRICK_WAVES;
    const int k = vc_key(val[i], by_value);
    const int kprev = __shfl_up(k, 1, 64);
    const bool start = k != 0 && (lane == 0 || kprev != k);
    const unsigned long long sm = __ballot(start);
    const int loc = r * BW + lane;
    int first = lane;
    if (k) first = 63 - __clzll((long long)(sm & (~0ull >> (63 - lane))));       // the run's start: at or below this lane
    par[loc] = r * BW + first;
    key[loc] = k;
  }
  __syncthreads();

  for (int r = wave; r < ROWS; r += VC_BRICK_WAVES) {
    const int dl = r / BH, hl = r % BH, loc = r * BW + lane;
    const int k = key[loc];
    const bool cont = lane > 0 && k && key[loc - 1] == k;                        // same run as lane - 1
#pragma unroll
    for (int o = 0; o < 4; ++o) {                                                // the rows before this one
      const int dd = o < 3 ? -1 : 0, dh = o < 3 ? o - 1 : -1;
      const int nr = (dd != 0) + (dh != 0);
      const int dl2 = dl + dd, hl2 = hl + dh;
      if (nr > level || dl2 < 0 || hl2 < 0 || hl2 >= BH) continue;               // wave-uniform
      const int nbi = (dl2 * BH + hl2) * BW + lane;
      const int k0 = key[nbi];
      const int km = lane > 0 ? key[nbi - 1] : 0, kp = lane < 63 ? key[nbi + 1] : 0;
      if (!k) continue;
      if (k0 == k) {
        // lane - 1 makes the same union when both voxels continue their runs; the diagonals are in k0's run
        if (!(cont && km == k)) vc_union<true>(par, loc, nbi);
      } else if (nr < level) {
        if (km == k) vc_union<true>(par, loc, nbi - 1);
        if (kp == k) vc_union<true>(par, loc, nbi + 1);
      }
    }
  }
  __syncthreads();

  for (int r = wave; r < ROWS; r += VC_BRICK_WAVES) {
    const int d = d0 + r / BH, h = h0 + r % BH, loc = r * BW + lane;
    if (d >= D || h >= H || w >= W) continue;
    int out = -1;
    if (key[loc]) {
      const int root = vc_find<true, true>(par, loc);
      const int rr = root / BW;
      out = (int)(((int64_t)(d0 + rr / BH) * H + (h0 + rr % BH)) * W + (w0 + root % BW));
    }
    parent[n * S + ((int64_t)d * H + h) * W + w] = out;
  }
}

// ---- seam pass ----
template <typename T>
__global__ __launch_bounds__(VC_THREADS) void vc_seam_kernel(const T* __restrict__ grid, int64_t sN, int64_t sD, int64_t sH, int D,
                                                             int H, int W, int nbd, int nbh, int nbw, int level, int by_value,
                                                             int32_t* parent) {
  const int64_t n = blockIdx.y;
  // the three counts and their sum are below D*H*W < 2^31 (the host checks the sum): 32-bit divisions
  const unsigned nd = (unsigned)(nbd - 1) * H * W, nh = (unsigned)D * (nbh - 1) * W, nw = (unsigned)D * H * (nbw - 1);
  unsigned i = blockIdx.x * VC_THREADS + threadIdx.x;
  if (i >= nd + nh + nw) return;
  int d, h, w;
  if (i < nd) {                                              // the planes d = k * BD
    const unsigned t = i / (unsigned)W;
    w = (int)(i - t * W);
    d = (int)(t / (unsigned)H);
    h = (int)(t - (unsigned)d * H);
    d = (d + 1) * BD;
  } else if (i < nd + nh) {                                  // the planes h = k * BH that are on no d plane
    i -= nd;
    const unsigned t = i / (unsigned)W, m = nbh - 1;
    w = (int)(i - t * W);
    d = (int)(t / m);
    h = ((int)(t - (unsigned)d * m) + 1) * BH;
    if (d % BD == 0 && d > 0) return;
  } else {                                                   // the planes w = k * BW that are on neither
    i -= nd + nh;
    const unsigned m = nbw - 1, t = i / m;
    w = ((int)(i - t * m) + 1) * BW;
    d = (int)(t / (unsigned)H);
    h = (int)(t - (unsigned)d * H);
    if ((d % BD == 0 && d > 0) || (h % BH == 0 && h > 0)) return;
  }
  const T* g = grid + n * sN;
  const int k = vc_key(g[d * sD + h * sH + w], by_value);
  if (!k) return;
  int32_t* p = parent + n * (int64_t)D * H * W;
  const int v = (int)(((int64_t)d * H + h) * W + w);
  const bool cont = w % BW != 0 && vc_key(g[d * sD + h * sH + w - 1], by_value) == k;
  for (int dd = -1; dd <= 1; ++dd)
    for (int dh = -1; dh <= 1; ++dh)
      for (int dw = -1; dw <= 1; ++dw) {
        const int nrm = (dd != 0) + (dh != 0) + (dw != 0);
        if (nrm == 0 || nrm > level) continue;
        const int e = d + dd, j = h + dh, x = w + dw;
        if (e < 0 || e >= D || j < 0 || j >= H || x < 0 || x >= W) continue;
        if (e / BD == d / BD && j / BH == h / BH && x / BW == w / BW) continue;    // same brick: the brick pass did it
        const T* row = g + e * sD + j * sH;
        if (vc_key(row[x], by_value) != k) continue;
        // the thread of w - 1 makes the same union when both voxels continue runs that lie in their bricks
        if (dw == 0 && cont && vc_key(row[x - 1], by_value) == k) continue;
        vc_union<false>(p, v, (int)(((int64_t)e * H + j) * W + x));
      }
}

// ---- flatten and number ----
__global__ __launch_bounds__(VC_CHUNK) void vc_flatten_kernel(int32_t* parent, int32_t* __restrict__ labels, int64_t S, int nchunks,
                                                              int32_t* __restrict__ counts) {
  const int64_t n = blockIdx.y;
  const int64_t v = (int64_t)blockIdx.x * VC_CHUNK + threadIdx.x;
  int32_t* p = parent + n * S;
  int flag = 0;
  if (v < S) {
    int l = 0;
    if (p[v] >= 0) {
      const int root = vc_find<false, false>(p, (int)v);
      l = root + 1;
      flag = root == (int)v;
    }
    labels[n * S + v] = l;
  }
  const int c = __syncthreads_count(flag);
  if (threadIdx.x == 0) counts[n * nchunks + blockIdx.x] = c;
}

// exclusive prefix sum over the VC_CHUNK threads of a workgroup; total: the sum.  wsum: VC_CHUNK / 64 ints of LDS.
__device__ __forceinline__ int vc_block_scan(int v, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();                                           // wsum of the round before has been read
  if (lane == 63) wsum[wid] = inc;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < VC_CHUNK / 64; ++i) {
    const int s = wsum[i];
    all += s;
    if (i < wid) before += s;
  }
  total = all;
  return before + inc - v;
}

__global__ __launch_bounds__(VC_CHUNK) void vc_scan_kernel(int32_t* counts, int nchunks, int64_t* __restrict__ num) {
  __shared__ int wsum[VC_CHUNK / 64];
  int32_t* c = counts + (int64_t)blockIdx.x * nchunks;
  int carry = 0;
  for (int base = 0; base < nchunks; base += VC_CHUNK) {     // block-uniform trip count
    const int i = base + threadIdx.x;
    const int v = i < nchunks ? c[i] : 0;
    int total;
    const int ex = vc_block_scan(v, wsum, total);
    if (i < nchunks) c[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) num[blockIdx.x] = carry;
}

__global__ __launch_bounds__(VC_CHUNK) void vc_number_kernel(int32_t* __restrict__ parent, const int32_t* __restrict__ labels, int64_t S,
                                                             int nchunks, const int32_t* __restrict__ counts,
                                                             const int64_t* __restrict__ num) {
  __shared__ int wsum[VC_CHUNK / 64];
  const int64_t n = blockIdx.y;
  const int32_t* c = counts + n * nchunks + blockIdx.x;
  const int64_t next = blockIdx.x + 1 < (unsigned)nchunks ? (int64_t)c[1] : num[n];
  if (next == c[0]) return;                                  // a chunk without a root (workgroup-uniform)
  const int64_t v = (int64_t)blockIdx.x * VC_CHUNK + threadIdx.x;
  const int flag = v < S && labels[n * S + v] == (int32_t)v + 1;
  int total;
  const int rank = vc_block_scan(flag, wsum, total);
  if (flag) parent[n * S + v] = c[0] + rank + 1;
}

__global__ __launch_bounds__(VC_THREADS) void vc_relabel_kernel(const int32_t* __restrict__ parent, int32_t* __restrict__ labels,
                                                                int64_t S) {
  const int64_t n = blockIdx.y;
  const int64_t v = (int64_t)blockIdx.x * VC_THREADS + threadIdx.x;
  if (v >= S) return;
  const int32_t l = labels[n * S + v];
  if (l) labels[n * S + v] = parent[n * S + l - 1];
}

// ---- stats ----
__global__ __launch_bounds__(VC_THREADS) void vc_stats_init_kernel(int64_t K, unsigned long long* __restrict__ size, int32_t* __restrict__ bbox,
                                                                   unsigned long long* __restrict__ first) {
  const int64_t c = (int64_t)blockIdx.x * VC_THREADS + threadIdx.x;
  if (c >= K) return;
  size[c] = 0;
  first[c] = (unsigned long long)INT64_MAX;
#pragma unroll
  for (int i = 0; i < 6; ++i) bbox[6 * c + i] = i < 3 ? INT32_MAX : 0;
}

// A workgroup walks VC_STATS_ROUNDS x VC_THREADS consecutive voxels, lanes along the linear index.  The first lane of
// every stretch of equal labels within a row and a wave adds for the whole stretch -- into a small table in LDS when its
// slot (label mod VC_STATS_SLOTS) is free or already the label's, else straight into the outputs; the table is added to the
// outputs at the end.  A large component would otherwise send every one of its runs to the same few addresses.  Integer
// atomics throughout, so the result does not depend on the order.
constexpr int VC_STATS_ROUNDS = 16, VC_STATS_SLOTS = 32;

__device__ __forceinline__ void vc_stats_add(unsigned long long* size, int32_t* bbox, unsigned long long* first, int64_t c,
                                             unsigned len, unsigned v, const int* lo, const int* hi) {
  atomicAdd(size + c, (unsigned long long)len);
  atomicMin(first + c, (unsigned long long)v);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    atomicMin(bbox + 6 * c + i, lo[i]);
    atomicMax(bbox + 6 * c + 3 + i, hi[i]);
  }
}

__global__ __launch_bounds__(VC_THREADS) void vc_stats_kernel(const int32_t* __restrict__ labels, int H, int W, int64_t S,
                                                              const int64_t* __restrict__ offsets, unsigned long long* __restrict__ size,
                                                              int32_t* __restrict__ bbox, unsigned long long* __restrict__ first) {
  __shared__ int tkey[VC_STATS_SLOTS], tlo[VC_STATS_SLOTS][3], thi[VC_STATS_SLOTS][3];
  __shared__ unsigned tsize[VC_STATS_SLOTS], tfirst[VC_STATS_SLOTS];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < VC_STATS_SLOTS) {
    tkey[tid] = 0;
    tsize[tid] = 0;
    tfirst[tid] = 0xffffffffu;
#pragma unroll
    for (int i = 0; i < 3; ++i) { tlo[tid][i] = INT32_MAX; thi[tid][i] = 0; }
  }
  __syncthreads();
  const int64_t n = blockIdx.y;
  const int64_t c0 = offsets[n], kn = offsets[n + 1] - c0;
  const int64_t base = (int64_t)blockIdx.x * (VC_STATS_ROUNDS * VC_THREADS);
  for (int it = 0; it < VC_STATS_ROUNDS; ++it) {             // fixed trip count: every lane takes part in the ballots
    const int64_t v = base + it * VC_THREADS + tid;          // < S + 4096 <= 2^31 + 4095: 32-bit divisions
    int l = v < S ? labels[n * S + v] : 0;
    if (l < 0 || l > kn) l = 0;                              // not a label of this grid: never index outside the outputs
    const unsigned row = (unsigned)v / (unsigned)W;
    const int w = (int)((unsigned)v - row * (unsigned)W);
    const int lprev = __shfl_up(l, 1, 64);
    const bool start = l != 0 && (lane == 0 || lprev != l || w == 0);
    const unsigned long long sm = __ballot(start), fg = __ballot(l != 0);
    if (start) {
      const unsigned long long m = lane < 63 ? (sm | ~fg) & (~0ull << (lane + 1)) : 0ull;
      const int len = (m ? __ffsll((long long)m) - 1 : 64) - lane;
      const int d = (int)(row / (unsigned)H), h = (int)(row - (unsigned)d * (unsigned)H);
      const int lo[3] = {d, h, w}, hi[3] = {d + 1, h + 1, w + len};
      const int slot = l & (VC_STATS_SLOTS - 1);
      const int old = atomicCAS(&tkey[slot], 0, l);
      if (old == 0 || old == l) {
        atomicAdd(&tsize[slot], (unsigned)len);
        atomicMin(&tfirst[slot], (unsigned)v);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          atomicMin(&tlo[slot][i], lo[i]);
          atomicMax(&thi[slot][i], hi[i]);
        }
      } else {
        vc_stats_add(size, bbox, first, c0 + l - 1, (unsigned)len, (unsigned)v, lo, hi);
      }
    }
  }
  __syncthreads();
  if (tid < VC_STATS_SLOTS && tkey[tid])
    vc_stats_add(size, bbox, first, c0 + tkey[tid] - 1, tsize[tid], tfirst[tid], tlo[tid], thi[tid]);
}

template <typename T>
__global__ __launch_bounds__(VC_THREADS) void vc_stats_value_kernel(const T* __restrict__ grid, int64_t sN, int64_t sD, int64_t sH, int N,
                                                                    int H, int W, const int64_t* __restrict__ offsets, int64_t K,
                                                                    const unsigned long long* __restrict__ first, int32_t* __restrict__ value) {
  const int64_t c = (int64_t)blockIdx.x * VC_THREADS + threadIdx.x;
  if (c >= K) return;
  int lo = 0, hi = N;                                        // the grid n with offsets[n] <= c < offsets[n + 1]
  for (int it = 0; it < 32; ++it) {                          // fixed trip count >= log2(N)
    const int mid = (lo + hi) >> 1;
    if (hi - lo > 1) { if (offsets[mid] <= c) lo = mid; else hi = mid; }
  }
  const unsigned long long f = first[c];
  if (f == (unsigned long long)INT64_MAX) { value[c] = 0; return; }
  const int64_t v = (int64_t)f;
  const int w = (int)(v % W);
  const int64_t t = v / W;
  value[c] = (int32_t)grid[lo * sN + (t / H) * sD + (t % H) * sH + w];
}

inline int64_t vc_chunks(int64_t S) { return (S + VC_CHUNK - 1) / VC_CHUNK; }
inline size_t vc_align(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" int crn_voxel_components_bricks(int32_t* out3) {
  if (!out3) return CRN_EINVAL;
  out3[0] = BD; out3[1] = BH; out3[2] = BW;
  return CRN_OK;
}

extern "C" size_t crn_voxel_components_workspace_bytes(int N, int D, int H, int W) {
  if (N < 1 || D < 1 || H < 1 || W < 1) return 0;
  const int64_t S = (int64_t)D * H * W;
  return vc_align((size_t)N * S * 4) + vc_align((size_t)N * vc_chunks(S) * 4);
}

extern "C" int crn_voxel_components(const void* grid, const int64_t* strides, int dtype, int N, int D, int H, int W, int connectivity,
                                    int by_value, void* workspace, size_t workspace_bytes, int32_t* labels, int64_t* num_components,
                                    crnStream stream) {
  if (!vc_args_ok(grid, strides, dtype, N, D, H, W, connectivity, labels, num_components) || N > 65535 || !workspace) return CRN_EINVAL;
  if (workspace_bytes < crn_voxel_components_workspace_bytes(N, D, H, W)) return CRN_ENOMEM;
  const int nbd = crn_cdiv(D, BD), nbh = crn_cdiv(H, BH), nbw = crn_cdiv(W, BW);
  const int64_t nb = (int64_t)nbd * nbh * nbw, S = (int64_t)D * H * W;
  if (nb * N > INT32_MAX) return CRN_EINVAL;
  CRN_ENTRY(stream);
  hipStream_t st = (hipStream_t)stream;
  const int level = vc_level(connectivity);
  const int nchunks = (int)vc_chunks(S);
  int32_t* parent = (int32_t*)workspace;
  int32_t* counts = (int32_t*)((char*)workspace + vc_align((size_t)N * S * 4));
  const int64_t sN = strides[0], sD = strides[1], sH = strides[2];
  const int64_t seam = (int64_t)(nbd - 1) * H * W + (int64_t)D * (nbh - 1) * W + (int64_t)D * H * (nbw - 1);
  if (seam > INT32_MAX) return CRN_EINVAL;                   // (always below D*H*W: the seam kernel's 32-bit index)
  int rc;
#define CRN_VC(T)                                                                                                              \
  do {                                                                                                                         \
    rc = crn_launch(vc_brick_kernel<T>, dim3((unsigned)(nb * N)), dim3(VC_BRICK_THREADS), 2 * BV * sizeof(int), st,            \
                    (const T*)grid, sN, sD, sH, D, H, W, nbh, nbw, nb, level, by_value, parent);                               \
    if (rc != CRN_OK) return rc;                                                                                               \
    if (seam > 0)                                                                                                              \
      hipLaunchKernelGGL(vc_seam_kernel<T>, dim3((unsigned)crn_cdiv(seam, VC_THREADS), N), dim3(VC_THREADS), 0, st,            \
                         (const T*)grid, sN, sD, sH, D, H, W, nbd, nbh, nbw, level, by_value, parent);                         \
  } while (0)
  if (dtype == VC_U8) CRN_VC(uint8_t); else CRN_VC(int32_t);
#undef CRN_VC
  CRN_CHECK_LAUNCH();
  hipLaunchKernelGGL(vc_flatten_kernel, dim3(nchunks, N), dim3(VC_CHUNK), 0, st, parent, labels, S, nchunks, counts);
  hipLaunchKernelGGL(vc_scan_kernel, dim3(N), dim3(VC_CHUNK), 0, st, counts, nchunks, num_components);
  hipLaunchKernelGGL(vc_number_kernel, dim3(nchunks, N), dim3(VC_CHUNK), 0, st, parent, (const int32_t*)labels, S, nchunks,
                     (const int32_t*)counts, (const int64_t*)num_components);
  hipLaunchKernelGGL(vc_relabel_kernel, dim3((unsigned)crn_cdiv(S, VC_THREADS), N), dim3(VC_THREADS), 0, st, (const int32_t*)parent,
                     labels, S);
  CRN_CHECK_LAUNCH();
  return CRN_OK;
}

extern "C" int crn_component_stats(const int32_t* labels, const void* grid, const int64_t* strides, int dtype, int N, int D, int H,
                                   int W, const int64_t* offsets, int64_t K, int64_t* size, int32_t* bbox, int64_t* first,
                                   int32_t* value, crnStream stream) {
  if (!vc_stats_args_ok(labels, grid, strides, dtype, N, D, H, W, offsets, K, size, bbox, first, value) || N > 65535) return CRN_EINVAL;
  if (K > (int64_t)INT32_MAX * VC_THREADS) return CRN_EINVAL;
  CRN_ENTRY(stream);
  if (K == 0) return CRN_OK;
  hipStream_t st = (hipStream_t)stream;
  const int64_t S = (int64_t)D * H * W;
  unsigned long long* usize = reinterpret_cast<unsigned long long*>(size);
  unsigned long long* ufirst = reinterpret_cast<unsigned long long*>(first);
  const dim3 kgrid((unsigned)crn_cdiv(K, VC_THREADS));
  hipLaunchKernelGGL(vc_stats_init_kernel, kgrid, dim3(VC_THREADS), 0, st, K, usize, bbox, ufirst);
  hipLaunchKernelGGL(vc_stats_kernel, dim3((unsigned)crn_cdiv(S, VC_STATS_ROUNDS * VC_THREADS), N), dim3(VC_THREADS), 0, st, labels, H, W, S, offsets, usize,
                     bbox, ufirst);
  if (grid) {
    if (dtype == VC_U8)
      hipLaunchKernelGGL(vc_stats_value_kernel<uint8_t>, kgrid, dim3(VC_THREADS), 0, st, (const uint8_t*)grid, strides[0], strides[1],
                         strides[2], N, H, W, offsets, K, (const unsigned long long*)ufirst, value);
    else
      hipLaunchKernelGGL(vc_stats_value_kernel<int32_t>, kgrid, dim3(VC_THREADS), 0, st, (const int32_t*)grid, strides[0], strides[1],
                         strides[2], N, H, W, offsets, K, (const unsigned long long*)ufirst, value);
  }
  CRN_CHECK_LAUNCH();
  return CRN_OK;
}
