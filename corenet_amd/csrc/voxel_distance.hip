// Batched exact squared Euclidean distance transform on gfx950 (corenet_amd.voxel_distance).  Contract:
// include/corenet_hip.h and DESIGN section 18; host twin: voxel_distance_cpu.cpp (identical d2 and index: both follow
// the same separable recurrence, and every minimum is an exact integer minimum with a fixed tie rule).
//
// Three passes, none of which waits for another workgroup; every loop has a fixed or data-bounded trip count:
//   row      a wave owns a row (lanes along w, one 64-voxel word at a time).  A sweep upwards takes the ballot of the
//            target predicate and gives every lane the nearest target at or below it (count-leading-zeros on the masked
//            word, the last target of the words before as carry); a sweep downwards does the same from above and keeps
//            the nearer one, ties to the lower w.
//   line     out[i] = min_j g[j] + (i - j)^2 along h, then along d.  A workgroup stages a tile of L x 64 columns in LDS
//            (64 neighbouring columns, so a wave reads row j without a bank conflict), lists the rows j that hold a
//            target in any of its columns, and every wave keeps VD_R outputs i per lane in registers while it walks the
//            list: j is wave-uniform, so (i - j)^2 is scalar and a pair costs one add and one min.  Rows that are
//            NO_TARGET in all 64 columns are never visited, and the walk goes outwards from the wave's outputs and ends
//            once the squared step alone reaches the largest value any of them still holds (g >= 0).  In place for d2:
//            the tile is complete before anything is written.  Three forms of the inner step:
//              values   no index wanted.
//              packed   (value << bits(L)) | j in one word, a plain min then implements "ties to the lower j".
//              select   compare and select, where the packed word does not fit.
//            A NO_TARGET element is staged as a sentinel above every real candidate, small enough that sentinel + (i - j)^2
//            cannot wrap: nothing is added to 2^31 - 1 in signed arithmetic, and no lane needs a branch.
//   global   lines longer than VD_CAP: a thread per output reads the line from a copy in the workspace.
#include "crn_common.h"
#include "voxel_distance_common.h"

namespace {

constexpr int VD_R = CRN_VD_LINE_R;              // outputs per lane of the line pass
constexpr int VD_CAP = CRN_VD_LINE_CAP;          // longest line staged in LDS
constexpr int VD_PACK_BITS = CRN_VD_PACK_BITS;   // packed form iff (bound + 1) << bits(L) <= 2^VD_PACK_BITS
constexpr int VD_ROW_WAVES = 4;
constexpr int VD_MAX_WAVES = 16;
constexpr int VD_GLOBAL_WAVES = 4;
constexpr int VD_STAGE = 8;                      // rows a wave loads before it stores them into the tile
constexpr int VD_REFRESH = 16;                   // rows of a sweep before the first refresh of its bound
constexpr unsigned NT = (unsigned)CRN_VD_NO_TARGET;
static_assert((size_t)VD_CAP * 64 * 4 + (size_t)VD_CAP * 8 + 16 <= 160 * 1024, "the tile, the flags and the list fit the CU's LDS");

// ---- row pass ----
template <typename T>
__global__ __launch_bounds__(VD_ROW_WAVES * 64) void vd_row_kernel(const T* __restrict__ grid, int64_t sN, int64_t sD, int64_t sH, int D,
                                                                   int H, int W, int64_t rows, int mode, int32_t* d2, int32_t* idx) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * VD_ROW_WAVES + (threadIdx.x >> 6);
  if (r >= rows) return;                                     // wave-uniform
  const int64_t n = r / ((int64_t)D * H);
  const int rem = (int)(r - n * D * H);
  const int d = rem / H, h = rem - d * H;
  const T* g = grid + n * sN;
  int32_t* o2 = d2 + r * W;
  int last = -1;                                             // the last target of the words below
  for (int base = 0; base < W; base += 64) {
    const int w = base + lane;
    const bool tg = w < W && vd_target(g, sD, sH, D, H, W, d, h, w, mode);
    const unsigned long long m = __ballot(tg);
    const unsigned long long mm = m & (~0ull >> (63 - lane));
    const int lo = mm ? base + 63 - __clzll((long long)mm) : last;
    if (w < W) o2[w] = lo;                                   // read back by this lane in the sweep downwards
    if (m) last = base + 63 - __clzll((long long)m);
  }
  int next = -1;                                             // the first target of the words above
  for (int base = ((W - 1) / 64) * 64; base >= 0; base -= 64) {
    const int w = base + lane;
    const int lo = w < W ? o2[w] : -1;
    const unsigned long long m = __ballot(w < W && lo == w); // lo == w: the voxel is a target itself
    const unsigned long long mm = m & (~0ull << lane);
    const int hi = mm ? base + __ffsll((long long)mm) - 1 : next;
    int win = lo;
    if (hi >= 0 && (lo < 0 || hi - w < w - lo)) win = hi;    // a tie goes to the lower w
    if (w < W) {
      o2[w] = win < 0 ? (int32_t)NT : (win - w) * (win - w);
      if (idx) idx[r * W + w] = win;
    }
    if (m) next = base + __ffsll((long long)m) - 1;
  }
}

// ---- line pass ----
// Column c of grid n starts at n * S + (c / inner) * outer + c % inner and its elements are ls apart: the h pass has
// inner = W, outer = H * W, ls = W (columns (d, w)); the d pass inner = ncols = H * W, ls = H * W.
struct VdLine {
  int64_t S, ls, outer;
  int L, inner, ncols, groups;
};

__device__ __forceinline__ int64_t vd_column(const VdLine& a, unsigned block, int lane, bool& ok) {
  const unsigned n = block / (unsigned)a.groups, grp = block - n * (unsigned)a.groups;
  const int c = (int)grp * 64 + lane;
  ok = c < a.ncols;
  const int q = ok ? c / a.inner : 0;
  return (int64_t)n * a.S + (int64_t)q * a.outer + (ok ? c - q * a.inner : 0);
}

enum { VD_VALUES = 0, VD_PACKED = 1, VD_SELECT = 2 };

// One row j against the VD_R outputs i0 .. i0 + VD_R - 1 of a lane.  j is wave-uniform, so the squares are scalar.
// DOWN: the rows come in descending order and a tie goes to the new, lower j (SELECT; the packed word orders ties itself).
template <int MODE, bool DOWN>
__device__ __forceinline__ void vd_visit(unsigned v, int j, int i0, int bits, unsigned (&best)[VD_R], int (&bj)[VD_R]) {
  const int s = i0 - j;
#pragma unroll
  for (int r = 0; r < VD_R; ++r) {
    const unsigned sq = (unsigned)((s + r) * (s + r));
    if (MODE == VD_SELECT) {
      const unsigned cand = v + sq;
      if (DOWN ? cand <= best[r] : cand < best[r]) { best[r] = cand; bj[r] = j; }
    } else {
      const unsigned cand = v + (sq << bits);
      best[r] = cand < best[r] ? cand : best[r];
    }
  }
}

// The largest value among the outputs of the wave that will be written (wave-uniform).
template <int MODE>
__device__ __forceinline__ unsigned vd_bound(const unsigned (&best)[VD_R], int i0, int L, bool ok, int bits) {
  unsigned m = 0;
#pragma unroll
  for (int r = 0; r < VD_R; ++r) {
    const unsigned val = MODE == VD_PACKED ? best[r] >> bits : best[r];
    if (i0 + r < L && val > m) m = val;
  }
  if (!ok) m = 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned x = (unsigned)__shfl_xor((int)m, o, 64);
    m = x > m ? x : m;
  }
  return (unsigned)__builtin_amdgcn_readfirstlane((int)m);
}

template <int MODE>
__global__ __launch_bounds__(VD_MAX_WAVES * 64) void vd_line_kernel(int32_t* d2, const int32_t* __restrict__ idx_in, int32_t* __restrict__ idx_out,
                                                                    VdLine a, int bits, unsigned sentinel) {
  extern __shared__ unsigned vd_lds[];
  const int L = a.L;
  unsigned* tile = vd_lds;                                   // [L][64]
  int* flag = (int*)(tile + (size_t)L * 64);                 // [L] row j holds a target in one of the 64 columns
  int* list = flag + L;                                      // [L] those rows, ascending
  int* cnt = list + L;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  bool ok;
  const int64_t base = vd_column(a, blockIdx.x, lane, ok);

  for (int j0 = wave; j0 < L; j0 += nw * VD_STAGE) {         // VD_STAGE loads in flight per lane
    unsigned g[VD_STAGE];
#pragma unroll
    for (int u = 0; u < VD_STAGE; ++u) {
      const int j = j0 + u * nw;
      g[u] = ok && j < L ? (unsigned)d2[base + j * a.ls] : NT;
    }
#pragma unroll
    for (int u = 0; u < VD_STAGE; ++u) {
      const int j = j0 + u * nw;
      if (j >= L) break;                                     // wave-uniform
      const bool has = g[u] != NT;
      const unsigned x = has ? g[u] : sentinel;
      tile[j * 64 + lane] = MODE == VD_PACKED ? (x << bits) | (unsigned)j : x;
      const unsigned long long any = __ballot(has);
      if (lane == 0) flag[j] = any != 0;
    }
  }
  __syncthreads();
  if (wave == 0) {
    int total = 0;
    for (int b = 0; b < L; b += 64) {                        // fixed trip count
      const int j = b + lane;
      const bool f = j < L && flag[j];
      const unsigned long long m = __ballot(f);
      if (f) list[total + __popcll(m & ((1ull << lane) - 1))] = j;
      total += __popcll(m);
    }
    if (lane == 0) *cnt = total;
  }
  __syncthreads();
  const int nact = *cnt;

  const int chunks = (L + VD_R - 1) / VD_R;
  for (int ch = wave; ch < chunks; ch += nw) {
    const int i0 = ch * VD_R;
    unsigned best[VD_R];
    int bj[VD_R];                                            // SELECT only (dead otherwise)
#pragma unroll
    for (int r = 0; r < VD_R; ++r) {
      best[r] = 0xffffffffu;
      if (MODE == VD_SELECT) bj[r] = -1;
    }
    // the first listed row at or above the chunk (wave-uniform)
    int p = 0;
    for (int b = 0; b < nact; b += 64) {                     // fixed trip count
      const int k = b + lane;
      p += __popcll(__ballot(k < nact && list[k] < i0));
    }
    // Two sweeps away from the chunk, each ended early: bound is the largest value any output of the wave still holds
    // (refreshed after VD_REFRESH rows of a sweep, then after twice as many, ...; a stale one is only larger), and a row
    // whose squared step alone reaches it cannot win.  Upwards a tie loses to the lower j already seen, so >= ends the sweep; downwards a tie would win, so only >.
    // The list is read 64 entries at a time, one per lane, and row k comes out of that register with a readlane; the
    // tile row of the next step is fetched before the arithmetic of this one.
    int mine = 0, blk = -1;
    auto row_at = [&](int k) {                               // k is wave-uniform
      if ((k >> 6) != blk) {
        blk = k >> 6;
        const int q = (blk << 6) + lane;
        mine = q < nact ? list[q] : 0;
      }
      return __builtin_amdgcn_readlane(mine, k & 63);
    };
    unsigned bound = 0xffffffffu;
    if (p < nact) {
      int jn = row_at(p);
      unsigned vn = tile[jn * 64 + lane];
      for (int k = p, n = 1, next = VD_REFRESH;; ++k, ++n) { // data-bounded: at most nact - p rounds
        const int j = jn;
        const unsigned v = vn;
        const bool more = k + 1 < nact;
        if (more) {
          jn = row_at(k + 1);
          vn = tile[jn * 64 + lane];
        }
        const int gap = j - (i0 + VD_R - 1);
        if (gap > 0 && (unsigned)(gap * gap) >= bound) break;
        vd_visit<MODE, false>(v, j, i0, bits, best, bj);
        if (!more) break;
        if (n == next) { bound = vd_bound<MODE>(best, i0, L, ok, bits); next *= 2; }
      }
    }
    if (p > 0) {
      bound = vd_bound<MODE>(best, i0, L, ok, bits);
      int jn = row_at(p - 1);
      unsigned vn = tile[jn * 64 + lane];
      for (int k = p - 1, n = 1, next = VD_REFRESH;; --k, ++n) {             // at most p rounds
        const int j = jn;
        const unsigned v = vn;
        const bool more = k > 0;
        if (more) {
          jn = row_at(k - 1);
          vn = tile[jn * 64 + lane];
        }
        const int gap = i0 - j;
        if ((unsigned)(gap * gap) > bound) break;
        vd_visit<MODE, true>(v, j, i0, bits, best, bj);
        if (!more) break;
        if (n == next) { bound = vd_bound<MODE>(best, i0, L, ok, bits); next *= 2; }
      }
    }
#pragma unroll
    for (int r = 0; r < VD_R; ++r) {
      const int i = i0 + r;
      if (i >= L || !ok) continue;
      const unsigned val = MODE == VD_PACKED ? best[r] >> bits : best[r];
      const bool none = val >= sentinel;
      d2[base + i * a.ls] = none ? (int32_t)NT : (int32_t)val;
      if (MODE != VD_VALUES) {
        const int j = MODE == VD_PACKED ? (int)(best[r] & ((1u << bits) - 1)) : bj[r];
        idx_out[base + i * a.ls] = none ? -1 : (int32_t)(j * a.ls) + idx_in[base + j * a.ls];   // the winner keeps row j's index
      }
    }
  }
}

// Lines longer than VD_CAP: one thread per output, the line read from src (a copy of d2) in global memory.
template <bool INDEX>
__global__ __launch_bounds__(VD_GLOBAL_WAVES * 64) void vd_line_global_kernel(const int32_t* __restrict__ src, int32_t* __restrict__ d2,
                                                                              const int32_t* __restrict__ idx_in, int32_t* __restrict__ idx_out,
                                                                              VdLine a, int ichunks) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned col_block = blockIdx.x / (unsigned)ichunks;
  const int i = (int)(blockIdx.x - col_block * (unsigned)ichunks) * VD_GLOBAL_WAVES + wave;
  bool ok;
  const int64_t base = vd_column(a, col_block, lane, ok);
  if (i >= a.L || !ok) return;
  unsigned best = NT;
  int bj = -1;
  for (int j = 0; j < a.L; ++j) {                            // fixed trip count
    const unsigned g = (unsigned)src[base + j * a.ls];
    const unsigned cand = g + (unsigned)((i - j) * (i - j)); // g == NT: cand >= NT, never below best
    if (cand < best) { best = cand; bj = j; }
  }
  d2[base + i * a.ls] = (int32_t)best;
  if (INDEX) idx_out[base + i * a.ls] = bj < 0 ? -1 : (int32_t)(bj * a.ls) + idx_in[base + bj * a.ls];
}

inline size_t vd_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline int vd_bits(int L) {
  int b = 0;
  while ((1 << b) < L) ++b;
  return b;
}

}  // namespace

extern "C" int crn_voxel_distance_tiles(int32_t* out3) {
  if (!out3) return CRN_EINVAL;
  out3[0] = VD_R; out3[1] = VD_CAP; out3[2] = VD_PACK_BITS;
  return CRN_OK;
}

extern "C" size_t crn_voxel_distance_workspace_bytes(int N, int D, int H, int W, int want_index) {
  if (N < 1 || D < 1 || H < 1 || W < 1) return 0;
  const size_t one = vd_align((size_t)N * D * H * W * 4);
  return (want_index ? one : 0) + ((H > VD_CAP || D > VD_CAP) ? one : 0);
}

extern "C" int crn_voxel_distance(const void* grid, const int64_t* strides, int dtype, int N, int D, int H, int W, int mode,
                                  void* workspace, size_t workspace_bytes, int32_t* d2, int32_t* index, crnStream stream) {
  if (!vd_args_ok(grid, strides, dtype, N, D, H, W, mode, d2)) return CRN_EINVAL;
  if (N == 0) return CRN_OK;
  const size_t need = crn_voxel_distance_workspace_bytes(N, D, H, W, index != nullptr);
  if (need && !workspace) return CRN_EINVAL;
  if (workspace_bytes < need) return CRN_ENOMEM;
  const int64_t S = (int64_t)D * H * W, rows = (int64_t)N * D * H;
  const int64_t row_blocks = (rows + VD_ROW_WAVES - 1) / VD_ROW_WAVES;
  if (row_blocks > INT32_MAX) return CRN_EINVAL;
  // the launch sizes of the two line passes, checked before anything is queued
  struct Pass { int L; VdLine a; int64_t bound; };
  Pass passes[2];
  int np = 0;
  int64_t bound = (int64_t)(W - 1) * (W - 1);                 // the largest real value so far
  if (H > 1) {
    bound += (int64_t)(H - 1) * (H - 1);
    passes[np++] = {H, {S, W, (int64_t)H * W, H, W, D * W, 0}, bound};
  }
  if (D > 1) {
    bound += (int64_t)(D - 1) * (D - 1);
    passes[np++] = {D, {S, (int64_t)H * W, 0, D, H * W, H * W, 0}, bound};
  }
  for (int p = 0; p < np; ++p) {
    Pass& ps = passes[p];
    if ((int64_t)ps.a.ncols > INT32_MAX - 64) return CRN_EINVAL;
    ps.a.groups = (ps.a.ncols + 63) / 64;
    int64_t blocks = (int64_t)N * ps.a.groups;
    if (ps.L > VD_CAP) blocks *= (ps.L + VD_GLOBAL_WAVES - 1) / VD_GLOBAL_WAVES;
    if (blocks > INT32_MAX) return CRN_EINVAL;
  }
  CRN_ENTRY(stream);
  hipStream_t st = (hipStream_t)stream;
  const size_t one = vd_align((size_t)N * S * 4);
  int32_t* ws_idx = index ? (int32_t*)workspace : nullptr;
  int32_t* ws_d2 = (int32_t*)((char*)workspace + (index ? one : 0));     // used only by a global pass
  // the index lands in `index` after the last pass: every pass reads one buffer and writes the other
  int32_t* cur = index ? ((np & 1) ? ws_idx : index) : nullptr;
  if (dtype == VD_U8)
    hipLaunchKernelGGL(vd_row_kernel<uint8_t>, dim3((unsigned)row_blocks), dim3(VD_ROW_WAVES * 64), 0, st, (const uint8_t*)grid, strides[0],
                       strides[1], strides[2], D, H, W, rows, mode, d2, cur);
  else
    hipLaunchKernelGGL(vd_row_kernel<int32_t>, dim3((unsigned)row_blocks), dim3(VD_ROW_WAVES * 64), 0, st, (const int32_t*)grid, strides[0],
                       strides[1], strides[2], D, H, W, rows, mode, d2, cur);
  CRN_CHECK_LAUNCH();
  for (int p = 0; p < np; ++p) {
    const Pass& ps = passes[p];
    int32_t* nxt = index ? (cur == index ? ws_idx : index) : nullptr;
    const unsigned cols = (unsigned)((int64_t)N * ps.a.groups);
    if (ps.L > VD_CAP) {
      CRN_HIP(hipMemcpyAsync(ws_d2, d2, (size_t)N * S * 4, hipMemcpyDeviceToDevice, st));
      const int ichunks = (ps.L + VD_GLOBAL_WAVES - 1) / VD_GLOBAL_WAVES;
      if (index)
        hipLaunchKernelGGL(vd_line_global_kernel<true>, dim3(cols * (unsigned)ichunks), dim3(VD_GLOBAL_WAVES * 64), 0, st,
                           (const int32_t*)ws_d2, d2, (const int32_t*)cur, nxt, ps.a, ichunks);
      else
        hipLaunchKernelGGL(vd_line_global_kernel<false>, dim3(cols * (unsigned)ichunks), dim3(VD_GLOBAL_WAVES * 64), 0, st,
                           (const int32_t*)ws_d2, d2, (const int32_t*)nullptr, (int32_t*)nullptr, ps.a, ichunks);
      CRN_CHECK_LAUNCH();
    } else {
      const int chunks = (ps.L + VD_R - 1) / VD_R;
      const dim3 block((unsigned)(chunks < VD_MAX_WAVES ? chunks : VD_MAX_WAVES) * 64);
      const size_t lds = (size_t)ps.L * 64 * 4 + (size_t)ps.L * 8 + 16;
      const int bits = vd_bits(ps.L);
      int rc;
      if (!index)
        rc = crn_launch(vd_line_kernel<VD_VALUES>, dim3(cols), block, lds, st, d2, (const int32_t*)nullptr, (int32_t*)nullptr, ps.a, 0, NT);
      else if (((ps.bound + 1) << bits) <= ((int64_t)1 << VD_PACK_BITS))
        rc = crn_launch(vd_line_kernel<VD_PACKED>, dim3(cols), block, lds, st, d2, (const int32_t*)cur, nxt, ps.a, bits,
                        (unsigned)(ps.bound + 1));
      else
        rc = crn_launch(vd_line_kernel<VD_SELECT>, dim3(cols), block, lds, st, d2, (const int32_t*)cur, nxt, ps.a, 0, NT);
      if (rc != CRN_OK) return rc;
    }
    cur = nxt;
  }
  return CRN_OK;
}
