// Batched voxel visibility from an eye on gfx950 (corenet_amd.voxel_visibility).  Contract: include/corenet_hip.h and
// DESIGN section 19; host twin: voxel_visibility_cpu.cpp (identical occluded and first: both run the integer walk of
// voxel_visibility_common.h over one occupancy bit per voxel).
//
// Two passes, neither of which waits for another workgroup; every loop has a fixed or bounded trip count:
//   pack     a wave owns a row (lanes along w, one 64-voxel word at a time): the ballot of the occupancy predicate is the
//            fine word.  With a coarse map, lane 0 folds the word into one bit per 4 voxels (16 bricks along w) and ORs
//            the non-zero ones into the map, one bit per brick of 4^3 voxels: at most two atomics per occupied word.
//   walk     a workgroup owns VV_WG_WORDS consecutive 64-voxel words of one grid, a wave one word at a time, a lane one
//            voxel.  The lane runs vv_step until the walk reaches the eye or leaves the grid: at most D + H + W steps,
//            since every step moves one axis or more towards leaving.  The path does not depend on what it finds.
//              coarse   the workgroup first stages the grid's coarse map in LDS (one barrier, reached by every thread:
//                       nothing returns before it); a step tests the brick bit there and reads the fine word from global
//                       memory only inside an occupied brick.
//              flat     a step reads the fine word; no LDS and no barrier.
//            Without `first` a lane stops at its first hit; with it the lane walks on and keeps the latest hit, the
//            occupied voxel nearest the eye.  A wave leaves its word when all its lanes are done.
//            The eyes of up to VV_BATCH grids travel in the kernel arguments (blockIdx.y picks the grid), so nothing is
//            copied and a call is one walk launch per VV_BATCH grids.
#include "crn_common.h"
#include "voxel_visibility_common.h"

namespace {

constexpr int VV_PACK_WAVES = 4;
constexpr int VV_WALK_WAVES = 16;
constexpr int VV_WG_WORDS = CRN_VV_WG_WORDS;     // 64-voxel words a walk workgroup owns
constexpr int VV_BATCH = 64;                     // grids per walk launch (their eyes are kernel arguments)
constexpr int VV_CAP = CRN_VV_COARSE_CAP_BYTES;  // largest coarse map staged in LDS
static_assert(CRN_VV_BRICK == 4, "the fold of the pack pass and the shifts of the walk pass assume bricks of 4^3");
static_assert(2 * VV_CAP <= 160 * 1024, "two walk workgroups of 16 waves fit a CU's LDS");

struct VvEyes { int32_t e[VV_BATCH][3]; };

struct VvShape {
  int D, H, W, words;          // words: 64-bit words per row
  int Hc, Wc, cwords;          // bricks along h and w; 32-bit words of a grid's coarse map (a multiple of 4)
  int tasks;                   // D * H * words
  int64_t per_grid;            // fine words per grid
};

// ---- pack pass ----
template <typename T>
__global__ __launch_bounds__(VV_PACK_WAVES * 64) void vv_pack_kernel(const T* __restrict__ grid, int64_t sN, int64_t sD, int64_t sH, VvShape s,
                                                                     int64_t rows, uint64_t* __restrict__ fine, unsigned* coarse) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * VV_PACK_WAVES + (threadIdx.x >> 6);
  if (r >= rows) return;                                     // wave-uniform; the kernel has no barrier
  const int64_t n = r / ((int64_t)s.D * s.H);
  const int rem = (int)(r - n * s.D * s.H);
  const int z = rem / s.H, y = rem - z * s.H;
  const T* g = grid + n * sN + z * sD + y * sH;
  uint64_t* out = fine + r * s.words;                        // per_grid == D * H * words: rows of all grids are contiguous
  const int crow = ((z >> 2) * s.Hc + (y >> 2)) * s.Wc;
  for (int base = 0; base < s.W; base += 64) {               // fixed trip count
    const int w = base + lane;
    const bool occ = w < s.W && vv_occupied(g[w]);
    const unsigned long long m = __ballot(occ);
    if (lane == 0) out[base >> 6] = m;
    if (lane != 0 || !coarse || !m) continue;                // the lanes meet again at the loop's end, before the next ballot
    unsigned long long f = m | (m >> 1);                     // bit 4j of f: any of the voxels 4j .. 4j + 3
    f = (f | (f >> 2)) & 0x1111111111111111ull;
    f = (f | (f >> 3)) & 0x0303030303030303ull;              // squeeze the 16 bits together
    f = (f | (f >> 6)) & 0x000f000f000f000full;
    f = (f | (f >> 12)) & 0x000000ff000000ffull;
    f = (f | (f >> 24)) & 0xffffull;
    const int ci = crow + (base >> 2);                       // the brick bit of voxel `base`; bits beyond W are 0 in m
    unsigned* cw = coarse + n * s.cwords + (ci >> 5);
    const int sh = ci & 31;
    const unsigned lo = (unsigned)(f << sh), hi = sh > 16 ? (unsigned)(f >> (32 - sh)) : 0u;
    if (lo) atomicOr(cw, lo);
    if (hi) atomicOr(cw + 1, hi);                            // hi != 0 only for a brick that exists: inside the map
  }
}

// ---- walk pass ----
template <bool COARSE, bool FIRST>
__global__ __launch_bounds__(VV_WALK_WAVES * 64) void vv_walk_kernel(const uint64_t* __restrict__ fine, const unsigned* __restrict__ coarse,
                                                                     VvEyes eyes, VvShape s, uint8_t* __restrict__ occluded,
                                                                     int32_t* __restrict__ first) {
  extern __shared__ __attribute__((aligned(16))) unsigned vv_map[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int n = blockIdx.y;
  fine += n * s.per_grid;
  if (COARSE) {
    const uint4* src = (const uint4*)(coarse + (int64_t)n * s.cwords);
    for (int i = threadIdx.x; i < (s.cwords >> 2); i += blockDim.x) ((uint4*)vv_map)[i] = src[i];
    __syncthreads();                                         // every thread of the workgroup arrives: no return above
  }
  const int32_t eye[3] = {eyes.e[n][0], eyes.e[n][1], eyes.e[n][2]};
  const int64_t S = (int64_t)s.D * s.H * s.W;
  const int t0 = blockIdx.x * VV_WG_WORDS;
  const int t1 = t0 + VV_WG_WORDS < s.tasks ? t0 + VV_WG_WORDS : s.tasks;
  for (int task = t0 + wave; task < t1; task += nw) {        // wave-uniform, at most VV_WG_WORDS / nw rounds
    const int row = task / s.words, wd = task - row * s.words;
    const int z = row / s.H, y = row - z * s.H, x = wd * 64 + lane;
    if (x >= s.W) continue;
    VvWalk k = vv_start(x, y, z, eye);
    int hrow = -1, hx = 0;                                   // the latest hit: its row z * H + y (-1: none) and its x
    while (vv_step(k, s.D, s.H, s.W)) {                      // at most D + H + W rounds
      const int px = k.pos[0], py = k.pos[1], pz = k.pos[2];
      const int prow = __mul24(pz, s.H) + py;                // below 2^22; the word index below 2^27
      bool look = true;
      if (COARSE) {
        const int ci = __mul24(__mul24(pz >> 2, s.Hc) + (py >> 2), s.Wc) + (px >> 2);
        look = (vv_map[ci >> 5] >> (ci & 31)) & 1;
      }
      unsigned hit = 0;
      if (look) hit = (unsigned)(fine[__mul24(prow, s.words) + (px >> 6)] >> (px & 63)) & 1u;
      if (FIRST) {
        // One back edge, and the hit selected with a mask, not a branch: with a `continue` for an empty brick or a branch
        // on the hit the compiler splits the loop there, and a lane in an occupied brick then waits until the rest of
        // its wave has finished walking before it goes on (measured: 3 x the time on the sparse label grids).
        const int keep = (int)hit - 1;                       // all ones without a hit
        hrow = (hrow & keep) | (prow & ~keep);
        hx = (hx & keep) | (px & ~keep);
      } else if (hit) {
        hrow = prow;
        break;
      }
    }
    const int64_t v = n * S + (int64_t)row * s.W + x;
    occluded[v] = hrow >= 0;
    if (FIRST) first[v] = hrow < 0 ? -1 : hrow * s.W + hx;
  }
}

inline size_t vv_align(size_t b) { return (b + 255) & ~(size_t)255; }

inline VvShape vv_shape(int D, int H, int W) {
  VvShape s;
  s.D = D; s.H = H; s.W = W;
  s.words = vv_words64(W);
  s.Hc = (H + 3) >> 2; s.Wc = (W + 3) >> 2;
  const int64_t bricks = (int64_t)((D + 3) >> 2) * s.Hc * s.Wc;            // at most 512^3 = 2^27
  s.cwords = (int)(((bricks + 31) / 32 + 3) & ~(int64_t)3);
  s.tasks = D * H * s.words;                                               // at most 2048 * 2048 * 32 = 2^27
  s.per_grid = (int64_t)s.tasks;
  return s;
}
inline bool vv_coarse_fits(const VvShape& s) { return (size_t)s.cwords * 4 <= (size_t)VV_CAP; }

}  // namespace

extern "C" int crn_voxel_visibility_tiles(int32_t* out3) {
  if (!out3) return CRN_EINVAL;
  out3[0] = CRN_VV_BRICK; out3[1] = VV_CAP; out3[2] = VV_WG_WORDS;
  return CRN_OK;
}

extern "C" size_t crn_voxel_visibility_workspace_bytes(int N, int D, int H, int W) {
  if (N < 1 || D < 1 || H < 1 || W < 1 || D > CRN_VV_MAX_EXTENT || H > CRN_VV_MAX_EXTENT || W > CRN_VV_MAX_EXTENT) return 0;
  const VvShape s = vv_shape(D, H, W);
  return vv_align((size_t)N * s.per_grid * 8) + (vv_coarse_fits(s) ? vv_align((size_t)N * s.cwords * 4) : 0);
}

extern "C" int crn_voxel_visibility(const void* grid, const int64_t* strides, int dtype, int N, int D, int H, int W,
                                    const int32_t* eye_q, int flags, void* workspace, size_t workspace_bytes, uint8_t* occluded,
                                    int32_t* first, crnStream stream) {
  if (!vv_args_ok(grid, strides, dtype, N, D, H, W, eye_q, flags, CRN_VV_FLAT, occluded)) return CRN_EINVAL;
  if (N == 0) return CRN_OK;
  if (!workspace) return CRN_EINVAL;
  if (workspace_bytes < crn_voxel_visibility_workspace_bytes(N, D, H, W)) return CRN_ENOMEM;
  const VvShape s = vv_shape(D, H, W);
  const bool use_coarse = vv_coarse_fits(s) && !(flags & CRN_VV_FLAT);
  const int64_t rows = (int64_t)N * D * H, S = (int64_t)D * H * W;
  const int64_t row_blocks = (rows + VV_PACK_WAVES - 1) / VV_PACK_WAVES;
  if (row_blocks > INT32_MAX) return CRN_EINVAL;
  CRN_ENTRY(stream);
  hipStream_t st = (hipStream_t)stream;
  uint64_t* fine = (uint64_t*)workspace;
  unsigned* coarse = use_coarse ? (unsigned*)((char*)workspace + vv_align((size_t)N * s.per_grid * 8)) : nullptr;
  if (coarse) CRN_HIP(hipMemsetAsync(coarse, 0, (size_t)N * s.cwords * 4, st));
  if (dtype == VV_U8)
    hipLaunchKernelGGL(vv_pack_kernel<uint8_t>, dim3((unsigned)row_blocks), dim3(VV_PACK_WAVES * 64), 0, st, (const uint8_t*)grid, strides[0],
                       strides[1], strides[2], s, rows, fine, coarse);
  else
    hipLaunchKernelGGL(vv_pack_kernel<int32_t>, dim3((unsigned)row_blocks), dim3(VV_PACK_WAVES * 64), 0, st, (const int32_t*)grid, strides[0],
                       strides[1], strides[2], s, rows, fine, coarse);
  CRN_CHECK_LAUNCH();
  const int waves = s.tasks < VV_WALK_WAVES ? s.tasks : VV_WALK_WAVES;
  const unsigned blocks = (unsigned)((s.tasks + VV_WG_WORDS - 1) / VV_WG_WORDS);
  const size_t lds = use_coarse ? (size_t)s.cwords * 4 : 0;
  for (int n0 = 0; n0 < N; n0 += VV_BATCH) {
    const int nb = N - n0 < VV_BATCH ? N - n0 : VV_BATCH;
    VvEyes eyes = {};
    for (int i = 0; i < nb * 3; ++i) eyes.e[i / 3][i % 3] = eye_q[(int64_t)n0 * 3 + i];
    const uint64_t* f = fine + n0 * s.per_grid;
    const unsigned* c = coarse ? coarse + (int64_t)n0 * s.cwords : nullptr;
    uint8_t* occ = occluded + n0 * S;
    int32_t* fst = first ? first + n0 * S : nullptr;
    const dim3 g(blocks, (unsigned)nb), b((unsigned)waves * 64);
    int rc;
    if (use_coarse)
      rc = first ? crn_launch(vv_walk_kernel<true, true>, g, b, lds, st, f, c, eyes, s, occ, fst)
                 : crn_launch(vv_walk_kernel<true, false>, g, b, lds, st, f, c, eyes, s, occ, fst);
    else
      rc = first ? crn_launch(vv_walk_kernel<false, true>, g, b, lds, st, f, c, eyes, s, occ, fst)
                 : crn_launch(vv_walk_kernel<false, false>, g, b, lds, st, f, c, eyes, s, occ, fst);
    if (rc != CRN_OK) return rc;
  }
  return CRN_OK;
}
