// Marching cubes on gfx950 (corenet_amd.visualization; reference: MarchingCubesArtifact, visualization/artifacts.py:202-289,
// which runs skimage.measure.marching_cubes on the host).  Contract: include/corenet_hip.h and DESIGN section 13.
//
// Cells are taken in raster order per object, CPB = 1024 cells per workgroup (256 threads x 4 cells, cell = base +
// i * 256 + lane, so a wave's loads are contiguous along w); a workgroup never spans two objects.
//   count       classify every cell (8 corner loads, neighbours through L1 / L2), count its triangles and the crossing
//               edges it owns (the three at its minimum corner); one (vertices, faces) pair per workgroup
//   reduce      sums of 1024 workgroup pairs
//   scan        one workgroup: exclusive 64-bit scan of those sums, 1024 per round, ceil(S / 1024) rounds
//   distribute  exclusive offset of every workgroup pair = scanned super-block sum + in-block scan
//   sizes       counts[n] = offsets of object n + 1 minus those of object n
//   -- the caller reads counts (the one synchronisation) and sizes the outputs --
//   apply       per chunk of objects: object-local vertex offset of every cell that owns a crossing edge -> workspace
//   emit        per chunk: owned vertices (position, normal, optional matrix), then the cell's faces; the vertex id of an
//               edge owned by another cell = that cell's offset from `apply` + the crossing edges it owns on lower axes
// apply and emit workgroups whose count was zero leave at once (most of a near-binary grid).
// Offsets between workgroups are int64; object-local vertex ids are int32 (CRN_MC_MAX_OBJECT_CELLS).  No atomics: every
// output position follows from the scans, so two runs and the host twin (marching_cubes_cpu.cpp) give the same arrays.
#include "crn_common.h"
#define CRN_MC_TABLE_QUAL static __constant__
#include "mc_tables.h"
#include "marching_cubes_common.h"

namespace {

constexpr int MC_THREADS = 256;
constexpr int MC_PER_THREAD = 4;
constexpr int MC_CPB = MC_THREADS * MC_PER_THREAD;     // cells per workgroup
constexpr int SCAN_THREADS = 1024;
constexpr int64_t MC_CHUNK_CELLS = (int64_t)1 << 26;   // apply / emit: objects per chunk so that the vertex-offset
                                                        // workspace stays <= 256 MiB (one int32 per cell)

struct McLayout {
  int64_t cells;       // per object
  int bpo;             // workgroups per object
  int64_t nb;          // workgroups in all
  int64_t ns;          // super-blocks (1024 workgroups each)
  int chunk;           // objects per apply / emit chunk
  size_t o_bsum, o_ssum, o_boff, o_voff, bytes;
};

McLayout mc_layout(int N, int D, int H, int W) {
  McLayout L;
  L.cells = (int64_t)(D + 1) * (H + 1) * (W + 1);
  L.bpo = (int)((L.cells + MC_CPB - 1) / MC_CPB);
  L.nb = (int64_t)N * L.bpo;
  L.ns = (L.nb + SCAN_THREADS - 1) / SCAN_THREADS;
  int64_t c = MC_CHUNK_CELLS / L.cells;
  L.chunk = (int)(c < 1 ? 1 : (c > N ? N : c));
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  L.o_bsum = 0;                                                   // int32 [nb][2]
  L.o_ssum = al(L.o_bsum + (size_t)L.nb * 8);                     // int64 [ns][2] + total [2]
  L.o_boff = al(L.o_ssum + (size_t)(L.ns + 1) * 16);              // int64 [nb][2]
  L.o_voff = al(L.o_boff + (size_t)L.nb * 16);                    // int32 [chunk * cells]
  L.bytes = al(L.o_voff + (size_t)L.chunk * L.cells * 4);
  return L;
}

__device__ __forceinline__ void cell_coords(int64_t cell, int W, int H, int& z, int& y, int& x) {
  const int64_t row = cell / (W + 1);
  x = (int)(cell - row * (W + 1));
  z = (int)(row / (H + 1));
  y = (int)(row - (int64_t)z * (H + 1));
}

__device__ __forceinline__ int cell_case(const crnMcGrid& g, const float* obj, int z, int y, int x) {
  int cs = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) cs |= mc_inside(mc_at(g, obj, z + (c >> 2), y + ((c >> 1) & 1), x + (c & 1)), g.level) << c;
  return cs;
}

// exclusive scan over the block (blockDim.x == NT threads) in thread order; `total` gets the block sum
template <int NT, typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* lds, T& total) {
  const int tid = threadIdx.x;
  lds[tid] = v;
  __syncthreads();
  for (int off = 1; off < NT; off <<= 1) {
    const T a = tid >= off ? lds[tid - off] : (T)0;
    __syncthreads();
    lds[tid] += a;
    __syncthreads();
  }
  const T incl = lds[tid];
  total = lds[NT - 1];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(MC_THREADS) void mc_count_kernel(crnMcGrid g, int bpo, int64_t cells, int32_t* __restrict__ bsum) {
  __shared__ int32_t lds[MC_THREADS];
  const int n = blockIdx.x / bpo, b = blockIdx.x - n * bpo;
  const float* obj = g.p + n * g.sN;
  int32_t packed = 0;                                   // vertices | faces << 16 (<= 3072 | 5120 << 16)
#pragma unroll
  for (int i = 0; i < MC_PER_THREAD; ++i) {
    const int64_t cell = (int64_t)b * MC_CPB + i * MC_THREADS + threadIdx.x;
    if (cell >= cells) break;
    int z, y, x;
    cell_coords(cell, g.W, g.H, z, y, x);
    const int cs = cell_case(g, obj, z, y, x);
    if (cs != 0 && cs != 255) packed += mc_popc3(mc_case_owned_bits(cs)) | ((int32_t)crn_mc_num_tri[cs] << 16);
  }
  int32_t total;
  block_exclusive_scan<MC_THREADS>(packed, lds, total);
  if (threadIdx.x == 0) {
    bsum[2 * (int64_t)blockIdx.x] = total & 0xffff;
    bsum[2 * (int64_t)blockIdx.x + 1] = total >> 16;
  }
}

__global__ __launch_bounds__(SCAN_THREADS) void mc_reduce_kernel(const int32_t* __restrict__ bsum, int64_t nb,
                                                                  int64_t* __restrict__ ssum) {
  __shared__ int64_t lds[SCAN_THREADS];
  const int64_t i = (int64_t)blockIdx.x * SCAN_THREADS + threadIdx.x;
  int64_t tv, tt;
  block_exclusive_scan<SCAN_THREADS>(i < nb ? (int64_t)bsum[2 * i] : (int64_t)0, lds, tv);
  block_exclusive_scan<SCAN_THREADS>(i < nb ? (int64_t)bsum[2 * i + 1] : (int64_t)0, lds, tt);
  if (threadIdx.x == 0) { ssum[2 * blockIdx.x] = tv; ssum[2 * blockIdx.x + 1] = tt; }
}

// one workgroup; ssum[ns][2] -> exclusive offsets in place, ssum[ns] = totals
__global__ __launch_bounds__(SCAN_THREADS) void mc_scan_kernel(int64_t* __restrict__ ssum, int64_t ns) {
  __shared__ int64_t lds[SCAN_THREADS];
  int64_t cv = 0, ct = 0;
  const int64_t rounds = (ns + SCAN_THREADS - 1) / SCAN_THREADS;
  for (int64_t r = 0; r < rounds; ++r) {
    const int64_t i = r * SCAN_THREADS + threadIdx.x;
    const int64_t v = i < ns ? ssum[2 * i] : 0, t = i < ns ? ssum[2 * i + 1] : 0;
    int64_t tv, tt;
    const int64_t ev = block_exclusive_scan<SCAN_THREADS>(v, lds, tv);
    const int64_t et = block_exclusive_scan<SCAN_THREADS>(t, lds, tt);
    if (i < ns) { ssum[2 * i] = cv + ev; ssum[2 * i + 1] = ct + et; }
    cv += tv;
    ct += tt;
  }
  if (threadIdx.x == 0) { ssum[2 * ns] = cv; ssum[2 * ns + 1] = ct; }
}

__global__ __launch_bounds__(SCAN_THREADS) void mc_distribute_kernel(const int32_t* __restrict__ bsum, const int64_t* __restrict__ soff,
                                                                      int64_t nb, int64_t* __restrict__ boff) {
  __shared__ int64_t lds[SCAN_THREADS];
  const int64_t i = (int64_t)blockIdx.x * SCAN_THREADS + threadIdx.x;
  int64_t tv, tt;
  const int64_t ev = block_exclusive_scan<SCAN_THREADS>(i < nb ? (int64_t)bsum[2 * i] : (int64_t)0, lds, tv);
  const int64_t et = block_exclusive_scan<SCAN_THREADS>(i < nb ? (int64_t)bsum[2 * i + 1] : (int64_t)0, lds, tt);
  if (i < nb) {
    boff[2 * i] = soff[2 * blockIdx.x] + ev;
    boff[2 * i + 1] = soff[2 * blockIdx.x + 1] + et;
  }
}

__global__ void mc_sizes_kernel(const int64_t* __restrict__ boff, const int64_t* __restrict__ total, int N, int bpo,
                                int64_t* __restrict__ counts) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const int64_t* a = boff + 2 * (int64_t)n * bpo;
  const int64_t* e = n + 1 < N ? boff + 2 * (int64_t)(n + 1) * bpo : total;
  counts[2 * n] = e[0] - a[0];
  counts[2 * n + 1] = e[1] - a[1];
}

// object-local vertex offset of every cell of objects [n0, n0 + chunk) that owns a crossing edge
__global__ __launch_bounds__(MC_THREADS) void mc_apply_kernel(crnMcGrid g, int n0, int bpo, int64_t cells,
                                                              const int32_t* __restrict__ bsum, const int64_t* __restrict__ boff,
                                                              int32_t* __restrict__ voff) {
  __shared__ int32_t lds[MC_THREADS];
  const int nl = blockIdx.x / bpo, b = blockIdx.x - nl * bpo, n = n0 + nl;
  const int64_t blk = (int64_t)n * bpo + b;
  if (bsum[2 * blk] == 0) return;                                 // no crossing edge in the workgroup (uniform)
  const float* obj = g.p + n * g.sN;
  int32_t carry = (int32_t)(boff[2 * blk] - boff[2 * (int64_t)n * bpo]);
#pragma unroll
  for (int i = 0; i < MC_PER_THREAD; ++i) {
    const int64_t cell = (int64_t)b * MC_CPB + i * MC_THREADS + threadIdx.x;
    int nv = 0;
    if (cell < cells) {
      int z, y, x;
      cell_coords(cell, g.W, g.H, z, y, x);
      nv = mc_popc3(mc_owned_bits(g, obj, z, y, x));
    }
    int32_t tot;
    const int32_t ex = block_exclusive_scan<MC_THREADS>(nv, lds, tot);
    if (nv) voff[(int64_t)nl * cells + cell] = carry + ex;
    carry += tot;
  }
}

__global__ __launch_bounds__(MC_THREADS) void mc_emit_kernel(crnMcGrid g, int n0, int bpo, int64_t cells,
                                                             const int32_t* __restrict__ bsum, const int64_t* __restrict__ boff,
                                                             const int32_t* __restrict__ voff,
                                                             const float* __restrict__ matrices, float* __restrict__ vertices,
                                                             float* __restrict__ normals, int32_t* __restrict__ faces) {
  __shared__ int32_t lds[MC_THREADS];
  const int nl = blockIdx.x / bpo, b = blockIdx.x - nl * bpo, n = n0 + nl;
  const int64_t blk = (int64_t)n * bpo + b;
  if (bsum[2 * blk + 1] == 0) return;                             // no face in the workgroup (uniform): most of a grid
  const float* obj = g.p + n * g.sN;
  const int64_t vobj = boff[2 * (int64_t)n * bpo];                // first vertex of the object
  int64_t tnext = boff[2 * blk + 1];                              // next face of the workgroup
  const int32_t* vo = voff + (int64_t)nl * cells;
  const float* m = matrices ? matrices + 16 * (int64_t)n : nullptr;
  const int CW = g.W + 1, CP = (g.W + 1) * (g.H + 1);
  for (int i = 0; i < MC_PER_THREAD; ++i) {
    const int64_t cell = (int64_t)b * MC_CPB + i * MC_THREADS + threadIdx.x;
    int cs = 0, z = 0, y = 0, x = 0;
    if (cell < cells) {
      cell_coords(cell, g.W, g.H, z, y, x);
      cs = cell_case(g, obj, z, y, x);
    }
    const int nt = (cs == 0 || cs == 255) ? 0 : crn_mc_num_tri[cs];
    int32_t tot;
    const int32_t ex = block_exclusive_scan<MC_THREADS>(nt, lds, tot);
    if (nt) {
      const int own = mc_case_owned_bits(cs);
      if (own) {
        int64_t v = vobj + vo[cell];
        for (int a = 0; a < 3; ++a) {
          if (!((own >> a) & 1)) continue;
          float pos[3], nrm[3];
          mc_vertex(g, obj, z, y, x, a, pos, nrm);
          if (m) mc_transform(m, pos, nrm);
          for (int c = 0; c < 3; ++c) { vertices[3 * v + c] = pos[c]; normals[3 * v + c] = nrm[c]; }
          ++v;
        }
      }
      int64_t f = tnext + ex;
      for (int k = 0; k < nt; ++k, ++f) {
        for (int j = 0; j < 3; ++j) {
          int a, dx, dy, dz;
          mc_edge(crn_mc_tri[cs][3 * k + j], a, dx, dy, dz);
          const int oz = z + dz, oy = y + dy, ox = x + dx;
          int32_t idx = vo[cell + dz * (int64_t)CP + dy * CW + dx];
          if (a >= 1) idx += mc_crosses(g, obj, oz, oy, ox, 0);
          if (a == 2) idx += mc_crosses(g, obj, oz, oy, ox, 1);
          faces[3 * f + j] = idx;
        }
      }
    }
    tnext += tot;
  }
}

__global__ void box_filter_kernel(const float* __restrict__ in, int64_t sN, int64_t sD, int64_t sH, int64_t sW,
                                  float* __restrict__ out, int N, int D, int H, int W, int axis, int k, float scale) {
  const int64_t total = (int64_t)N * D * H * W;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = i;
    const int w = (int)(r % W); r /= W;
    const int h = (int)(r % H); r /= H;
    const int d = (int)(r % D);
    const int n = (int)(r / D);
    const int64_t base = n * sN + d * sD + h * sH + w * sW;
    float v;
    if (axis == 0) v = mc_box_tap(in, base - w * sW, sW, w, W, k, scale);
    else if (axis == 1) v = mc_box_tap(in, base - h * sH, sH, h, H, k, scale);
    else v = mc_box_tap(in, base - d * sD, sD, d, D, k, scale);
    out[i] = v;
  }
}

bool mc_args_ok(const float* grid, const int64_t* strides, int N, int D, int H, int W, float level) {
  return grid && strides && N >= 1 && D >= 1 && H >= 1 && W >= 1 && level > 0.f && strides[3] == 1 &&
         (int64_t)(D + 1) * (H + 1) * (W + 1) <= CRN_MC_MAX_OBJECT_CELLS;
}

}  // namespace

extern "C" size_t crn_marching_cubes_workspace_bytes(int N, int D, int H, int W) {
  if (N < 1 || D < 1 || H < 1 || W < 1) return 0;
  return mc_layout(N, D, H, W).bytes;
}

extern "C" int crn_marching_cubes_count(const float* grid, const int64_t* strides, int N, int D, int H, int W, float level,
                                        void* workspace, size_t workspace_bytes, int64_t* counts, crnStream s) {
  if (!mc_args_ok(grid, strides, N, D, H, W, level) || !workspace || !counts) return CRN_EINVAL;
  const McLayout L = mc_layout(N, D, H, W);
  if (workspace_bytes < L.bytes || L.nb >= ((int64_t)1 << 31)) return CRN_EINVAL;
  char* ws = (char*)workspace;
  int32_t* bsum = (int32_t*)(ws + L.o_bsum);
  int64_t* ssum = (int64_t*)(ws + L.o_ssum);
  int64_t* boff = (int64_t*)(ws + L.o_boff);
  const crnMcGrid g{grid, strides[0], strides[1], strides[2], D, H, W, level};
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(mc_count_kernel, dim3((unsigned)L.nb), dim3(MC_THREADS), 0, st, g, L.bpo, L.cells, bsum);
  CRN_CHECK_LAUNCH();
  hipLaunchKernelGGL(mc_reduce_kernel, dim3((unsigned)L.ns), dim3(SCAN_THREADS), 0, st, bsum, L.nb, ssum);
  CRN_CHECK_LAUNCH();
  hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, ssum, L.ns);
  CRN_CHECK_LAUNCH();
  hipLaunchKernelGGL(mc_distribute_kernel, dim3((unsigned)L.ns), dim3(SCAN_THREADS), 0, st, bsum, ssum, L.nb, boff);
  CRN_CHECK_LAUNCH();
  hipLaunchKernelGGL(mc_sizes_kernel, dim3((N + 255) / 256), dim3(256), 0, st, boff, ssum + 2 * L.ns, N, L.bpo, counts);
  CRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int crn_marching_cubes_emit(const float* grid, const int64_t* strides, int N, int D, int H, int W, float level,
                                       const float* matrices, void* workspace, size_t workspace_bytes, float* vertices,
                                       float* normals, int32_t* faces, crnStream s) {
  if (!mc_args_ok(grid, strides, N, D, H, W, level) || !workspace) return CRN_EINVAL;
  const McLayout L = mc_layout(N, D, H, W);
  if (workspace_bytes < L.bytes) return CRN_EINVAL;
  char* ws = (char*)workspace;
  const int32_t* bsum = (const int32_t*)(ws + L.o_bsum);
  const int64_t* boff = (const int64_t*)(ws + L.o_boff);
  int32_t* voff = (int32_t*)(ws + L.o_voff);
  const crnMcGrid g{grid, strides[0], strides[1], strides[2], D, H, W, level};
  hipStream_t st = (hipStream_t)s;
  for (int n0 = 0; n0 < N; n0 += L.chunk) {
    const int nc = N - n0 < L.chunk ? N - n0 : L.chunk;
    const unsigned blocks = (unsigned)((int64_t)nc * L.bpo);
    hipLaunchKernelGGL(mc_apply_kernel, dim3(blocks), dim3(MC_THREADS), 0, st, g, n0, L.bpo, L.cells, bsum, boff, voff);
    CRN_CHECK_LAUNCH();
    hipLaunchKernelGGL(mc_emit_kernel, dim3(blocks), dim3(MC_THREADS), 0, st, g, n0, L.bpo, L.cells, bsum,
                       boff, (const int32_t*)voff, matrices, vertices, normals, faces);
    CRN_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int crn_box_filter(const float* in, const int64_t* strides, float* out, int N, int D, int H, int W, int k,
                              void* workspace, size_t workspace_bytes, crnStream s) {
  if (!in || !strides || !out || N < 1 || D < 1 || H < 1 || W < 1 || k < 1) return CRN_EINVAL;
  const int64_t total = (int64_t)N * D * H * W;
  if (!workspace || workspace_bytes < (size_t)total * 4) return CRN_EINVAL;
  float* tmp = (float*)workspace;
  const float inv = 1.0f / (float)((int64_t)k * k * k);
  hipStream_t st = (hipStream_t)s;
  const int64_t want = (total + 255) / 256;
  const unsigned blocks = (unsigned)(want < 65536 ? want : 65536);
  const int64_t cD = (int64_t)H * W, cN = (int64_t)D * H * W;
  hipLaunchKernelGGL(box_filter_kernel, dim3(blocks), dim3(256), 0, st, in, strides[0], strides[1], strides[2], strides[3],
                     out, N, D, H, W, 0, k, 1.f);
  CRN_CHECK_LAUNCH();
  hipLaunchKernelGGL(box_filter_kernel, dim3(blocks), dim3(256), 0, st, (const float*)out, cN, cD, (int64_t)W, (int64_t)1,
                     tmp, N, D, H, W, 1, k, 1.f);
  CRN_CHECK_LAUNCH();
  hipLaunchKernelGGL(box_filter_kernel, dim3(blocks), dim3(256), 0, st, (const float*)tmp, cN, cD, (int64_t)W, (int64_t)1,
                     out, N, D, H, W, 2, k, inv);
  CRN_CHECK_LAUNCH();
  return 0;
}
