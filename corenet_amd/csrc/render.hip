// Batched triangle renderer and voxel-face extraction on gfx950 (corenet_amd.visualization.render; reference:
// scene_renderer.py / voxel_renderer.py, which draw through OpenGL).  Contract: include/corenet_hip.h, the arithmetic:
// render_common.h, DESIGN section 14.
//
// Renderer, I images of H x W, 16 x 16 pixel tiles:
//   setup   one thread per (image, triangle of its range): transform, cull, homogeneous edges, z plane, pixel box ->
//           a 64-byte record; one counter atomic per overlapped tile of the image
//   scan    one workgroup: exclusive 64-bit scan of the per-(image, tile) counts (rounds of 1024)
//   -- the caller reads the total (the one synchronisation) and sizes the tile lists --
//   fill    same threads as setup: every overlapped tile gets the record id at offset + (atomic decrement of its count)
//   raster  one workgroup per (image, tile), one pixel per lane: walk the tile's list, keep the winning (z, record id)
//           in registers, then shade the winner once and store uint8 RGB.  With textures a second instantiation runs,
//           which multiplies the winner's diffuse colour by one bilinear fetch (4 x 32-bit RGBA8 loads) before shading.
// The order inside a list is whatever the atomics made it; the winner is min z then max record id (GL LEQUAL in
// submission order), a total order, so the image does not depend on it: two runs and the host twin agree bit for bit.
//
// Voxel faces, N grids, 1024 voxels per workgroup (256 threads x 4, voxel = base + i * 256 + lane):
//   count    exposed-face triangles per workgroup (+ optional box of the transformed occupied centres: wave min / max,
//            then one order-preserving int atomic per wave and component -- min / max commute, so it is exact)
//   scan     one workgroup, as above;  sizes: counts[n]
//   emit     the workgroup's voxels again, in-block exclusive scans in voxel order, triangles at the scanned offsets.
#include "crn_common.h"
#include "render_common.h"

namespace {

constexpr int RD_T = CRN_RENDER_TILE;
constexpr int RD_THREADS = RD_T * RD_T;
constexpr int SCAN_THREADS = 1024;
constexpr int VX_THREADS = 256;
constexpr int VX_PER_THREAD = 4;
constexpr int VX_BLOCK = VX_THREADS * VX_PER_THREAD;

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

// one workgroup: out[i] = sum in[0..i), out[n] = total
__global__ __launch_bounds__(SCAN_THREADS) void rd_scan_kernel(const int32_t* __restrict__ in, int64_t n,
                                                               int64_t* __restrict__ out) {
  __shared__ int64_t lds[SCAN_THREADS];
  int64_t base = 0;
  const int64_t rounds = (n + SCAN_THREADS - 1) / SCAN_THREADS;
  for (int64_t r = 0; r < rounds; ++r) {
    const int64_t i = r * SCAN_THREADS + threadIdx.x;
    int64_t tot;
    const int64_t e = block_exclusive_scan<SCAN_THREADS>(i < n ? (int64_t)in[i] : (int64_t)0, lds, tot);
    if (i < n) out[i] = base + e;
    base += tot;
  }
  if (threadIdx.x == 0) out[n] = base;
}

__device__ __forceinline__ void load_rec(const float* __restrict__ recs, int64_t id, crnRdRec& r) {
  const float4* p = reinterpret_cast<const float4*>(recs + 16 * id);
  const float4 a = p[0], b = p[1], c = p[2], d = p[3];
  r.e[0][0] = a.x; r.e[0][1] = a.y; r.e[0][2] = a.z; r.e[1][0] = a.w;
  r.e[1][1] = b.x; r.e[1][2] = b.y; r.e[2][0] = b.z; r.e[2][1] = b.w;
  r.e[2][2] = c.x; r.z[0] = c.y; r.z[1] = c.z; r.z[2] = c.w;
  r.box[0] = __float_as_int(d.x); r.box[1] = __float_as_int(d.y);
  r.box[2] = __float_as_int(d.z); r.box[3] = __float_as_int(d.w);
}

__device__ __forceinline__ void load_box(const float* __restrict__ recs, int64_t id, int32_t box[4]) {
  const float4 d = reinterpret_cast<const float4*>(recs + 16 * id)[3];
  box[0] = __float_as_int(d.x); box[1] = __float_as_int(d.y); box[2] = __float_as_int(d.z); box[3] = __float_as_int(d.w);
}

__global__ __launch_bounds__(256) void rd_setup_kernel(const float* __restrict__ tri, const crnRenderImage* __restrict__ imgs,
                                                       int H, int W, float* __restrict__ recs, int32_t* __restrict__ counts) {
  const int i = blockIdx.y;
  const crnRenderImage& im = imgs[i];
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= im.t1 - im.t0) return;
  crnRdRec r;
  const bool vis = rd_setup(im, H, W, tri + 9 * (int64_t)(im.t0 + k), r);
  float4* p = reinterpret_cast<float4*>(recs + 16 * (int64_t)(im.inst0 + k));
  p[0] = make_float4(r.e[0][0], r.e[0][1], r.e[0][2], r.e[1][0]);
  p[1] = make_float4(r.e[1][1], r.e[1][2], r.e[2][0], r.e[2][1]);
  p[2] = make_float4(r.e[2][2], r.z[0], r.z[1], r.z[2]);
  p[3] = make_float4(__int_as_float(r.box[0]), __int_as_float(r.box[1]), __int_as_float(r.box[2]), __int_as_float(r.box[3]));
  if (!vis) return;
  const int tx = (W + RD_T - 1) / RD_T, ntiles = tx * ((H + RD_T - 1) / RD_T);
  int32_t* c = counts + (int64_t)i * ntiles;
  for (int y = r.box[1] / RD_T; y <= r.box[3] / RD_T; ++y)
    for (int x = r.box[0] / RD_T; x <= r.box[2] / RD_T; ++x) atomicAdd(c + y * tx + x, 1);
}

__global__ __launch_bounds__(256) void rd_fill_kernel(const crnRenderImage* __restrict__ imgs, int H, int W,
                                                      const float* __restrict__ recs, int32_t* __restrict__ counts,
                                                      const int64_t* __restrict__ offs, int32_t* __restrict__ list) {
  const int i = blockIdx.y;
  const crnRenderImage& im = imgs[i];
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= im.t1 - im.t0) return;
  const int32_t id = im.inst0 + k;
  int32_t box[4];
  load_box(recs, id, box);
  if (box[0] > box[2] || box[1] > box[3]) return;
  const int tx = (W + RD_T - 1) / RD_T, ntiles = tx * ((H + RD_T - 1) / RD_T);
  const int64_t b0 = (int64_t)i * ntiles;
  for (int y = box[1] / RD_T; y <= box[3] / RD_T; ++y)
    for (int x = box[0] / RD_T; x <= box[2] / RD_T; ++x) {
      const int64_t b = b0 + y * tx + x;
      list[offs[b] + atomicSub(counts + b, 1) - 1] = id;
    }
}

// One pixel per lane.  TEX only adds the fetch in front of rd_shade: the untextured instantiation is the kernel as it
// was, and only the winning fragment of a pixel samples.
template <bool TEX>
__device__ __forceinline__ void rd_raster_pixel(const float* __restrict__ tri, const float* __restrict__ nrm,
                                                const int32_t* __restrict__ mids, const float* __restrict__ mats, int M,
                                                const crnRenderImage* __restrict__ imgs, int H, int W,
                                                const float* __restrict__ recs, const int64_t* __restrict__ offs,
                                                const int32_t* __restrict__ list, uint8_t* __restrict__ out,
                                                const crnRdTex& tex) {
  const int i = blockIdx.y;
  const crnRenderImage& im = imgs[i];
  const int tx = (W + RD_T - 1) / RD_T, ntiles = tx * ((H + RD_T - 1) / RD_T);
  const int tile = blockIdx.x, ty = tile / tx;
  const int col = (tile - ty * tx) * RD_T + (threadIdx.x & (RD_T - 1)), row = ty * RD_T + threadIdx.x / RD_T;
  const int64_t b = (int64_t)i * ntiles + tile;
  const int64_t beg = offs[b], end = offs[b + 1];
  float bz = 0.f;
  int32_t bid = -1;
  for (int64_t q = beg; q < end; ++q) {
    const int32_t id = list[q];
    crnRdRec r;
    load_rec(recs, id, r);
    float E[3], z;
    if (rd_fragment(r, col, row, E, z) && rd_wins(z, id, bz, bid)) {
      bz = z;
      bid = id;
    }
  }
  if (col >= W || row >= H) return;
  uint8_t* o = out + (((int64_t)i * H + row) * W + col) * 3;
  if (bid < 0) {
    o[0] = rd_u8(im.clear[0]); o[1] = rd_u8(im.clear[1]); o[2] = rd_u8(im.clear[2]);
    return;
  }
  crnRdRec r;
  load_rec(recs, bid, r);
  float E[3], z;
  rd_fragment(r, col, row, E, z);
  const int64_t t = (int64_t)im.t0 + (bid - im.inst0);
  const int32_t m = mids[t];
  float p[9], n[9];
  for (int q = 0; q < 9; ++q) p[q] = tri[9 * t + q];
  if (im.normal_mode == 1)
    for (int q = 0; q < 9; ++q) n[q] = nrm[9 * t + q];
  else if (im.normal_mode == 2)
    for (int q = 0; q < 3; ++q) n[q] = nrm[9 * t + q];
  float mat[10];
  const bool has_mat = m >= 0 && m < M;
  if (has_mat)
    for (int q = 0; q < 10; ++q) mat[q] = mats[10 * (int64_t)m + q];
  if constexpr (TEX) {
    const int32_t layer = has_mat ? tex.ids[m] : -1;
    if (layer >= 0 && layer < tex.L) {
      float uv[6];
      if (tex.uv)
        for (int q = 0; q < 6; ++q) uv[q] = tex.uv[6 * t + q];
      rd_tex_diffuse(E, tex.uv ? uv : nullptr, tex.texels, tex.Ht, tex.Wt, layer, mat);
    }
  }
  uint8_t rgb[3];
  rd_shade(im, p, n, has_mat ? mat : nullptr, E, rgb);
  o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
}

__global__ __launch_bounds__(RD_THREADS) void rd_raster_kernel(const float* __restrict__ tri, const float* __restrict__ nrm,
                                                               const int32_t* __restrict__ mids, const float* __restrict__ mats,
                                                               int M, const crnRenderImage* __restrict__ imgs, int H, int W,
                                                               const float* __restrict__ recs, const int64_t* __restrict__ offs,
                                                               const int32_t* __restrict__ list, uint8_t* __restrict__ out) {
  rd_raster_pixel<false>(tri, nrm, mids, mats, M, imgs, H, W, recs, offs, list, out, crnRdTex{});
}

__global__ __launch_bounds__(RD_THREADS) void rd_raster_tex_kernel(
    const float* __restrict__ tri, const float* __restrict__ nrm, const int32_t* __restrict__ mids,
    const float* __restrict__ mats, int M, const crnRenderImage* __restrict__ imgs, int H, int W,
    const float* __restrict__ recs, const int64_t* __restrict__ offs, const int32_t* __restrict__ list,
    uint8_t* __restrict__ out, crnRdTex tex) {
  rd_raster_pixel<true>(tri, nrm, mids, mats, M, imgs, H, W, recs, offs, list, out, tex);
}

// ---------------- geometry buffers ----------------
// The raster pass again, without shading: same winner rule, then the winner's triangle index, barycentrics, clip w and
// z_ndc instead of a colour.  The tile's list is walked in chunks staged in LDS: the workgroup copies RD_CHUNK records
// at a time, one 16-byte load per thread (thread = record * 4 + quarter), and every lane tests the chunk from there (all
// lanes read one address: a broadcast).  The colour kernels' walk, every lane loading each listed record itself, was
// measured beside it and was slower; the winner is decided by the key (z, record id) alone, so the
// outputs do not depend on the walk.
constexpr int RD_CHUNK = RD_THREADS / 4;

struct crnRdGeomOut {
  int32_t* tri;     // [I][H][W] or NULL
  float* bary;      // [I][H][W][3] or NULL
  float* depth;     // [I][H][W] or NULL
  float* z;         // [I][H][W] or NULL
};

__global__ __launch_bounds__(RD_THREADS) void rd_raster_geometry_kernel(
    const float* __restrict__ tri, const crnRenderImage* __restrict__ imgs, int H, int W, const float* __restrict__ recs,
    const int64_t* __restrict__ offs, const int32_t* __restrict__ list, crnRdGeomOut out) {
  __shared__ float4 s_rec[RD_CHUNK * 4];
  __shared__ int32_t s_id[RD_CHUNK];
  const int i = blockIdx.y;
  const crnRenderImage& im = imgs[i];
  const int tx = (W + RD_T - 1) / RD_T, ntiles = tx * ((H + RD_T - 1) / RD_T);
  const int tile = blockIdx.x, ty = tile / tx;
  const int col = (tile - ty * tx) * RD_T + (threadIdx.x & (RD_T - 1)), row = ty * RD_T + threadIdx.x / RD_T;
  const int64_t b = (int64_t)i * ntiles + tile;
  const int64_t beg = offs[b], end = offs[b + 1];
  const int j = threadIdx.x >> 2, quarter = threadIdx.x & 3;
  float bz = 0.f;
  int32_t bid = -1;
  for (int64_t base = beg; base < end; base += RD_CHUNK) {          // uniform bounds: every thread meets every barrier
    const int n = (int)(end - base < RD_CHUNK ? end - base : RD_CHUNK);
    if (base != beg) __syncthreads();                               // the previous chunk has been tested by every lane
    if (j < n) {
      const int32_t id = list[base + j];
      s_rec[threadIdx.x] = reinterpret_cast<const float4*>(recs + 16 * (int64_t)id)[quarter];
      if (quarter == 0) s_id[j] = id;
    }
    __syncthreads();
    for (int k = 0; k < n; ++k) {
      const int32_t id = s_id[k];
      crnRdRec r;
      load_rec(reinterpret_cast<const float*>(s_rec), k, r);
      float E[3], z;
      if (rd_fragment(r, col, row, E, z) && rd_wins(z, id, bz, bid)) {
        bz = z;
        bid = id;
      }
    }
  }
  if (col >= W || row >= H) return;
  const int64_t px = ((int64_t)i * H + row) * W + col;
  int32_t t = -1;
  float bary[3] = {0.f, 0.f, 0.f}, depth = INFINITY, z = INFINITY;
  if (bid >= 0) {
    crnRdRec r;
    load_rec(recs, bid, r);
    float E[3];
    rd_fragment(r, col, row, E, z);
    t = im.t0 + (bid - im.inst0);
    float p[9];
    for (int q = 0; q < 9; ++q) p[q] = tri[9 * (int64_t)t + q];
    rd_geometry(im, p, E, bary, depth);
  }
  if (out.tri) out.tri[px] = t;
  if (out.bary) {
    out.bary[3 * px] = bary[0]; out.bary[3 * px + 1] = bary[1]; out.bary[3 * px + 2] = bary[2];
  }
  if (out.depth) out.depth[px] = depth;
  if (out.z) out.z[px] = z;
}

// ---------------- voxel faces ----------------
struct VxLayout {
  int64_t vox;        // per grid
  int bpg;            // workgroups per grid
  int64_t nb;
  size_t o_bcnt, o_boff, o_keys, bytes;
};

VxLayout vx_layout(int N, int D, int H, int W) {
  VxLayout L;
  L.vox = (int64_t)D * H * W;
  L.bpg = (int)((L.vox + VX_BLOCK - 1) / VX_BLOCK);
  L.nb = (int64_t)N * L.bpg;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  L.o_bcnt = 0;                                          // int32 [nb]
  L.o_boff = al(L.o_bcnt + (size_t)L.nb * 4);            // int64 [nb + 1]
  L.o_keys = al(L.o_boff + (size_t)(L.nb + 1) * 8);      // int32 [N][6] box keys
  L.bytes = al(L.o_keys + (size_t)N * 24);
  return L;
}

__device__ __forceinline__ void vx_coords(int64_t v, int H, int W, int& z, int& y, int& x) {
  const int64_t row = v / W;
  x = (int)(v - row * W);
  z = (int)(row / H);
  y = (int)(row - (int64_t)z * H);
}

__global__ void vx_key_init_kernel(int32_t* keys, int N) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < 6 * N) keys[j] = (j % 6) < 3 ? INT32_MAX : INT32_MIN;
}

__global__ __launch_bounds__(VX_THREADS) void vx_count_kernel(const int32_t* __restrict__ lab, int D, int H, int W,
                                                              const float* __restrict__ pal, int P, int bpg, int64_t vox,
                                                              const float* __restrict__ bm, int32_t* __restrict__ bcnt,
                                                              int32_t* __restrict__ keys) {
  __shared__ int32_t lds[VX_THREADS];
  const int n = blockIdx.y, bb = blockIdx.x;
  const int32_t* g = lab + (int64_t)n * vox;
  int32_t cnt = 0;
  int32_t kmin[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, kmax[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
#pragma unroll
  for (int i = 0; i < VX_PER_THREAD; ++i) {
    const int64_t v = (int64_t)bb * VX_BLOCK + i * VX_THREADS + threadIdx.x;
    if (v >= vox) break;
    int z, y, x;
    vx_coords(v, H, W, z, y, x);
    cnt += 2 * vx_popc(vx_faces(g, D, H, W, z, y, x, pal, P));
    if (bm && g[v] != 0) {
      float c[3];
      vx_centre(bm + 16 * n, z, y, x, c);
      for (int q = 0; q < 3; ++q) {
        if (c[q] != c[q]) continue;
        const int32_t k = vx_key(c[q]);
        kmin[q] = min(kmin[q], k);
        kmax[q] = max(kmax[q], k);
      }
    }
  }
  int32_t total;
  block_exclusive_scan<VX_THREADS>(cnt, lds, total);
  if (threadIdx.x == 0) bcnt[(int64_t)n * bpg + bb] = total;
  if (bm) {
    for (int q = 0; q < 3; ++q) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        kmin[q] = min(kmin[q], __shfl_xor(kmin[q], o, 64));
        kmax[q] = max(kmax[q], __shfl_xor(kmax[q], o, 64));
      }
    }
    if ((threadIdx.x & 63) == 0)
      for (int q = 0; q < 3; ++q) {
        if (kmin[q] != INT32_MAX) atomicMin(keys + 6 * n + q, kmin[q]);
        if (kmax[q] != INT32_MIN) atomicMax(keys + 6 * n + 3 + q, kmax[q]);
      }
  }
}

__global__ void vx_sizes_kernel(const int64_t* __restrict__ boff, int N, int bpg, const int32_t* __restrict__ keys,
                                float* __restrict__ box, int64_t* __restrict__ counts) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  counts[n] = boff[(int64_t)(n + 1) * bpg] - boff[(int64_t)n * bpg];
  if (box) {
    const bool none = keys[6 * n] == INT32_MAX;
    for (int q = 0; q < 6; ++q) box[6 * n + q] = none ? 0.f : vx_unkey(keys[6 * n + q]);
  }
}

__global__ __launch_bounds__(VX_THREADS) void vx_emit_kernel(const int32_t* __restrict__ lab, int D, int H, int W,
                                                             const float* __restrict__ pal, int P, int bpg, int64_t vox,
                                                             const float* __restrict__ mats, int mbase,
                                                             const int64_t* __restrict__ boff, float* __restrict__ tri,
                                                             float* __restrict__ nrm, int32_t* __restrict__ mids) {
  __shared__ int32_t lds[VX_THREADS];
  const int n = blockIdx.y, bb = blockIdx.x;
  const int64_t blk = (int64_t)n * bpg + bb;
  if (boff[blk + 1] == boff[blk]) return;
  const int32_t* g = lab + (int64_t)n * vox;
  const float* m = mats + 16 * n;
  int64_t base = boff[blk];
#pragma unroll 1
  for (int i = 0; i < VX_PER_THREAD; ++i) {
    const int64_t v = (int64_t)bb * VX_BLOCK + i * VX_THREADS + threadIdx.x;
    int z = 0, y = 0, x = 0, mask = 0;
    if (v < vox) {
      vx_coords(v, H, W, z, y, x);
      mask = vx_faces(g, D, H, W, z, y, x, pal, P);
    }
    int32_t total;
    const int32_t e = block_exclusive_scan<VX_THREADS>(2 * vx_popc(mask), lds, total);
    int64_t o = base + e;
    for (int f = 0; f < 6; ++f) {
      if (!((mask >> f) & 1)) continue;
      float t18[18], nn[3];
      vx_quad(m, z, y, x, f, t18, nn);
      for (int q = 0; q < 18; ++q) tri[9 * o + q] = t18[q];
      for (int k = 0; k < 6; ++k)
        for (int q = 0; q < 3; ++q) nrm[9 * o + 3 * k + q] = nn[q];
      mids[o] = mbase + g[v];
      mids[o + 1] = mbase + g[v];
      o += 2;
    }
    base += total;
  }
}

bool rd_args_ok(const crnRenderImage* images, int I, int H, int W, int max_len) {
  return images && I >= 1 && I <= 65535 && H >= 1 && W >= 1 && H <= (1 << 14) && W <= (1 << 14) && max_len >= 0;
}

}  // namespace

extern "C" int crn_render_bin(const float* triangles, const crnRenderImage* images, int I, int H, int W, int max_len,
                              int64_t num_inst, float* records, int32_t* bin_counts, int64_t* bin_offsets, crnStream s) {
  if (!rd_args_ok(images, I, H, W, max_len) || !bin_counts || !bin_offsets || num_inst < 0 ||
      num_inst >= ((int64_t)1 << 31) || (num_inst > 0 && (!triangles || !records)))
    return CRN_EINVAL;
  hipStream_t st = (hipStream_t)s;
  const int64_t nb = (int64_t)I * ((W + RD_T - 1) / RD_T) * ((H + RD_T - 1) / RD_T);
  CRN_HIP(hipMemsetAsync(bin_counts, 0, (size_t)nb * 4, st));
  if (max_len > 0) {
    hipLaunchKernelGGL(rd_setup_kernel, dim3((unsigned)crn_cdiv(max_len, 256), (unsigned)I), dim3(256), 0, st, triangles,
                       images, H, W, records, bin_counts);
    CRN_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(rd_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, bin_counts, nb, bin_offsets);
  CRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int crn_render_raster(const float* triangles, const float* normals, const int32_t* material_ids,
                                 const float* materials, int M, const crnRenderImage* images, int I, int H, int W,
                                 int max_len, const float* records, int32_t* bin_counts, const int64_t* bin_offsets,
                                 int32_t* bin_list, uint8_t* out, crnStream s) {
  return crn_render_raster_tex(triangles, normals, material_ids, materials, M, images, I, H, W, max_len, records,
                               bin_counts, bin_offsets, bin_list, out, nullptr, nullptr, nullptr, 0, 0, 0, s);
}

extern "C" int crn_render_raster_tex(const float* triangles, const float* normals, const int32_t* material_ids,
                                     const float* materials, int M, const crnRenderImage* images, int I, int H, int W,
                                     int max_len, const float* records, int32_t* bin_counts, const int64_t* bin_offsets,
                                     int32_t* bin_list, uint8_t* out, const float* texcoords, const int32_t* texture_ids,
                                     const uint8_t* textures, int L, int Ht, int Wt, crnStream s) {
  if (!rd_args_ok(images, I, H, W, max_len) || !bin_counts || !bin_offsets || !out || M < 0) return CRN_EINVAL;
  if (max_len > 0 && (!triangles || !material_ids || !records || !bin_list)) return CRN_EINVAL;
  if (textures && (!rd_tex_dims_ok(L, Ht, Wt) || ((uintptr_t)textures & 3))) return CRN_EINVAL;
  hipStream_t st = (hipStream_t)s;
  const int ntiles = ((W + RD_T - 1) / RD_T) * ((H + RD_T - 1) / RD_T);
  if (max_len > 0) {
    hipLaunchKernelGGL(rd_fill_kernel, dim3((unsigned)crn_cdiv(max_len, 256), (unsigned)I), dim3(256), 0, st, images, H, W,
                       records, bin_counts, bin_offsets, bin_list);
    CRN_CHECK_LAUNCH();
  }
  if (textures && texture_ids && M > 0) {
    const crnRdTex tex = {texcoords, texture_ids, reinterpret_cast<const uint32_t*>(textures), L, Ht, Wt};
    hipLaunchKernelGGL(rd_raster_tex_kernel, dim3((unsigned)ntiles, (unsigned)I), dim3(RD_THREADS), 0, st, triangles,
                       normals, material_ids, materials, M, images, H, W, records, bin_offsets, bin_list, out, tex);
  } else {
    hipLaunchKernelGGL(rd_raster_kernel, dim3((unsigned)ntiles, (unsigned)I), dim3(RD_THREADS), 0, st, triangles, normals,
                       material_ids, materials, M, images, H, W, records, bin_offsets, bin_list, out);
  }
  CRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int crn_render_raster_geometry(const float* triangles, const crnRenderImage* images, int I, int H, int W,
                                          int max_len, const float* records, int32_t* bin_counts,
                                          const int64_t* bin_offsets, int32_t* bin_list, int32_t* triangle_index,
                                          float* barycentrics, float* depth, float* z_ndc, crnStream s) {
  if (!rd_args_ok(images, I, H, W, max_len) || !bin_counts || !bin_offsets) return CRN_EINVAL;
  if (!triangle_index && !barycentrics && !depth && !z_ndc) return CRN_EINVAL;
  if (max_len > 0 && (!triangles || !records || !bin_list)) return CRN_EINVAL;
  hipStream_t st = (hipStream_t)s;
  const int ntiles = ((W + RD_T - 1) / RD_T) * ((H + RD_T - 1) / RD_T);
  if (max_len > 0) {
    hipLaunchKernelGGL(rd_fill_kernel, dim3((unsigned)crn_cdiv(max_len, 256), (unsigned)I), dim3(256), 0, st, images, H, W,
                       records, bin_counts, bin_offsets, bin_list);
    CRN_CHECK_LAUNCH();
  }
  const crnRdGeomOut out = {triangle_index, barycentrics, depth, z_ndc};
  hipLaunchKernelGGL(rd_raster_geometry_kernel, dim3((unsigned)ntiles, (unsigned)I), dim3(RD_THREADS), 0, st, triangles,
                     images, H, W, records, bin_offsets, bin_list, out);
  CRN_CHECK_LAUNCH();
  return 0;
}

extern "C" size_t crn_voxel_faces_workspace_bytes(int N, int D, int H, int W) {
  if (N < 1 || D < 1 || H < 1 || W < 1) return 0;
  return vx_layout(N, D, H, W).bytes;
}

extern "C" int crn_voxel_faces_count(const int32_t* labels, int N, int D, int H, int W, const float* palette, int P,
                                     const float* box_matrices, float* box_out, void* workspace, size_t workspace_bytes,
                                     int64_t* counts, crnStream s) {
  if (!labels || N < 1 || N > 65535 || D < 1 || H < 1 || W < 1 || !palette || P < 1 || !workspace || !counts ||
      (box_matrices && !box_out))
    return CRN_EINVAL;
  const VxLayout L = vx_layout(N, D, H, W);
  if (workspace_bytes < L.bytes || L.nb >= ((int64_t)1 << 31)) return CRN_EINVAL;
  char* ws = (char*)workspace;
  int32_t* bcnt = (int32_t*)(ws + L.o_bcnt);
  int64_t* boff = (int64_t*)(ws + L.o_boff);
  int32_t* keys = (int32_t*)(ws + L.o_keys);
  hipStream_t st = (hipStream_t)s;
  if (box_matrices) {
    hipLaunchKernelGGL(vx_key_init_kernel, dim3(crn_cdiv(6 * N, 256)), dim3(256), 0, st, keys, N);
    CRN_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(vx_count_kernel, dim3((unsigned)L.bpg, (unsigned)N), dim3(VX_THREADS), 0, st, labels, D, H, W, palette,
                     P, L.bpg, L.vox, box_matrices, bcnt, keys);
  CRN_CHECK_LAUNCH();
  hipLaunchKernelGGL(rd_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, bcnt, L.nb, boff);
  CRN_CHECK_LAUNCH();
  hipLaunchKernelGGL(vx_sizes_kernel, dim3(crn_cdiv(N, 256)), dim3(256), 0, st, boff, N, L.bpg, keys,
                     box_matrices ? box_out : nullptr, counts);
  CRN_CHECK_LAUNCH();
  return 0;
}

extern "C" int crn_voxel_faces_emit(const int32_t* labels, int N, int D, int H, int W, const float* palette, int P,
                                    const float* matrices, int material_base, void* workspace, size_t workspace_bytes,
                                    float* triangles, float* normals, int32_t* material_ids, crnStream s) {
  if (!labels || N < 1 || N > 65535 || D < 1 || H < 1 || W < 1 || !palette || P < 1 || !matrices || !workspace ||
      !triangles || !normals || !material_ids)
    return CRN_EINVAL;
  const VxLayout L = vx_layout(N, D, H, W);
  if (workspace_bytes < L.bytes) return CRN_EINVAL;
  const int64_t* boff = (const int64_t*)((char*)workspace + L.o_boff);
  hipLaunchKernelGGL(vx_emit_kernel, dim3((unsigned)L.bpg, (unsigned)N), dim3(VX_THREADS), 0, (hipStream_t)s, labels, D, H,
                     W, palette, P, L.bpg, L.vox, matrices, material_base, boff, triangles, normals, material_ids);
  CRN_CHECK_LAUNCH();
  return 0;
}
