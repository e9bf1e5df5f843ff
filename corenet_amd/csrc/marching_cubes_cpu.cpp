// Marching cubes and the box filter on the host: the twin of marching_cubes.hip, part of the product library.
// Same contract, same tables (mc_tables.h), same per-sample arithmetic (marching_cubes_common.h), same output order:
// the GPU and this twin return identical arrays.
//
// One object per task (std::thread workers pulling object ids).  Emit walks the cells plane by plane in raster order
// and keeps the per-cell vertex offsets of two planes (z and z + 1): every crossing edge a cell touches is owned by a
// grid point of plane z or z + 1 (edges owned by points of the last padded planes lie in the zero border and never cross).
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

#include "../../include/corenet_hip.h"
#include "marching_cubes_common.h"
#include "mc_tables.h"

namespace {

int cell_case(const crnMcGrid& g, const float* obj, int z, int y, int x) {
  int cs = 0;
  for (int c = 0; c < 8; ++c) cs |= mc_inside(mc_at(g, obj, z + (c >> 2), y + ((c >> 1) & 1), x + (c & 1)), g.level) << c;
  return cs;
}

// per-cell object-local vertex offsets of plane z, starting at `base`; returns the running count after the plane
int64_t plane_offsets(const crnMcGrid& g, const float* obj, int z, int64_t base, std::vector<int32_t>& off) {
  const int CW = g.W + 1, CH = g.H + 1;
  for (int y = 0; y < CH; ++y)
    for (int x = 0; x < CW; ++x) {
      off[(size_t)y * CW + x] = (int32_t)base;
      base += mc_popc3(mc_owned_bits(g, obj, z, y, x));
    }
  return base;
}

void count_object(const crnMcGrid& g, int n, int64_t* counts) {
  const float* obj = g.p + n * g.sN;
  int64_t nv = 0, nt = 0;
  for (int z = 0; z <= g.D; ++z)
    for (int y = 0; y <= g.H; ++y)
      for (int x = 0; x <= g.W; ++x) {
        const int cs = cell_case(g, obj, z, y, x);
        if (cs == 0 || cs == 255) continue;
        nv += mc_popc3(mc_case_owned_bits(cs));
        nt += crn_mc_num_tri[cs];
      }
  counts[2 * n] = nv;
  counts[2 * n + 1] = nt;
}

void emit_object(const crnMcGrid& g, int n, int64_t vbase, int64_t tbase, const float* matrices, float* vertices,
                 float* normals, int32_t* faces) {
  const float* obj = g.p + n * g.sN;
  const float* m = matrices ? matrices + 16 * (int64_t)n : nullptr;
  const int CW = g.W + 1, CH = g.H + 1;
  std::vector<int32_t> cur((size_t)CW * CH), nxt((size_t)CW * CH);
  int64_t running = plane_offsets(g, obj, 0, 0, cur);
  int64_t tri = tbase;
  for (int z = 0; z <= g.D; ++z) {
    if (z < g.D) running = plane_offsets(g, obj, z + 1, running, nxt);
    for (int y = 0; y < CH; ++y)
      for (int x = 0; x < CW; ++x) {
        const int cs = cell_case(g, obj, z, y, x);
        if (cs == 0 || cs == 255) continue;
        const int own = mc_case_owned_bits(cs);
        int32_t v = cur[(size_t)y * CW + x];
        for (int a = 0; a < 3; ++a) {
          if (!((own >> a) & 1)) continue;
          float pos[3], nrm[3];
          mc_vertex(g, obj, z, y, x, a, pos, nrm);
          if (m) mc_transform(m, pos, nrm);
          const int64_t gv = vbase + v;
          for (int c = 0; c < 3; ++c) { vertices[3 * gv + c] = pos[c]; normals[3 * gv + c] = nrm[c]; }
          ++v;
        }
        const int nt = crn_mc_num_tri[cs];
        for (int k = 0; k < 3 * nt; ++k) {
          int a, dx, dy, dz;
          mc_edge(crn_mc_tri[cs][k], a, dx, dy, dz);
          const int oz = z + dz, oy = y + dy, ox = x + dx;
          const std::vector<int32_t>& pl = dz ? nxt : cur;
          int32_t idx = pl[(size_t)oy * CW + ox];
          if (a >= 1) idx += mc_crosses(g, obj, oz, oy, ox, 0);
          if (a == 2) idx += mc_crosses(g, obj, oz, oy, ox, 1);
          faces[3 * tri + k % 3] = idx;
          if (k % 3 == 2) ++tri;
        }
      }
    cur.swap(nxt);
  }
}

template <typename F>
void for_objects(int N, int num_threads, F fn) {
  int nt = num_threads > 0 ? num_threads : (int)std::thread::hardware_concurrency();
  if (nt < 1) nt = 1;
  if (nt > N) nt = N;
  std::atomic<int> next(0);
  auto work = [&]() {
    for (int n = next.fetch_add(1); n < N; n = next.fetch_add(1)) fn(n);
  };
  std::vector<std::thread> th;
  for (int i = 1; i < nt; ++i) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
}

}  // namespace

extern "C" int crn_marching_cubes_cpu(const float* grid, const int64_t* strides, int N, int D, int H, int W, float level,
                                      const float* matrices, int64_t* counts, float* vertices, float* normals,
                                      int32_t* faces, int num_threads) {
  if (!grid || !strides || !counts || N < 1 || D < 1 || H < 1 || W < 1 || !(level > 0.f)) return CRN_EINVAL;
  if (strides[3] != 1 || (int64_t)(D + 1) * (H + 1) * (W + 1) > CRN_MC_MAX_OBJECT_CELLS) return CRN_EINVAL;
  if (vertices && (!normals || !faces)) return CRN_EINVAL;
  const crnMcGrid g{grid, strides[0], strides[1], strides[2], D, H, W, level};
  if (!vertices) {
    for_objects(N, num_threads, [&](int n) { count_object(g, n, counts); });
    return 0;
  }
  std::vector<int64_t> vb(N), tb(N);
  int64_t v = 0, t = 0;
  for (int n = 0; n < N; ++n) { vb[n] = v; tb[n] = t; v += counts[2 * n]; t += counts[2 * n + 1]; }
  for_objects(N, num_threads, [&](int n) { emit_object(g, n, vb[n], tb[n], matrices, vertices, normals, faces); });
  return 0;
}

extern "C" int crn_box_filter_cpu(const float* in, const int64_t* strides, float* out, int N, int D, int H, int W, int k,
                                  int num_threads) {
  if (!in || !strides || !out || N < 1 || D < 1 || H < 1 || W < 1 || k < 1) return CRN_EINVAL;
  const int64_t S = (int64_t)D * H * W;
  const float inv = 1.0f / (float)((int64_t)k * k * k);
  std::vector<float> tmp((size_t)(N * S));
  float* tp = tmp.data();
  // pass w: in (strided) -> out; pass h: out -> tmp; pass d: tmp -> out, scaled
  for_objects(N, num_threads, [&](int n) {
    for (int d = 0; d < D; ++d)
      for (int h = 0; h < H; ++h)
        for (int w = 0; w < W; ++w)
          out[n * S + ((int64_t)d * H + h) * W + w] =
              mc_box_tap(in, n * strides[0] + d * strides[1] + h * strides[2], strides[3], w, W, k, 1.f);
    for (int d = 0; d < D; ++d)
      for (int h = 0; h < H; ++h)
        for (int w = 0; w < W; ++w)
          tp[n * S + ((int64_t)d * H + h) * W + w] = mc_box_tap(out, n * S + (int64_t)d * H * W + w, W, h, H, k, 1.f);
    for (int d = 0; d < D; ++d)
      for (int h = 0; h < H; ++h)
        for (int w = 0; w < W; ++w)
          out[n * S + ((int64_t)d * H + h) * W + w] = mc_box_tap(tp, n * S + (int64_t)h * W + w, (int64_t)H * W, d, D, k, inv);
  });
  return 0;
}
