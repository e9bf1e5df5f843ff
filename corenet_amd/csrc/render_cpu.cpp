// Rendering and voxel-face extraction on the host: the twin of render.hip, part of the product library.  Same contract,
// same per-triangle and per-pixel arithmetic (render_common.h), same winner rule (min z, then the later triangle), so
// the GPU and this twin give identical images (and identical face arrays).
//
// Renderer: one image per task (std::thread workers pulling image ids); per image a depth / winner buffer, every setup
// record tested against the pixels of its box, then every pixel shaded once.  Voxel faces: one grid per task.
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

#include "../../include/corenet_hip.h"
#include "render_common.h"

namespace {

template <typename F>
void for_tasks(int n, int num_threads, F fn) {
  int nt = num_threads > 0 ? num_threads : (int)std::thread::hardware_concurrency();
  if (nt < 1) nt = 1;
  if (nt > n) nt = n;
  std::atomic<int> next(0);
  auto work = [&]() {
    for (int i = next++; i < n; i = next++) fn(i);
  };
  if (nt == 1) {
    work();
    return;
  }
  std::vector<std::thread> th;
  for (int k = 0; k < nt; ++k) th.emplace_back(work);
  for (auto& x : th) x.join();
}

// The setup records of an image's range and, per pixel, the winning record id (-1: none) and its z_ndc.
void winners(const float* tri, const crnRenderImage& im, int H, int W, std::vector<crnRdRec>& recs,
             std::vector<float>& bz, std::vector<int32_t>& bid) {
  const int64_t np = (int64_t)H * W;
  bz.assign(np, 0.f);
  bid.assign(np, -1);
  const int len = im.t1 - im.t0;
  recs.resize(len > 0 ? len : 0);
  for (int k = 0; k < len; ++k) {
    crnRdRec& r = recs[k];
    if (!rd_setup(im, H, W, tri + 9 * (int64_t)(im.t0 + k), r)) continue;
    const int32_t id = im.inst0 + k;
    for (int row = r.box[1]; row <= r.box[3]; ++row)
      for (int col = r.box[0]; col <= r.box[2]; ++col) {
        float E[3], z;
        const int64_t p = (int64_t)row * W + col;
        if (rd_fragment(r, col, row, E, z) && rd_wins(z, id, bz[p], bid[p])) {
          bz[p] = z;
          bid[p] = id;
        }
      }
  }
}

void render_image(const float* tri, const float* nrm, const int32_t* mids, const float* mats, int M,
                  const crnRenderImage& im, int H, int W, uint8_t* out, const crnRdTex& tex) {
  std::vector<crnRdRec> recs;
  std::vector<float> bz;
  std::vector<int32_t> bid;
  winners(tri, im, H, W, recs, bz, bid);
  for (int row = 0; row < H; ++row)
    for (int col = 0; col < W; ++col) {
      const int64_t p = (int64_t)row * W + col;
      uint8_t* o = out + 3 * p;
      if (bid[p] < 0) {
        o[0] = rd_u8(im.clear[0]); o[1] = rd_u8(im.clear[1]); o[2] = rd_u8(im.clear[2]);
        continue;
      }
      const int k = bid[p] - im.inst0;
      float E[3], z;
      rd_fragment(recs[k], col, row, E, z);
      const int64_t t = (int64_t)im.t0 + k;
      const int32_t m = mids[t];
      const bool has_mat = m >= 0 && m < M;
      const float* mat = has_mat ? mats + 10 * (int64_t)m : nullptr;
      float tmat[10];
      const int32_t layer = has_mat && tex.texels ? tex.ids[m] : -1;
      if (layer >= 0 && layer < tex.L) {
        for (int q = 0; q < 10; ++q) tmat[q] = mat[q];
        rd_tex_diffuse(E, tex.uv ? tex.uv + 6 * t : nullptr, tex.texels, tex.Ht, tex.Wt, layer, tmat);
        mat = tmat;
      }
      rd_shade(im, tri + 9 * t, nrm ? nrm + 9 * t : nullptr, mat, E, o);
    }
}

// The requested geometry outputs of one image (each pointer at the image's first pixel, or NULL).
void geometry_image(const float* tri, const crnRenderImage& im, int H, int W, int32_t* out_tri, float* out_bary,
                    float* out_depth, float* out_z) {
  std::vector<crnRdRec> recs;
  std::vector<float> bz;
  std::vector<int32_t> bid;
  winners(tri, im, H, W, recs, bz, bid);
  for (int row = 0; row < H; ++row)
    for (int col = 0; col < W; ++col) {
      const int64_t p = (int64_t)row * W + col;
      int32_t t = -1;
      float bary[3] = {0.f, 0.f, 0.f}, depth = INFINITY, z = INFINITY;
      if (bid[p] >= 0) {
        const int k = bid[p] - im.inst0;
        float E[3];
        rd_fragment(recs[k], col, row, E, z);
        t = im.t0 + k;
        rd_geometry(im, tri + 9 * (int64_t)t, E, bary, depth);
      }
      if (out_tri) out_tri[p] = t;
      if (out_bary) {
        out_bary[3 * p] = bary[0]; out_bary[3 * p + 1] = bary[1]; out_bary[3 * p + 2] = bary[2];
      }
      if (out_depth) out_depth[p] = depth;
      if (out_z) out_z[p] = z;
    }
}

}  // namespace

extern "C" int crn_render_cpu_geometry(const float* triangles, const crnRenderImage* images, int I, int H, int W,
                                       int32_t* triangle_index, float* barycentrics, float* depth, float* z_ndc,
                                       int num_threads) {
  if (!images || I < 1 || H < 1 || W < 1) return CRN_EINVAL;
  if (!triangle_index && !barycentrics && !depth && !z_ndc) return CRN_EINVAL;
  for (int i = 0; i < I; ++i) {
    if (images[i].t1 < images[i].t0) return CRN_EINVAL;
    if (images[i].t1 > images[i].t0 && !triangles) return CRN_EINVAL;
  }
  const int64_t np = (int64_t)H * W;
  for_tasks(I, num_threads, [&](int i) {
    geometry_image(triangles, images[i], H, W, triangle_index ? triangle_index + i * np : nullptr,
                   barycentrics ? barycentrics + 3 * i * np : nullptr, depth ? depth + i * np : nullptr,
                   z_ndc ? z_ndc + i * np : nullptr);
  });
  return 0;
}

extern "C" int crn_render_cpu(const float* triangles, const float* normals, const int32_t* material_ids,
                              const float* materials, int M, const crnRenderImage* images, int I, int H, int W,
                              uint8_t* out, int num_threads) {
  return crn_render_cpu_tex(triangles, normals, material_ids, materials, M, images, I, H, W, out, nullptr, nullptr,
                            nullptr, 0, 0, 0, num_threads);
}

extern "C" int crn_render_cpu_tex(const float* triangles, const float* normals, const int32_t* material_ids,
                                  const float* materials, int M, const crnRenderImage* images, int I, int H, int W,
                                  uint8_t* out, const float* texcoords, const int32_t* texture_ids,
                                  const uint8_t* textures, int L, int Ht, int Wt, int num_threads) {
  if (!images || I < 1 || H < 1 || W < 1 || !out || M < 0) return CRN_EINVAL;
  if (textures && (!rd_tex_dims_ok(L, Ht, Wt) || ((uintptr_t)textures & 3))) return CRN_EINVAL;
  crnRdTex tex = {nullptr, nullptr, nullptr, 0, 0, 0};
  if (textures && texture_ids) tex = {texcoords, texture_ids, reinterpret_cast<const uint32_t*>(textures), L, Ht, Wt};
  for (int i = 0; i < I; ++i) {
    if (images[i].t1 < images[i].t0) return CRN_EINVAL;
    if (images[i].t1 > images[i].t0 && (!triangles || !material_ids)) return CRN_EINVAL;
    if (images[i].normal_mode != 0 && images[i].t1 > images[i].t0 && !normals) return CRN_EINVAL;
  }
  for_tasks(I, num_threads, [&](int i) {
    render_image(triangles, normals, material_ids, materials, M, images[i], H, W, out + (int64_t)i * H * W * 3, tex);
  });
  return 0;
}

extern "C" int crn_voxel_faces_cpu(const int32_t* labels, int N, int D, int H, int W, const float* palette, int P,
                                   const float* box_matrices, float* box_out, const float* matrices, int material_base,
                                   int64_t* counts, float* triangles, float* normals, int32_t* material_ids,
                                   int num_threads) {
  if (!labels || N < 1 || D < 1 || H < 1 || W < 1 || !palette || P < 1 || !counts) return CRN_EINVAL;
  const int64_t vox = (int64_t)D * H * W;
  if (!triangles) {
    if (box_matrices && !box_out) return CRN_EINVAL;
    for_tasks(N, num_threads, [&](int n) {
      const int32_t* g = labels + n * vox;
      int64_t c = 0;
      int32_t kmin[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, kmax[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
      for (int z = 0; z < D; ++z)
        for (int y = 0; y < H; ++y)
          for (int x = 0; x < W; ++x) {
            c += 2 * vx_popc(vx_faces(g, D, H, W, z, y, x, palette, P));
            if (box_matrices && g[((int64_t)z * H + y) * W + x] != 0) {
              float q[3];
              vx_centre(box_matrices + 16 * n, z, y, x, q);
              for (int a = 0; a < 3; ++a) {
                if (q[a] != q[a]) continue;
                const int32_t k = vx_key(q[a]);
                kmin[a] = k < kmin[a] ? k : kmin[a];
                kmax[a] = k > kmax[a] ? k : kmax[a];
              }
            }
          }
      counts[n] = c;
      if (box_matrices) {
        const bool none = kmin[0] == INT32_MAX;
        for (int a = 0; a < 3; ++a) {
          box_out[6 * n + a] = none ? 0.f : vx_unkey(kmin[a]);
          box_out[6 * n + 3 + a] = none ? 0.f : vx_unkey(kmax[a]);
        }
      }
    });
    return 0;
  }
  if (!matrices || !normals || !material_ids) return CRN_EINVAL;
  std::vector<int64_t> base(N + 1, 0);
  for (int n = 0; n < N; ++n) base[n + 1] = base[n] + counts[n];
  for_tasks(N, num_threads, [&](int n) {
    const int32_t* g = labels + n * vox;
    const float* m = matrices + 16 * n;
    int64_t o = base[n];
    for (int z = 0; z < D; ++z)
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
          const int mask = vx_faces(g, D, H, W, z, y, x, palette, P);
          for (int f = 0; f < 6; ++f) {
            if (!((mask >> f) & 1)) continue;
            float t18[18], nn[3];
            vx_quad(m, z, y, x, f, t18, nn);
            for (int q = 0; q < 18; ++q) triangles[9 * o + q] = t18[q];
            for (int k = 0; k < 6; ++k)
              for (int q = 0; q < 3; ++q) normals[9 * o + 3 * k + q] = nn[q];
            const int32_t l = g[((int64_t)z * H + y) * W + x];
            material_ids[o] = material_base + l;
            material_ids[o + 1] = material_base + l;
            o += 2;
          }
        }
  });
  return 0;
}
