// Triangle and voxel-grid rendering: the per-triangle and per-pixel arithmetic shared by the HIP kernels (render.hip)
// and the host twin (render_cpu.cpp).  Both include this header, so a setup record, a coverage / depth decision and a
// shaded colour are the same float32 operations in the same order on either side (both are compiled with
// -ffp-contract=off; normalize is sqrtf and divides).  Contract: corenet_amd/visualization/render.py, DESIGN section 14.
//
// Screen: image row r, column c samples window (c + 0.5, r + 0.5); window x = (x_ndc + 1) / 2 * W, y likewise with H,
// so row 0 is NDC y = -1.  Rasterisation is homogeneous (Olano & Greer): with V_k = (X_k, Y_k, w_k) the window-scaled
// clip vertices (X = (x + w) W / 2, Y = (y + w) H / 2), edge i is the cross product of the other two vertices and the
// barycentrics at window point p are lambda_i = E_i(p) / det.  A pixel is covered iff every lambda_i >= 0 (top-left
// rule on E_i == 0), which is exactly the part of the triangle in front of the eye (w > 0): no clipping pass, no
// wrap-around.  z_ndc = sum lambda_i z_clip_i is a plane in window space; a fragment survives iff it is in [-1, 1].
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/corenet_hip.h"

#if defined(__HIP__)
#define CRN_RD_HD __host__ __device__ inline
#else
#define CRN_RD_HD inline
#endif

// Setup record of one (image, triangle): sign-normalised edges (a, b, c) x 3, the z_ndc plane, and the pixel box
// [c0, c1] x [r0, r1] (inclusive; c0 > c1 when the triangle is invisible).  16 words = 4 x float4.
struct crnRdRec {
  float e[3][3];
  float z[3];
  int32_t box[4];          // c0, r0, c1, r1
};

CRN_RD_HD void rd_xform4(const float* m, float x, float y, float z, float o[4]) {
  for (int r = 0; r < 4; ++r) o[r] = ((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3];
}

CRN_RD_HD void rd_invisible(crnRdRec& r) {
  r.box[0] = 1; r.box[1] = 1; r.box[2] = 0; r.box[3] = 0;
}

CRN_RD_HD int rd_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// p: the triangle's 9 world coordinates.  Returns true iff the record can cover a pixel.
CRN_RD_HD bool rd_setup(const crnRenderImage& im, int H, int W, const float* p, crnRdRec& r) {
  float c[3][4];
  for (int k = 0; k < 3; ++k) rd_xform4(im.vp, p[3 * k], p[3 * k + 1], p[3 * k + 2], c[k]);
  rd_invisible(r);
  if (im.cull) {                                   // triangle_renderer.geom is_back_facing: NDC after the divide
    const float x0 = c[0][0] / c[0][3], y0 = c[0][1] / c[0][3];
    const float ax = c[1][0] / c[1][3] - x0, ay = c[1][1] / c[1][3] - y0;
    const float bx = c[2][0] / c[2][3] - x0, by = c[2][1] / c[2][3] - y0;
    if (ax * by - bx * ay <= 0.f) return false;
  }
  const float w0 = c[0][3], w1 = c[1][3], w2 = c[2][3];
  if (!(w0 > 0.f || w1 > 0.f || w2 > 0.f) || w0 != w0 || w1 != w1 || w2 != w2) return false;   // all behind the eye
  const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
  float X[3], Y[3], Wc[3];
  for (int k = 0; k < 3; ++k) {
    X[k] = (c[k][0] + c[k][3]) * hw;
    Y[k] = (c[k][1] + c[k][3]) * hh;
    Wc[k] = c[k][3];
  }
  for (int i = 0; i < 3; ++i) {
    const int j = i == 2 ? 0 : i + 1, k = i == 0 ? 2 : i - 1;
    r.e[i][0] = Y[j] * Wc[k] - Wc[j] * Y[k];
    r.e[i][1] = Wc[j] * X[k] - X[j] * Wc[k];
    r.e[i][2] = X[j] * Y[k] - Y[j] * X[k];
  }
  float det = (r.e[0][0] * X[0] + r.e[0][1] * Y[0]) + r.e[0][2] * Wc[0];
  if (!(det > 0.f || det < 0.f)) return false;     // degenerate or NaN
  if (det < 0.f) {
    det = -det;
    for (int i = 0; i < 3; ++i)
      for (int q = 0; q < 3; ++q) r.e[i][q] = -r.e[i][q];
  }
  for (int q = 0; q < 3; ++q) r.z[q] = ((r.e[0][q] * c[0][2] + r.e[1][q] * c[1][2]) + r.e[2][q] * c[2][2]) / det;
  int c0 = 0, r0 = 0, c1 = W - 1, r1 = H - 1;
  if (w0 > 0.f && w1 > 0.f && w2 > 0.f) {          // else: part of it is behind the eye, the whole image bounds it
    float xs[3], ys[3];
    for (int k = 0; k < 3; ++k) {
      xs[k] = fminf(fmaxf(X[k] / Wc[k], -2.f), (float)W + 2.f);
      ys[k] = fminf(fmaxf(Y[k] / Wc[k], -2.f), (float)H + 2.f);
    }
    c0 = rd_clampi((int)floorf(fminf(fminf(xs[0], xs[1]), xs[2])) - 1, 0, W - 1);
    c1 = rd_clampi((int)floorf(fmaxf(fmaxf(xs[0], xs[1]), xs[2])) + 1, 0, W - 1);
    r0 = rd_clampi((int)floorf(fminf(fminf(ys[0], ys[1]), ys[2])) - 1, 0, H - 1);
    r1 = rd_clampi((int)floorf(fmaxf(fmaxf(ys[0], ys[1]), ys[2])) + 1, 0, H - 1);
  }
  r.box[0] = c0; r.box[1] = r0; r.box[2] = c1; r.box[3] = r1;
  return true;
}

CRN_RD_HD bool rd_edge_in(float a, float b, float c, float px, float py, float& E) {
  E = (a * px + b * py) + c;
  return E > 0.f || (E == 0.f && (a > 0.f || (a == 0.f && b > 0.f)));
}

// Coverage and depth of pixel (col, row): true iff covered and z_ndc in [-1, 1] (NaN fails); E and z returned.
CRN_RD_HD bool rd_fragment(const crnRdRec& r, int col, int row, float E[3], float& z) {
  if (col < r.box[0] || col > r.box[2] || row < r.box[1] || row > r.box[3]) return false;
  const float px = (float)col + 0.5f, py = (float)row + 0.5f;
  if (!rd_edge_in(r.e[0][0], r.e[0][1], r.e[0][2], px, py, E[0])) return false;
  if (!rd_edge_in(r.e[1][0], r.e[1][1], r.e[1][2], px, py, E[1])) return false;
  if (!rd_edge_in(r.e[2][0], r.e[2][1], r.e[2][2], px, py, E[2])) return false;
  z = (r.z[0] * px + r.z[1] * py) + r.z[2];
  return z >= -1.f && z <= 1.f;
}

// GL depth test LESS_EQUAL in submission order == the smallest z wins, the later primitive on equal z.
CRN_RD_HD bool rd_wins(float z, int32_t id, float bz, int32_t bid) {
  return bid < 0 || z < bz || (z == bz && id > bid);
}

// Geometry of the winning fragment (crn_render_raster_geometry): the perspective-correct weights b_i = E_i / s with
// s = (E0 + E1) + E2, the ones rd_shade and rd_tex_diffuse interpolate with, and the fragment's clip-space w,
// sum E_k w_k / s with w_k the fourth component of vp . (p_k, 1).  p: the triangle's 9 world coordinates.
CRN_RD_HD void rd_geometry(const crnRenderImage& im, const float* p, const float E[3], float b[3], float& depth) {
  const float s = (E[0] + E[1]) + E[2];
  float w[3];
  for (int k = 0; k < 3; ++k) {
    float c[4];
    rd_xform4(im.vp, p[3 * k], p[3 * k + 1], p[3 * k + 2], c);
    w[k] = c[3];
  }
  for (int i = 0; i < 3; ++i) b[i] = E[i] / s;
  depth = ((E[0] * w[0] + E[1] * w[1]) + E[2] * w[2]) / s;
}

CRN_RD_HD float rd_dot(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

CRN_RD_HD void rd_normalize(float* v) {
  const float l = sqrtf(rd_dot(v, v));
  v[0] = v[0] / l; v[1] = v[1] / l; v[2] = v[2] / l;
}

CRN_RD_HD void rd_cross(const float* a, const float* b, float* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

CRN_RD_HD uint8_t rd_u8(float c) { return (uint8_t)rintf(fminf(fmaxf(c, 0.f), 1.f) * 255.f); }

// point_light_illumination.frag for the winning triangle at a pixel.  p: 9 positions, nrm: the triangle's 9 normals
// (mode 1: per vertex, normalised here as triangle_renderer.geom does; mode 2: flat, nrm[0..2]) or unused (mode 0:
// the geometric normal), mat: ambient 3, diffuse 3, specular 3, shininess (NULL: black).
CRN_RD_HD void rd_shade(const crnRenderImage& im, const float* p, const float* nrm, const float* mat, const float E[3],
                        uint8_t* out) {
  if (!mat) {
    out[0] = out[1] = out[2] = 0;
    return;
  }
  const float s = (E[0] + E[1]) + E[2];
  float pos[3], n[3];
  for (int q = 0; q < 3; ++q) pos[q] = ((E[0] * p[q] + E[1] * p[3 + q]) + E[2] * p[6 + q]) / s;
  if (im.normal_mode == 1) {
    float nk[3][3];
    for (int k = 0; k < 3; ++k) {
      for (int q = 0; q < 3; ++q) nk[k][q] = nrm[3 * k + q];
      rd_normalize(nk[k]);
    }
    for (int q = 0; q < 3; ++q) n[q] = ((E[0] * nk[0][q] + E[1] * nk[1][q]) + E[2] * nk[2][q]) / s;
  } else if (im.normal_mode == 2) {
    for (int q = 0; q < 3; ++q) n[q] = nrm[q];
  } else {
    float e1[3], e2[3];
    for (int q = 0; q < 3; ++q) {
      e1[q] = p[3 + q] - p[q];
      e2[q] = p[6 + q] - p[q];
    }
    rd_normalize(e1);
    rd_normalize(e2);
    rd_cross(e1, e2, n);
    rd_normalize(n);
  }
  float L[3], V[3], R[3];
  rd_normalize(n);
  for (int q = 0; q < 3; ++q) {
    L[q] = im.light[q] - pos[q];
    V[q] = im.cam[q] - pos[q];
  }
  rd_normalize(L);
  rd_normalize(V);
  for (int q = 0; q < 3; ++q) V[q] = -V[q];
  const float dNL = rd_dot(L, n);
  const float k2 = 2.f * rd_dot(n, L);
  for (int q = 0; q < 3; ++q) R[q] = L[q] - k2 * n[q];
  const float dRV = rd_dot(R, V);
  const float sp = powf(fmaxf(dRV, 0.f), mat[9]);
  for (int q = 0; q < 3; ++q) {
    const float d = (mat[3 + q] * fabsf(dNL)) * im.light_color[q] + im.ambient_light[q] * mat[3 + q];
    const float sc = (mat[6 + q] * im.light_color[q]) * sp;
    out[q] = rd_u8((mat[q] + d) + sc);
  }
}

// ---------------- diffuse textures (point_light_illumination.frag: diffuse * texture(textures, (s, t, layer))) --------
// GL's rule for the array the reference binds: GL_LINEAR both ways, no mip-maps, GL_REPEAT, unsigned-normalised bytes.
// One axis of n texels at coordinate s:  s' = s - floorf(s), and s' = 0 unless 0 <= s' < 1 (NaN, infinity, a rounding to
// 1); u = s' * n - 0.5 in [-0.5, n - 0.5); i0 = floorf(u), weight a = u - i0 of i1 = i0 + 1; i0 = -1 wraps to n - 1 and
// i1 = n to 0.  Both indices are in [0, n) for every s and every n >= 1 (the clamp below never acts for n <= 2^14; it
// makes that independent of the rounding argument).
CRN_RD_HD void rd_tex_axis(float s, int n, int& i0, int& i1, float& a) {
  float f = s - floorf(s);
  if (!(f >= 0.f && f < 1.f)) f = 0.f;
  const float u = f * (float)n - 0.5f;
  const float fl = floorf(u);
  a = u - fl;
  i0 = rd_clampi((int)fl, -1, n - 1);
  i1 = i0 + 1;
  if (i0 < 0) i0 = n - 1;
  if (i1 >= n) i1 = 0;
}

// tex: RGBA8 texels as little-endian words [L][Ht][Wt] (R in the low byte, alpha ignored), row 0 is t = 0.  The caller
// guarantees 0 <= layer < L.  A channel is byte / 255.f; the four texels are blended as two lerps along s and one along
// t, each written x + w * (y - x):  top = c00 + a (c10 - c00), bot = c01 + a (c11 - c01), tau = top + b (bot - top)
// (c_ij: column i_, row j_).  That is the bilinear blend with weights (1-a)(1-b), a(1-b), (1-a)b, ab, in an order that
// returns equal texels unchanged: an all-255 texture gives tau == 1.0f exactly.
CRN_RD_HD void rd_tex_fetch(const uint32_t* tex, int Ht, int Wt, int layer, float s, float t, float tau[3]) {
  int i0, i1, j0, j1;
  float a, b;
  rd_tex_axis(s, Wt, i0, i1, a);
  rd_tex_axis(t, Ht, j0, j1, b);
  const uint32_t* r0 = tex + ((int64_t)layer * Ht + j0) * Wt;
  const uint32_t* r1 = tex + ((int64_t)layer * Ht + j1) * Wt;
  const uint32_t w00 = r0[i0], w10 = r0[i1], w01 = r1[i0], w11 = r1[i1];
  for (int q = 0; q < 3; ++q) {
    const float c00 = (float)((w00 >> (8 * q)) & 255u) / 255.f, c10 = (float)((w10 >> (8 * q)) & 255u) / 255.f;
    const float c01 = (float)((w01 >> (8 * q)) & 255u) / 255.f, c11 = (float)((w11 >> (8 * q)) & 255u) / 255.f;
    const float top = c00 + a * (c10 - c00), bot = c01 + a * (c11 - c01);
    tau[q] = top + b * (bot - top);
  }
}

// The texture arguments of a render call (contract: include/corenet_hip.h); texels == NULL: nothing is textured.
struct crnRdTex {
  const float* uv;          // [T][3][2] or NULL (all zero)
  const int32_t* ids;       // [M]
  const uint32_t* texels;   // RGBA8 words [L][Ht][Wt]
  int L, Ht, Wt;
};

// L, Ht, Wt of a texture array the entry points accept (2^14 per side, like an image: n and s' * n are exact floats)
CRN_RD_HD bool rd_tex_dims_ok(int L, int Ht, int Wt) {
  return L >= 1 && Ht >= 1 && Wt >= 1 && L <= (1 << 14) && Ht <= (1 << 14) && Wt <= (1 << 14);
}

// The textured material of the winning fragment: (s, t) interpolated like position from the triangle's 6 texture
// coordinates uv (NULL: all zero), then mat's diffuse colour (mat[3..5]) times tau.  The rest of rd_shade is unchanged.
CRN_RD_HD void rd_tex_diffuse(const float E[3], const float* uv, const uint32_t* tex, int Ht, int Wt, int layer,
                              float* mat) {
  float st[2] = {0.f, 0.f};
  if (uv) {
    const float s = (E[0] + E[1]) + E[2];
    for (int q = 0; q < 2; ++q) st[q] = ((E[0] * uv[q] + E[1] * uv[2 + q]) + E[2] * uv[4 + q]) / s;
  }
  float tau[3];
  rd_tex_fetch(tex, Ht, Wt, layer, st[0], st[1], tau);
  for (int q = 0; q < 3; ++q) mat[3 + q] = mat[3 + q] * tau[q];
}

// ---------------- voxel faces (voxel_renderer.geom) ----------------
// A label is drawn iff it indexes the palette and its colour has no negative channel.
CRN_RD_HD bool vx_drawn(int32_t l, const float* pal, int P) {
  if (l < 0 || l >= P) return false;
  return !(pal[3 * l] < 0.f || pal[3 * l + 1] < 0.f || pal[3 * l + 2] < 0.f);
}

CRN_RD_HD bool vx_drawn_at(const int32_t* g, int D, int H, int W, int z, int y, int x, const float* pal, int P) {
  if (z < 0 || z >= D || y < 0 || y >= H || x < 0 || x >= W) return false;
  return vx_drawn(g[((int64_t)z * H + y) * W + x], pal, P);
}

// Exposed faces of voxel (z, y, x) as a bit mask over the order +x, -x, +y, -y, +z, -z (0 if the voxel is not drawn).
CRN_RD_HD int vx_faces(const int32_t* g, int D, int H, int W, int z, int y, int x, const float* pal, int P) {
  if (!vx_drawn(g[((int64_t)z * H + y) * W + x], pal, P)) return 0;
  int m = 0;
  m |= !vx_drawn_at(g, D, H, W, z, y, x + 1, pal, P) << 0;
  m |= !vx_drawn_at(g, D, H, W, z, y, x - 1, pal, P) << 1;
  m |= !vx_drawn_at(g, D, H, W, z, y + 1, x, pal, P) << 2;
  m |= !vx_drawn_at(g, D, H, W, z, y - 1, x, pal, P) << 3;
  m |= !vx_drawn_at(g, D, H, W, z + 1, y, x, pal, P) << 4;
  m |= !vx_drawn_at(g, D, H, W, z - 1, y, x, pal, P) << 5;
  return m;
}

CRN_RD_HD int vx_popc(int m) {
  int c = 0;
  for (int f = 0; f < 6; ++f) c += (m >> f) & 1;
  return c;
}

// emit_quad(center, dy, dx) of face f of voxel (z, y, x) through m (row-major 4x4, no homogeneous divide as in the
// shader): two triangles (v0, v1, v2), (v2, v1, v3) -> tri[18], the flat normal normalize(cross(dx', dy')) -> n[3].
CRN_RD_HD void vx_quad(const float* m, int z, int y, int x, int f, float* tri, float* n) {
  float c[3] = {(float)x + 0.5f, (float)y + 0.5f, (float)z + 0.5f};
  const int axis = f >> 1;
  c[axis] = (f & 1) ? c[axis] - 0.5f : c[axis] + 0.5f;
  // (dy, dx) axes of the quad per face, voxel_renderer.geom
  const int ay[6] = {1, 2, 2, 0, 0, 1}, ax[6] = {2, 1, 0, 2, 1, 0};
  float dyv[3] = {0.f, 0.f, 0.f}, dxv[3] = {0.f, 0.f, 0.f};
  dyv[ay[f]] = 0.5f;
  dxv[ax[f]] = 0.5f;
  float cc[3], dx[3], dy[3];
  for (int r = 0; r < 3; ++r) {
    cc[r] = ((m[4 * r] * c[0] + m[4 * r + 1] * c[1]) + m[4 * r + 2] * c[2]) + m[4 * r + 3];
    dx[r] = (m[4 * r] * dxv[0] + m[4 * r + 1] * dxv[1]) + m[4 * r + 2] * dxv[2];
    dy[r] = (m[4 * r] * dyv[0] + m[4 * r + 1] * dyv[1]) + m[4 * r + 2] * dyv[2];
  }
  rd_cross(dx, dy, n);
  rd_normalize(n);
  float v[4][3];
  for (int q = 0; q < 3; ++q) {
    v[0][q] = cc[q] + (dx[q] - dy[q]);
    v[1][q] = cc[q] + (-dx[q] - dy[q]);
    v[2][q] = cc[q] + (dx[q] + dy[q]);
    v[3][q] = cc[q] + (-dx[q] + dy[q]);
  }
  const int order[6] = {0, 1, 2, 2, 1, 3};
  for (int k = 0; k < 6; ++k)
    for (int q = 0; q < 3; ++q) tri[3 * k + q] = v[order[k]][q];
}

// transform_points of voxel centre (x + 0.5, y + 0.5, z + 0.5) with the homogeneous divide
CRN_RD_HD void vx_centre(const float* m, int z, int y, int x, float* o) {
  float h[4];
  rd_xform4(m, (float)x + 0.5f, (float)y + 0.5f, (float)z + 0.5f, h);
  o[0] = h[0] / h[3]; o[1] = h[1] / h[3]; o[2] = h[2] / h[3];
}

// order-preserving float <-> int32 key (min / max of keys == min / max of the floats; NaN is never fed)
CRN_RD_HD int32_t vx_key(float f) {
  union { float f; int32_t i; } u;
  u.f = f;
  return u.i >= 0 ? u.i : u.i ^ 0x7fffffff;
}
CRN_RD_HD float vx_unkey(int32_t k) {
  union { float f; int32_t i; } u;
  u.i = k >= 0 ? k : k ^ 0x7fffffff;
  return u.f;
}
