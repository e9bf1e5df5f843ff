// Mesh clean-up on the host: the twin of mesh_ops.hip, part of the product library.  Same contract (include/corenet_hip.h,
// DESIGN section 24) and the same outputs bit for bit: the formulas are those of mesh_ops_common.h, the sums run in list
// order, the clustering sums are exact integers.  Plain sequential loops: faces in ascending order fill every corner list
// in ascending order, so nothing needs sorting but the candidate lists (std::sort), and the lowest vertex of a cluster is
// the first one met.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/corenet_hip.h"
#include "mesh_ops_common.h"

namespace {

bool sizes_ok(int64_t F, int N, int64_t V) { return F >= 0 && N >= 0 && V >= 0 && V <= INT32_MAX && F <= INT32_MAX / 3; }

}  // namespace

extern "C" int crn_mesh_topology_cpu(const int32_t* faces, int64_t F, const int64_t* voff, const int64_t* foff, int N, int64_t V,
                                     int64_t* vf_offsets, int32_t* vf_corners, int64_t* vv_offsets, int32_t* vv_neighbours,
                                     uint8_t* irregular, int64_t* counts) {
  if (!sizes_ok(F, N, V) || !voff || !foff || !vf_offsets || !vv_offsets || !counts) return CRN_EINVAL;
  if ((V && !irregular) || (F && (!faces || !vf_corners))) return CRN_EINVAL;
  int64_t bad = 0;
  std::vector<uint8_t> good((size_t)F, 0);
  for (int64_t v = 0; v <= V; ++v) vf_offsets[v] = 0;
  for (int64_t f = 0; f < F; ++f) {
    int64_t g[3];
    int nbad;
    good[f] = mo_face_ids(faces, f, voff, foff, N, V, g, &nbad);
    bad += nbad;
    if (good[f])
      for (int c = 0; c < 3; ++c) ++vf_offsets[g[c] + 1];
  }
  for (int64_t v = 0; v < V; ++v) vf_offsets[v + 1] += vf_offsets[v];
  std::vector<int64_t> cursor(vf_offsets, vf_offsets + V);
  for (int64_t f = 0; f < F; ++f) {
    if (!good[f]) continue;
    int64_t g[3];
    int nbad;
    mo_face_ids(faces, f, voff, foff, N, V, g, &nbad);
    for (int c = 0; c < 3; ++c) vf_corners[cursor[g[c]]++] = (int32_t)(3 * f + c);
  }
  std::vector<uint32_t> cand;
  vv_offsets[0] = 0;
  for (int64_t v = 0; v < V; ++v) {
    cand.clear();
    for (int64_t i = vf_offsets[v]; i < vf_offsets[v + 1]; ++i) {
      const int64_t f = vf_corners[i] / 3;
      const int c = vf_corners[i] % 3;
      const int64_t base = voff[mo_object(foff, N, f)];
      cand.push_back((uint32_t)(2 * (base + faces[3 * f + (c + 1) % 3])));
      cand.push_back((uint32_t)(2 * (base + faces[3 * f + (c + 2) % 3]) + 1));
    }
    std::sort(cand.begin(), cand.end());
    bool irr = false;
    int64_t k = 0;
    size_t i = 0;
    while (i < cand.size()) {
      const uint32_t w = cand[i] >> 1;
      int nout = 0, nin = 0;
      for (; i < cand.size() && (cand[i] >> 1) == w; ++i) {
        if (cand[i] & 1u) ++nin; else ++nout;
      }
      if ((int64_t)w == v) { irr = true; continue; }
      if (vv_neighbours) vv_neighbours[vv_offsets[v] + k] = (int32_t)w;
      ++k;
      irr = irr || nout != 1 || nin != 1;
    }
    irregular[v] = irr;
    vv_offsets[v + 1] = vv_offsets[v] + k;
  }
  counts[0] = vv_offsets[V];
  counts[1] = bad;
  return CRN_OK;
}

extern "C" int crn_mesh_smooth_step_cpu(const float* vin, float* vout, const int64_t* vv_offsets, const int32_t* vv, const uint8_t* fixed,
                                        float factor, int64_t V) {
  if (V < 0 || V > INT32_MAX || (V && (!vin || !vout || !vv_offsets || vin == vout))) return CRN_EINVAL;
  for (int64_t v = 0; v < V; ++v) {
    const int64_t o0 = vv_offsets[v], o1 = vv_offsets[v + 1];
    if (o1 == o0 || (fixed && fixed[v])) {
      for (int a = 0; a < 3; ++a) vout[3 * v + a] = vin[3 * v + a];
      continue;
    }
    const int k = (int)(o1 - o0);
    for (int a = 0; a < 3; ++a) {
      float s = vin[3 * (int64_t)vv[o0] + a];
      for (int64_t i = o0 + 1; i < o1; ++i) s = s + vin[3 * (int64_t)vv[i] + a];
      vout[3 * v + a] = mo_smooth(vin[3 * v + a], s, k, factor);
    }
  }
  return CRN_OK;
}

extern "C" int crn_mesh_face_normals_cpu(const float* vertices, const int32_t* faces, int64_t F, const int64_t* voff, const int64_t* foff,
                                         int N, int64_t V, float* out) {
  if (!sizes_ok(F, N, V) || !voff || !foff || (F && (!faces || !out)) || (F && V && !vertices)) return CRN_EINVAL;
  for (int64_t f = 0; f < F; ++f) {
    int64_t g[3];
    int nbad;
    float n[3] = {0.f, 0.f, 0.f};
    if (mo_face_ids(faces, f, voff, foff, N, V, g, &nbad)) mo_cross(vertices + 3 * g[0], vertices + 3 * g[1], vertices + 3 * g[2], n);
    for (int a = 0; a < 3; ++a) out[3 * f + a] = n[a];
  }
  return CRN_OK;
}

extern "C" int crn_mesh_vertex_normals_cpu(const float* vertices, const int32_t* faces, int64_t F, const int64_t* voff, int N, int64_t V,
                                           const int64_t* vf_offsets, const int32_t* vf_corners, float* out) {
  if (!sizes_ok(F, N, V) || !voff || (V && (!vertices || !vf_offsets || !out)) || (F && !faces)) return CRN_EINVAL;
  for (int64_t v = 0; v < V; ++v) {
    const int n = mo_object(voff, N, v);
    float s[3] = {0.f, 0.f, 0.f}, r[3] = {0.f, 0.f, 0.f};
    if (n < N) {
      const int64_t base = voff[n], nv = voff[n + 1] - base;
      for (int64_t i = vf_offsets[v]; i < vf_offsets[v + 1]; ++i) {
        const int64_t f = (uint32_t)vf_corners[i] / 3u;
        if (f >= F) continue;
        const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        if (a < 0 || a >= nv || b < 0 || b >= nv || c < 0 || c >= nv) continue;
        float x[3];
        mo_cross(vertices + 3 * (base + a), vertices + 3 * (base + b), vertices + 3 * (base + c), x);
        for (int d = 0; d < 3; ++d) s[d] = s[d] + x[d];
      }
      mo_normalise(s, r);
    }
    for (int d = 0; d < 3; ++d) out[3 * v + d] = r[d];
  }
  return CRN_OK;
}

extern "C" int crn_mesh_cluster_cpu(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const int64_t* voff,
                                    const int64_t* foff, int N, float cell, int32_t* vertex_map, int64_t* counts, float* new_vertices,
                                    int32_t* cluster_size, int32_t* new_faces) {
  if (!sizes_ok(F, N, V) || V > CRN_MESH_CLUSTER_MAX_VERTICES || N > CRN_MESH_MAX_OBJECTS || !(cell > 0.f) || !voff || !foff || !counts)
    return CRN_EINVAL;
  if ((V && (!vertices || !vertex_map)) || (F && !faces)) return CRN_EINVAL;
  if (new_vertices && !cluster_size) return CRN_EINVAL;
  for (int i = 0; i <= 2 * N; ++i) counts[i] = 0;
  int64_t bad = 0;
  const int log2 = mo_table_log2(V);
  const uint32_t mask = (uint32_t)(((uint64_t)1 << log2) - 1);
  std::vector<uint64_t> keys((size_t)1 << log2, MO_EMPTY_KEY);
  std::vector<int32_t> ids((size_t)1 << log2, -1);                          // the new global id of the slot's cluster
  std::vector<int32_t> cells;                                              // per new vertex its three cell indices
  std::vector<int64_t> sums;
  std::vector<int32_t> size;
  for (int64_t v = 0; v < V; ++v) {
    const int n = mo_object(voff, N, v);
    int32_t c[3];
    int64_t u[3];
    if (n >= N || !mo_cells(vertices + 3 * v, cell, c, u)) {
      vertex_map[v] = -1;
      ++bad;
      continue;
    }
    const uint64_t key = mo_key(n, c);
    uint32_t slot = mo_hash(key, log2);
    while (keys[slot] != MO_EMPTY_KEY && keys[slot] != key) slot = (slot + 1) & mask;
    if (keys[slot] == MO_EMPTY_KEY) {                                      // v is the cluster's lowest vertex
      keys[slot] = key;
      ids[slot] = (int32_t)size.size();
      size.push_back(0);
      for (int a = 0; a < 3; ++a) { cells.push_back(c[a]); sums.push_back(0); }
      ++counts[n];
    }
    const int32_t id = ids[slot];
    vertex_map[v] = id;
    ++size[id];
    for (int a = 0; a < 3; ++a) sums[3 * (size_t)id + a] += u[a];
  }
  if (new_vertices)
    for (size_t id = 0; id < size.size(); ++id) {
      cluster_size[id] = size[id];
      for (int a = 0; a < 3; ++a) new_vertices[3 * id + a] = mo_position(cells[3 * id + a], sums[3 * id + a], size[id], cell);
    }
  std::vector<int64_t> new_voff((size_t)N + 1, 0);
  for (int n = 0; n < N; ++n) new_voff[n + 1] = new_voff[n] + counts[n];
  int64_t at = 0;
  for (int64_t f = 0; f < F; ++f) {
    int64_t g[3];
    int nbad;
    if (!mo_face_ids(faces, f, voff, foff, N, V, g, &nbad)) { bad += nbad; continue; }
    const int32_t a = vertex_map[g[0]], b = vertex_map[g[1]], c = vertex_map[g[2]];
    if (a < 0 || b < 0 || c < 0 || a == b || b == c || a == c) continue;
    const int n = mo_object(foff, N, f);
    ++counts[N + n];
    if (new_faces) {
      new_faces[3 * at] = (int32_t)(a - new_voff[n]);
      new_faces[3 * at + 1] = (int32_t)(b - new_voff[n]);
      new_faces[3 * at + 2] = (int32_t)(c - new_voff[n]);
    }
    ++at;
  }
  counts[2 * N] = bad;
  return CRN_OK;
}
