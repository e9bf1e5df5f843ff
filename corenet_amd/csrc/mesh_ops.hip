// Mesh clean-up on gfx950 (corenet_amd.mesh_ops): vertex / face incidence tables, Taubin smoothing, area-weighted
// normals and vertex clustering of batches of indexed meshes.  Contract: include/corenet_hip.h and DESIGN section 24; host
// twin: mesh_ops_cpu.cpp (identical outputs: integer atomics, per-list sorts and float32 sums in list order only).
//
// Every kernel is one thread per item (face, vertex, corner slot) with MO_THREADS threads per workgroup, no workgroup
// waits for another one, and every loop is bounded by a list length or the table size.  The prefix sums between the
// launches are the caller's (torch.cumsum).
//   * incidence: mo_count adds the corners of every face to its vertices' counters (integer atomics), mo_fill hands every
//     corner a slot of its vertex's list through an atomic cursor, so the order inside a list is arbitrary, and
//     mo_sort makes it ascending.  mo_candidates writes, per sorted corner, the next and the previous vertex of its face
//     (2 w + direction), mo_sort orders those per vertex as well, and mo_vv_count / mo_vv_fill read the distinct
//     neighbours and the regularity of every edge off the sorted list in one linear walk per vertex.
//   * mo_sort: a list of up to CRN_MESH_SORT_LANE keys is sorted by its own lane in a private array.  Longer lists are
//     collected in LDS and sorted by the whole workgroup one after the other, rank by counting: a thread holds one key,
//     the list passes through LDS in tiles of CRN_MESH_SORT_TILE keys, and the thread counts the keys in front of its own
//     (equal keys: the one with the lower index comes first, so every rank is taken once).
//   * clustering: mo_cluster_keys inserts every vertex's (object, cell) key into an open-addressing table (atomicCAS on
//     the key, linear probing) and atomicMin's its id into the slot's leader.  Everything after that goes through the
//     leader, never through the slot: flags, the prefix sum over them (new ids in the order of the leaders), 64-bit integer
//     sums of the 20-bit offsets, positions in float64 from the exact sums.
#include "crn_common.h"
#include "mesh_ops_common.h"

namespace {

constexpr int MO_THREADS = CRN_MESH_THREADS;
constexpr int MO_LANE = CRN_MESH_SORT_LANE;
constexpr int MO_TILE = CRN_MESH_SORT_TILE;
static_assert(MO_THREADS % 64 == 0 && MO_TILE % MO_THREADS == 0, "whole waves, whole passes over a tile");

__device__ __forceinline__ int64_t mo_item() { return (int64_t)blockIdx.x * MO_THREADS + threadIdx.x; }

inline dim3 mo_grid(int64_t items) { return dim3((unsigned)((items + MO_THREADS - 1) / MO_THREADS)); }

// ---- incidence ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MO_THREADS) void mo_count(const int32_t* __restrict__ faces, int64_t F, const int64_t* __restrict__ voff,
                                                       const int64_t* __restrict__ foff, int N, int64_t V, int32_t* deg, int64_t* bad) {
  const int64_t f = mo_item();
  if (f >= F) return;
  int64_t g[3];
  int nbad;
  if (!mo_face_ids(faces, f, voff, foff, N, V, g, &nbad)) {                // a face with a bad id is in no list
    atomicAdd(reinterpret_cast<unsigned long long*>(bad), (unsigned long long)nbad);
    return;
  }
  for (int c = 0; c < 3; ++c) atomicAdd(deg + g[c], 1);
}

__global__ __launch_bounds__(MO_THREADS) void mo_fill(const int32_t* __restrict__ faces, int64_t F, const int64_t* __restrict__ voff,
                                                      const int64_t* __restrict__ foff, int N, int64_t V,
                                                      const int64_t* __restrict__ vf_offsets, int32_t* cursor, uint32_t* vf_tmp) {
  const int64_t f = mo_item();
  if (f >= F) return;
  int64_t g[3];
  int nbad;
  if (!mo_face_ids(faces, f, voff, foff, N, V, g, &nbad)) return;
  for (int c = 0; c < 3; ++c) {
    const int32_t at = atomicAdd(cursor + g[c], 1);                        // < the count mo_count took for this vertex
    vf_tmp[vf_offsets[g[c]] + at] = (uint32_t)(3 * f + c);
  }
}

// Segment v of `in` is [mul * offsets[v], mul * offsets[v + 1]); out <- every segment ascending.
__global__ __launch_bounds__(MO_THREADS) void mo_sort(const int64_t* __restrict__ offsets, int mul, int64_t V,
                                                      const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  __shared__ uint32_t tile[MO_TILE];
  __shared__ int64_t longs[MO_THREADS];
  __shared__ int nlong;
  if (threadIdx.x == 0) nlong = 0;
  __syncthreads();                                                         // every thread of the workgroup arrives: no return above
  const int64_t v = mo_item();
  if (v < V) {
    const int64_t o0 = offsets[v] * mul, n = (offsets[v + 1] - offsets[v]) * mul;
    if (n > MO_LANE) {
      longs[atomicAdd(&nlong, 1)] = v;
    } else if (n > 0) {
      uint32_t k[MO_LANE];
      for (int i = 0; i < (int)n; ++i) {                                   // insertion sort
        const uint32_t x = in[o0 + i];
        int j = i;
        for (; j > 0 && k[j - 1] > x; --j) k[j] = k[j - 1];
        k[j] = x;
      }
      for (int i = 0; i < (int)n; ++i) out[o0 + i] = k[i];
    }
  }
  __syncthreads();
  const int count = nlong;                                                 // the same in every thread from here on
  for (int q = 0; q < count; ++q) {
    const int64_t lv = longs[q];
    const int64_t o0 = offsets[lv] * mul, n = (offsets[lv + 1] - offsets[lv]) * mul;
    const bool one_tile = n <= MO_TILE;
    for (int64_t ib = 0; ib < n; ib += MO_THREADS) {
      const int64_t i = ib + threadIdx.x;
      const bool active = i < n;
      const uint32_t key = active ? in[o0 + i] : 0u;
      int64_t rank = 0;
      for (int64_t t0 = 0; t0 < n; t0 += MO_TILE) {
        const int m = (int)(n - t0 < MO_TILE ? n - t0 : MO_TILE);
        if (!one_tile || ib == 0) {                                        // a list of one tile stays in LDS
          __syncthreads();
          for (int j = threadIdx.x; j < m; j += MO_THREADS) tile[j] = in[o0 + t0 + j];
          __syncthreads();
        }
        if (active) {
          int before = 0;
          for (int j = 0; j < m; ++j) {
            const uint32_t kj = tile[j];                                   // one address for the wave: a broadcast
            before += (kj < key) | ((kj == key) & (t0 + j < i));
          }
          rank += before;
        }
      }
      if (active) out[o0 + rank] = key;
    }
    __syncthreads();                                                       // the next list overwrites the tile
  }
}

// Slot s of the sorted corner lists -> the next and the previous vertex of that corner's face, as 2 w + direction
// (0: the edge leaves the list's vertex, 1: it arrives).
__global__ __launch_bounds__(MO_THREADS) void mo_candidates(const int32_t* __restrict__ faces, const int64_t* __restrict__ voff,
                                                            const int64_t* __restrict__ foff, int N, int64_t F, int64_t V,
                                                            const int64_t* __restrict__ vf_offsets, const uint32_t* __restrict__ vf_corners,
                                                            uint32_t* __restrict__ cand) {
  const int64_t s = mo_item();
  if (s >= 3 * F || s >= vf_offsets[V]) return;
  const uint32_t code = vf_corners[s];
  const int64_t f = code / 3u;
  const int c = (int)(code % 3u);
  const int n = mo_object(foff, N, f);                                     // a listed face has an object and good ids
  const int64_t base = voff[n];
  cand[2 * s] = (uint32_t)(2 * (base + faces[3 * f + (c + 1) % 3]));
  cand[2 * s + 1] = (uint32_t)(2 * (base + faces[3 * f + (c + 2) % 3]) + 1);
}

// One walk over the sorted candidates of vertex v: k distinct neighbours w != v, handed to `emit` in ascending order;
// returns whether an edge of v is not regular (a -> b and b -> a exactly once each; a self edge never is).
template <typename Emit>
__device__ __forceinline__ bool mo_walk(const uint32_t* __restrict__ cand, int64_t s0, int64_t s1, int64_t v, int32_t* k, Emit emit) {
  bool irregular = false;
  int32_t kk = 0;
  int64_t i = s0;
  while (i < s1) {
    const uint32_t w = cand[i] >> 1;
    int nout = 0, nin = 0;
    for (; i < s1 && (cand[i] >> 1) == w; ++i) {
      if (cand[i] & 1u) ++nin; else ++nout;
    }
    if ((int64_t)w == v) { irregular = true; continue; }
    emit(kk, w);
    ++kk;
    irregular = irregular || nout != 1 || nin != 1;
  }
  *k = kk;
  return irregular;
}

__global__ __launch_bounds__(MO_THREADS) void mo_vv_count(const uint32_t* __restrict__ cand, const int64_t* __restrict__ vf_offsets, int64_t V,
                                                          int32_t* __restrict__ vvdeg, uint8_t* __restrict__ irregular) {
  const int64_t v = mo_item();
  if (v >= V) return;
  int32_t k;
  irregular[v] = mo_walk(cand, 2 * vf_offsets[v], 2 * vf_offsets[v + 1], v, &k, [](int32_t, uint32_t) {});
  vvdeg[v] = k;
}

__global__ __launch_bounds__(MO_THREADS) void mo_vv_fill(const uint32_t* __restrict__ cand, const int64_t* __restrict__ vf_offsets,
                                                         const int64_t* __restrict__ vv_offsets, int64_t V, int32_t* __restrict__ vv) {
  const int64_t v = mo_item();
  if (v >= V) return;
  int32_t k;
  int32_t* dst = vv + vv_offsets[v];
  mo_walk(cand, 2 * vf_offsets[v], 2 * vf_offsets[v + 1], v, &k, [dst](int32_t at, uint32_t w) { dst[at] = (int32_t)w; });
}

// ---- smoothing and normals ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MO_THREADS) void mo_smooth_step(const float* __restrict__ vin, float* __restrict__ vout,
                                                             const int64_t* __restrict__ vv_offsets, const int32_t* __restrict__ vv,
                                                             const uint8_t* __restrict__ fixed, float factor, int64_t V) {
  const int64_t v = mo_item();
  if (v >= V) return;
  const int64_t o0 = vv_offsets[v], o1 = vv_offsets[v + 1];
  const float x = vin[3 * v], y = vin[3 * v + 1], z = vin[3 * v + 2];
  if (o1 == o0 || (fixed && fixed[v])) {
    vout[3 * v] = x; vout[3 * v + 1] = y; vout[3 * v + 2] = z;
    return;
  }
  const float* p = vin + 3 * (int64_t)vv[o0];
  float sx = p[0], sy = p[1], sz = p[2];
  for (int64_t i = o0 + 1; i < o1; ++i) {
    p = vin + 3 * (int64_t)vv[i];
    sx = sx + p[0]; sy = sy + p[1]; sz = sz + p[2];
  }
  const int k = (int)(o1 - o0);
  vout[3 * v] = mo_smooth(x, sx, k, factor);
  vout[3 * v + 1] = mo_smooth(y, sy, k, factor);
  vout[3 * v + 2] = mo_smooth(z, sz, k, factor);
}

__global__ __launch_bounds__(MO_THREADS) void mo_face_normals(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int64_t F,
                                                              const int64_t* __restrict__ voff, const int64_t* __restrict__ foff, int N,
                                                              int64_t V, float* __restrict__ out) {
  const int64_t f = mo_item();
  if (f >= F) return;
  int64_t g[3];
  int nbad;
  float n[3] = {0.f, 0.f, 0.f};
  if (mo_face_ids(faces, f, voff, foff, N, V, g, &nbad)) mo_cross(vertices + 3 * g[0], vertices + 3 * g[1], vertices + 3 * g[2], n);
  out[3 * f] = n[0]; out[3 * f + 1] = n[1]; out[3 * f + 2] = n[2];
}

__global__ __launch_bounds__(MO_THREADS) void mo_vertex_normals(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int64_t F,
                                                                const int64_t* __restrict__ voff, int N, int64_t V,
                                                                const int64_t* __restrict__ vf_offsets, const uint32_t* __restrict__ vf_corners,
                                                                float* __restrict__ out) {
  const int64_t v = mo_item();
  if (v >= V) return;
  const int n = mo_object(voff, N, v);                                     // a vertex and its faces share their object
  float s[3] = {0.f, 0.f, 0.f}, r[3] = {0.f, 0.f, 0.f};
  if (n < N) {
    const int64_t base = voff[n], nv = voff[n + 1] - base;
    for (int64_t i = vf_offsets[v]; i < vf_offsets[v + 1]; ++i) {
      const int64_t f = vf_corners[i] / 3u;
      if (f >= F) continue;
      const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
      if (a < 0 || a >= nv || b < 0 || b >= nv || c < 0 || c >= nv) continue;      // lists of other faces than these: nothing is read
      float x[3];
      mo_cross(vertices + 3 * (base + a), vertices + 3 * (base + b), vertices + 3 * (base + c), x);
      s[0] = s[0] + x[0]; s[1] = s[1] + x[1]; s[2] = s[2] + x[2];
    }
    mo_normalise(s, r);
  }
  out[3 * v] = r[0]; out[3 * v + 1] = r[1]; out[3 * v + 2] = r[2];
}

// ---- clustering --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MO_THREADS) void mo_cluster_keys(const float* __restrict__ vertices, int64_t V, const int64_t* __restrict__ voff,
                                                              int N, float cell, unsigned long long* keys, int32_t* leader, int log2,
                                                              int32_t* __restrict__ slot_of, int64_t* bad) {
  const int64_t v = mo_item();
  if (v >= V) return;
  const int n = mo_object(voff, N, v);
  int32_t c[3];
  int64_t u[3];
  if (n >= N || !mo_cells(vertices + 3 * v, cell, c, u)) {
    slot_of[v] = MO_NO_SLOT;
    atomicAdd(reinterpret_cast<unsigned long long*>(bad), 1ull);
    return;
  }
  const unsigned long long key = mo_key(n, c);
  const uint32_t mask = (uint32_t)(((uint64_t)1 << log2) - 1);
  uint32_t slot = mo_hash(key, log2);
  int32_t found = MO_NO_SLOT;
  for (uint64_t trip = 0; trip <= mask; ++trip) {                          // at most V of the >= 2 V slots are ever taken
    const unsigned long long prev = atomicCAS(keys + slot, (unsigned long long)MO_EMPTY_KEY, key);
    if (prev == MO_EMPTY_KEY || prev == key) { found = (int32_t)slot; break; }
    slot = (slot + 1) & mask;
  }
  slot_of[v] = found;
  if (found >= 0) atomicMin(leader + found, (int32_t)v);
  else atomicAdd(reinterpret_cast<unsigned long long*>(bad), 1ull);
}

__global__ __launch_bounds__(MO_THREADS) void mo_cluster_vflag(const int32_t* __restrict__ leader, const int32_t* __restrict__ slot_of, int64_t V,
                                                               int32_t* __restrict__ vflag) {
  const int64_t v = mo_item();
  if (v >= V) return;
  const int32_t s = slot_of[v];
  vflag[v] = s >= 0 && leader[s] == (int32_t)v;
}

__global__ __launch_bounds__(MO_THREADS) void mo_cluster_fflag(const int32_t* __restrict__ faces, int64_t F, const int64_t* __restrict__ voff,
                                                               const int64_t* __restrict__ foff, int N, int64_t V,
                                                               const int32_t* __restrict__ leader, const int32_t* __restrict__ slot_of,
                                                               int32_t* __restrict__ fkeep, int64_t* bad) {
  const int64_t f = mo_item();
  if (f >= F) return;
  int64_t g[3];
  int nbad;
  int32_t keep = 0;
  if (!mo_face_ids(faces, f, voff, foff, N, V, g, &nbad)) {
    atomicAdd(reinterpret_cast<unsigned long long*>(bad), (unsigned long long)nbad);
  } else {
    const int32_t s0 = slot_of[g[0]], s1 = slot_of[g[1]], s2 = slot_of[g[2]];
    if (s0 >= 0 && s1 >= 0 && s2 >= 0) {
      const int32_t a = leader[s0], b = leader[s1], c = leader[s2];
      keep = a != b && b != c && a != c;
    }
  }
  fkeep[f] = keep;
}

// vcs: the inclusive prefix sum of vflag, so a leader L has the new id vcs[L] - 1.
__global__ __launch_bounds__(MO_THREADS) void mo_cluster_accum(const float* __restrict__ vertices, int64_t V, float cell,
                                                               const int32_t* __restrict__ leader, const int32_t* __restrict__ slot_of,
                                                               const int64_t* __restrict__ vcs, int32_t* __restrict__ vertex_map,
                                                               int64_t new_V, unsigned long long* sums, int32_t* cluster_size) {
  const int64_t v = mo_item();
  if (v >= V) return;
  const int32_t s = slot_of[v];
  if (s < 0) { vertex_map[v] = -1; return; }
  const int64_t id = vcs[leader[s]] - 1;
  vertex_map[v] = (int32_t)id;
  if (id < 0 || id >= new_V) return;                                       // prefix sums of other flags than these: nothing is written
  int32_t c[3];
  int64_t u[3];
  mo_cells(vertices + 3 * v, cell, c, u);
  for (int a = 0; a < 3; ++a) atomicAdd(sums + 3 * id + a, (unsigned long long)u[a]);
  atomicAdd(cluster_size + id, 1);
}

__global__ __launch_bounds__(MO_THREADS) void mo_cluster_position(const float* __restrict__ vertices, int64_t V, float cell,
                                                                  const int32_t* __restrict__ vflag, const int64_t* __restrict__ vcs,
                                                                  const unsigned long long* __restrict__ sums,
                                                                  const int32_t* __restrict__ cluster_size, int64_t new_V,
                                                                  float* __restrict__ out) {
  const int64_t v = mo_item();
  if (v >= V || !vflag[v]) return;
  const int64_t id = vcs[v] - 1;
  if (id < 0 || id >= new_V) return;
  int32_t c[3];
  int64_t u[3];
  mo_cells(vertices + 3 * v, cell, c, u);
  for (int a = 0; a < 3; ++a) out[3 * id + a] = mo_position(c[a], (int64_t)sums[3 * id + a], cluster_size[id], cell);
}

// fcs: the inclusive prefix sum of fkeep; new_voff: the first new vertex of every object.
__global__ __launch_bounds__(MO_THREADS) void mo_cluster_faces(const int32_t* __restrict__ faces, int64_t F, const int64_t* __restrict__ voff,
                                                               const int64_t* __restrict__ foff, int N, const int32_t* __restrict__ vertex_map,
                                                               const int64_t* __restrict__ new_voff, const int32_t* __restrict__ fkeep,
                                                               const int64_t* __restrict__ fcs, int64_t new_F, int32_t* __restrict__ out) {
  const int64_t f = mo_item();
  if (f >= F || !fkeep[f]) return;                                         // a kept face has an object and good ids
  const int n = mo_object(foff, N, f);
  const int64_t base = voff[n], at = fcs[f] - 1;
  if (at < 0 || at >= new_F) return;
  for (int c = 0; c < 3; ++c) out[3 * at + c] = (int32_t)(vertex_map[base + faces[3 * f + c]] - new_voff[n]);
}

bool mo_sizes_ok(int64_t F, int N, int64_t V) { return F >= 0 && N >= 0 && V >= 0 && V <= INT32_MAX && F <= INT32_MAX / 3; }

}  // namespace

extern "C" int crn_mesh_tiles(int32_t* out7) {
  if (!out7) return CRN_EINVAL;
  out7[0] = CRN_MESH_THREADS; out7[1] = CRN_MESH_SORT_LANE; out7[2] = CRN_MESH_SORT_TILE; out7[3] = CRN_MESH_CELL_MIN;
  out7[4] = CRN_MESH_CELL_MAX; out7[5] = CRN_MESH_MAX_OBJECTS; out7[6] = CRN_MESH_CLUSTER_MAX_VERTICES;
  return CRN_OK;
}

extern "C" int crn_mesh_corner_count(const int32_t* faces, int64_t F, const int64_t* voff, const int64_t* foff, int N, int64_t V,
                                     int32_t* deg, int64_t* bad, crnStream stream) {
  if (!mo_sizes_ok(F, N, V) || !voff || !foff || !bad || (V && !deg) || (F && !faces)) return CRN_EINVAL;
  CRN_ENTRY(stream);
  hipStream_t st = (hipStream_t)stream;
  CRN_HIP(hipMemsetAsync(bad, 0, 8, st));
  if (V) CRN_HIP(hipMemsetAsync(deg, 0, (size_t)V * 4, st));
  if (!F) return CRN_OK;
  return crn_launch(mo_count, mo_grid(F), dim3(MO_THREADS), 0, st, faces, F, voff, foff, N, V, deg, bad);
}

extern "C" int crn_mesh_corner_lists(const int32_t* faces, int64_t F, const int64_t* voff, const int64_t* foff, int N, int64_t V,
                                     const int64_t* vf_offsets, int32_t* cursor, int32_t* vf_tmp, int32_t* vf_corners, int32_t* cand_tmp,
                                     int32_t* cand, int32_t* vvdeg, uint8_t* irregular, crnStream stream) {
  if (!mo_sizes_ok(F, N, V) || !voff || !foff || !vf_offsets) return CRN_EINVAL;
  if (V && (!cursor || !vvdeg || !irregular)) return CRN_EINVAL;
  if (F && (!faces || !vf_tmp || !vf_corners || !cand_tmp || !cand)) return CRN_EINVAL;
  if (!V) return CRN_OK;
  CRN_ENTRY(stream);
  hipStream_t st = (hipStream_t)stream;
  const dim3 blk(MO_THREADS);
  int rc;
  if (F) {
    CRN_HIP(hipMemsetAsync(cursor, 0, (size_t)V * 4, st));
    rc = crn_launch(mo_fill, mo_grid(F), blk, 0, st, faces, F, voff, foff, N, V, vf_offsets, cursor, (uint32_t*)vf_tmp);
    if (rc != CRN_OK) return rc;
    rc = crn_launch(mo_sort, mo_grid(V), blk, 0, st, vf_offsets, 1, V, (const uint32_t*)vf_tmp, (uint32_t*)vf_corners);
    if (rc != CRN_OK) return rc;
    rc = crn_launch(mo_candidates, mo_grid(3 * F), blk, 0, st, faces, voff, foff, N, F, V, vf_offsets, (const uint32_t*)vf_corners,
                    (uint32_t*)cand_tmp);
    if (rc != CRN_OK) return rc;
    rc = crn_launch(mo_sort, mo_grid(V), blk, 0, st, vf_offsets, 2, V, (const uint32_t*)cand_tmp, (uint32_t*)cand);
    if (rc != CRN_OK) return rc;
  }
  return crn_launch(mo_vv_count, mo_grid(V), blk, 0, st, (const uint32_t*)cand, vf_offsets, V, vvdeg, irregular);
}

extern "C" int crn_mesh_neighbours(const int32_t* cand, const int64_t* vf_offsets, const int64_t* vv_offsets, int64_t V,
                                   int32_t* vv_neighbours, crnStream stream) {
  if (V < 0 || V > INT32_MAX || !vf_offsets || !vv_offsets) return CRN_EINVAL;
  if (!V) return CRN_OK;
  CRN_ENTRY(stream);
  return crn_launch(mo_vv_fill, mo_grid(V), dim3(MO_THREADS), 0, (hipStream_t)stream, (const uint32_t*)cand, vf_offsets, vv_offsets, V,
                    vv_neighbours);
}

extern "C" int crn_mesh_smooth_step(const float* vin, float* vout, const int64_t* vv_offsets, const int32_t* vv_neighbours,
                                    const uint8_t* fixed, float factor, int64_t V, crnStream stream) {
  if (V < 0 || V > INT32_MAX || (V && (!vin || !vout || !vv_offsets || vin == vout))) return CRN_EINVAL;
  if (!V) return CRN_OK;
  CRN_ENTRY(stream);
  return crn_launch(mo_smooth_step, mo_grid(V), dim3(MO_THREADS), 0, (hipStream_t)stream, vin, vout, vv_offsets, vv_neighbours, fixed,
                    factor, V);
}

extern "C" int crn_mesh_face_normals(const float* vertices, const int32_t* faces, int64_t F, const int64_t* voff, const int64_t* foff,
                                     int N, int64_t V, float* out, crnStream stream) {
  if (!mo_sizes_ok(F, N, V) || !voff || !foff || (F && (!faces || !out)) || (F && V && !vertices)) return CRN_EINVAL;
  if (!F) return CRN_OK;
  CRN_ENTRY(stream);
  return crn_launch(mo_face_normals, mo_grid(F), dim3(MO_THREADS), 0, (hipStream_t)stream, vertices, faces, F, voff, foff, N, V, out);
}

extern "C" int crn_mesh_vertex_normals(const float* vertices, const int32_t* faces, int64_t F, const int64_t* voff, int N, int64_t V,
                                       const int64_t* vf_offsets, const int32_t* vf_corners, float* out, crnStream stream) {
  if (!mo_sizes_ok(F, N, V) || !voff || (V && (!vertices || !vf_offsets || !out)) || (F && !faces)) return CRN_EINVAL;
  if (!V) return CRN_OK;
  CRN_ENTRY(stream);
  return crn_launch(mo_vertex_normals, mo_grid(V), dim3(MO_THREADS), 0, (hipStream_t)stream, vertices, faces, F, voff, N, V, vf_offsets,
                    (const uint32_t*)vf_corners, out);
}

extern "C" int crn_mesh_cluster_build(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const int64_t* voff,
                                      const int64_t* foff, int N, float cell, int64_t* table_keys, int32_t* table_leader, int table_log2,
                                      int32_t* slot_of, int32_t* vflag, int32_t* fkeep, int64_t* bad, crnStream stream) {
  if (!mo_sizes_ok(F, N, V) || V > CRN_MESH_CLUSTER_MAX_VERTICES || N > CRN_MESH_MAX_OBJECTS || !(cell > 0.f) || !voff || !foff || !bad)
    return CRN_EINVAL;
  if (table_log2 < mo_table_log2(V) || table_log2 > 31) return CRN_EINVAL;
  if (V && (!vertices || !table_keys || !table_leader || !slot_of || !vflag)) return CRN_EINVAL;
  if (F && (!faces || !fkeep)) return CRN_EINVAL;
  CRN_ENTRY(stream);
  hipStream_t st = (hipStream_t)stream;
  const dim3 blk(MO_THREADS);
  CRN_HIP(hipMemsetAsync(bad, 0, 8, st));
  int rc;
  if (V) {
    const size_t slots = (size_t)1 << table_log2;
    CRN_HIP(hipMemsetAsync(table_keys, 0xFF, slots * 8, st));              // MO_EMPTY_KEY
    CRN_HIP(hipMemsetAsync(table_leader, 0x7F, slots * 4, st));            // above every vertex id
    rc = crn_launch(mo_cluster_keys, mo_grid(V), blk, 0, st, vertices, V, voff, N, cell, (unsigned long long*)table_keys, table_leader,
                    table_log2, slot_of, bad);
    if (rc != CRN_OK) return rc;
    rc = crn_launch(mo_cluster_vflag, mo_grid(V), blk, 0, st, (const int32_t*)table_leader, (const int32_t*)slot_of, V, vflag);
    if (rc != CRN_OK) return rc;
  }
  if (!F) return CRN_OK;
  return crn_launch(mo_cluster_fflag, mo_grid(F), blk, 0, st, faces, F, voff, foff, N, V, (const int32_t*)table_leader,
                    (const int32_t*)slot_of, fkeep, bad);
}

extern "C" int crn_mesh_cluster_emit(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const int64_t* voff,
                                     const int64_t* foff, int N, float cell, const int32_t* table_leader, const int32_t* slot_of,
                                     const int32_t* vflag, const int64_t* vcs, const int32_t* fkeep, const int64_t* fcs,
                                     const int64_t* new_voff, int64_t new_V, int64_t new_F, int32_t* vertex_map, int64_t* sums, int32_t* cluster_size,
                                     float* new_vertices, int32_t* new_faces, crnStream stream) {
  if (!mo_sizes_ok(F, N, V) || new_V < 0 || new_V > V || new_F < 0 || new_F > F || !(cell > 0.f) || !voff || !foff) return CRN_EINVAL;
  if (V && (!vertices || !table_leader || !slot_of || !vflag || !vcs || !vertex_map)) return CRN_EINVAL;
  if (new_V && (!sums || !cluster_size || !new_vertices)) return CRN_EINVAL;
  if (F && (!faces || !fkeep || !fcs || !new_voff || (new_F && !new_faces))) return CRN_EINVAL;
  CRN_ENTRY(stream);
  hipStream_t st = (hipStream_t)stream;
  const dim3 blk(MO_THREADS);
  int rc;
  if (V) {
    if (new_V) {
      CRN_HIP(hipMemsetAsync(sums, 0, (size_t)new_V * 24, st));
      CRN_HIP(hipMemsetAsync(cluster_size, 0, (size_t)new_V * 4, st));
    }
    rc = crn_launch(mo_cluster_accum, mo_grid(V), blk, 0, st, vertices, V, cell, table_leader, slot_of, vcs, vertex_map, new_V,
                    (unsigned long long*)sums, cluster_size);
    if (rc != CRN_OK) return rc;
    rc = crn_launch(mo_cluster_position, mo_grid(V), blk, 0, st, vertices, V, cell, vflag, vcs, (const unsigned long long*)sums,
                    (const int32_t*)cluster_size, new_V, new_vertices);
    if (rc != CRN_OK) return rc;
  }
  if (!F || !new_F) return CRN_OK;
  return crn_launch(mo_cluster_faces, mo_grid(F), blk, 0, st, faces, F, voff, foff, N, (const int32_t*)vertex_map, new_voff, fkeep, fcs,
                    new_F, new_faces);
}
