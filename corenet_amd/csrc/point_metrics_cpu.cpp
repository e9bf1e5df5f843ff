// Surface sampling, nearest-neighbour and point-to-triangle distances on the host: the twin of point_metrics.hip, part of the product
// library.  Same contract, same per-element arithmetic (point_metrics_common.h): the GPU and this twin return identical
// arrays.  One object per task (std::thread workers pulling object ids), as in marching_cubes_cpu.cpp.
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

#include "../../include/corenet_hip.h"
#include "point_metrics_common.h"

namespace {

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

bool offsets_ok(const int64_t* off, int N) {
  if (!off || off[0] < 0) return false;
  for (int n = 0; n < N; ++n)
    if (off[n + 1] < off[n]) return false;
  return true;
}

void sample_object(const float* tri, int64_t t0, int64_t t1, int64_t S, uint32_t seed, float* points, int32_t* tri_index,
                   uint8_t* valid) {
  float amax = 0.f;
  for (int64_t k = t0; k < t1; ++k) {
    const float a = pm_area(tri + 9 * k);
    if (pm_area_ok(a) && a > amax) amax = a;
  }
  if (!(amax > 0.f)) {
    *valid = 0;
    for (int64_t i = 0; i < S; ++i) {
      points[3 * i] = points[3 * i + 1] = points[3 * i + 2] = 0.f;
      tri_index[i] = -1;
    }
    return;
  }
  *valid = 1;
  std::vector<int64_t> cum((size_t)(t1 - t0));
  int64_t run = 0;
  for (int64_t k = t0; k < t1; ++k) cum[(size_t)(k - t0)] = run += pm_weight(pm_area(tri + 9 * k), amax);
  for (int64_t i = 0; i < S; ++i) pm_sample(tri, cum.data() - t0, t0, t1, run, i, S, seed, points + 3 * i, tri_index + i);
}

void nearest_object(const float* a, int64_t na, const float* b, int64_t nb, float* dist2, int32_t* index) {
  for (int64_t q = 0; q < na; ++q) {
    const float ax = a[3 * q], ay = a[3 * q + 1], az = a[3 * q + 2];
    float best = INFINITY;
    int32_t bi = -1;
    for (int64_t j = 0; j < nb; ++j) {
      const float d2 = pm_d2(ax, ay, az, b[3 * j], b[3 * j + 1], b[3 * j + 2]);
      if (d2 < best || (bi < 0 && d2 == d2)) { best = d2; bi = (int32_t)j; }     // (d2, index) minimum; NaN never
    }
    dist2[q] = best;
    index[q] = bi;
  }
}

void point_triangle_object(const float* p, int64_t np, const float* tri, int64_t nt, float* dist2, int32_t* index) {
  std::vector<float> rec((size_t)nt * PM_TRI_REC);
  for (int64_t j = 0; j < nt; ++j) pm_tri_record(tri + 9 * j, rec.data() + PM_TRI_REC * j);
  for (int64_t q = 0; q < np; ++q) {
    const float px = p[3 * q], py = p[3 * q + 1], pz = p[3 * q + 2];
    float best = INFINITY;
    int32_t bi = -1;
    for (int64_t j = 0; j < nt; ++j) {
      const float d2 = pm_tri_d2(px, py, pz, rec.data() + PM_TRI_REC * j);
      if (d2 < best) { best = d2; bi = (int32_t)j; }                             // strict, ascending: ties to the lowest index
    }
    dist2[q] = best;
    index[q] = bi;
  }
}

}  // namespace

extern "C" int crn_point_triangle_cpu(const float* p, const int64_t* p_offsets, const float* triangles, const int64_t* t_offsets,
                                      int N, float* dist2, int32_t* index, int num_threads) {
  if (N < 1 || !offsets_ok(p_offsets, N) || !offsets_ok(t_offsets, N)) return CRN_EINVAL;
  if (p_offsets[N] > 0 && (!p || !dist2 || !index)) return CRN_EINVAL;
  if (t_offsets[N] > 0 && !triangles) return CRN_EINVAL;
  for (int n = 0; n < N; ++n)
    if (t_offsets[n + 1] - t_offsets[n] > CRN_PM_MAX_CANDIDATES) return CRN_EINVAL;
  for_objects(N, num_threads, [&](int n) {
    const int64_t p0 = p_offsets[n], t0 = t_offsets[n];
    point_triangle_object(p + 3 * p0, p_offsets[n + 1] - p0, triangles + 9 * t0, t_offsets[n + 1] - t0, dist2 + p0, index + p0);
  });
  return 0;
}

extern "C" int crn_sample_surface_cpu(const float* triangles, const int64_t* tri_offsets, int N, int64_t S, uint32_t seed,
                                      float* points, int32_t* tri_index, uint8_t* valid, int num_threads) {
  if (N < 1 || S < 1 || S > CRN_PM_MAX_SAMPLES || !points || !tri_index || !valid || !offsets_ok(tri_offsets, N)) return CRN_EINVAL;
  if (!triangles && tri_offsets[N] > 0) return CRN_EINVAL;
  for_objects(N, num_threads, [&](int n) {
    sample_object(triangles, tri_offsets[n], tri_offsets[n + 1], S, seed, points + 3 * S * n, tri_index + S * n, valid + n);
  });
  return 0;
}

extern "C" int crn_nearest_cpu(const float* a, const int64_t* a_offsets, const float* b, const int64_t* b_offsets, int N,
                               float* dist2, int32_t* index, int num_threads) {
  if (N < 1 || !offsets_ok(a_offsets, N) || !offsets_ok(b_offsets, N)) return CRN_EINVAL;
  if (a_offsets[N] > 0 && (!a || !dist2 || !index)) return CRN_EINVAL;
  if (b_offsets[N] > 0 && !b) return CRN_EINVAL;
  for (int n = 0; n < N; ++n)
    if (b_offsets[n + 1] - b_offsets[n] > CRN_PM_MAX_CANDIDATES) return CRN_EINVAL;
  for_objects(N, num_threads, [&](int n) {
    const int64_t a0 = a_offsets[n], b0 = b_offsets[n];
    nearest_object(a + 3 * a0, a_offsets[n + 1] - a0, b + 3 * b0, b_offsets[n + 1] - b0, dist2 + a0, index + a0);
  });
  return 0;
}
