// Voxel connected components on the host: the twin of voxel_components.hip, part of the product library.  Same contract
// (include/corenet_hip.h) and the same labels, counts and stats: they are a function of the partition
// alone.  A plain two-pass union-find over the whole grid with no notion of bricks: pass 1 unites every foreground voxel
// with its equal-keyed backward neighbours (the 3 / 9 / 13 offsets that precede it in raster order), hooking the larger
// root under the smaller, so a root is the lowest index of its set; pass 2 numbers the roots in raster order.  One grid
// per host thread (std::thread workers pulling grid ids, as in eval_labels_cpu.cpp).
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

#include "../../include/corenet_hip.h"
#include "voxel_components_common.h"

namespace {

inline int32_t find(int32_t* p, int32_t x) {
  while (p[x] != x) {
    p[x] = p[p[x]];                                          // path halving
    x = p[x];
  }
  return x;
}

inline void unite(int32_t* p, int32_t a, int32_t b) {
  a = find(p, a);
  b = find(p, b);
  if (a < b) p[b] = a; else if (b < a) p[a] = b;
}

template <typename T>
void label_grid(const T* g, const int64_t* st, int D, int H, int W, int level, int by_value, int32_t* labels, int64_t* num) {
  const int64_t S = (int64_t)D * H * W;
  std::vector<int32_t> parent((size_t)S);
  int32_t* p = parent.data();
  // labels holds the keys during pass 1
  for (int d = 0; d < D; ++d)
    for (int h = 0; h < H; ++h) {
      const T* row = g + d * st[1] + h * st[2];
      int32_t* krow = labels + ((int64_t)d * H + h) * W;
      for (int w = 0; w < W; ++w) krow[w] = vc_key(row[w], by_value);
    }
  for (int d = 0; d < D; ++d)
    for (int h = 0; h < H; ++h)
      for (int w = 0; w < W; ++w) {
        const int32_t v = (int32_t)(((int64_t)d * H + h) * W + w);
        p[v] = v;
        const int32_t k = labels[v];
        if (!k) continue;
        for (int dd = -1; dd <= 0; ++dd)
          for (int dh = -1; dh <= 1; ++dh)
            for (int dw = -1; dw <= 1; ++dw) {
              if (dd == 0 && (dh > 0 || (dh == 0 && dw >= 0))) continue;          // not before v in raster order
              if ((dd != 0) + (dh != 0) + (dw != 0) > level) continue;
              const int e = d + dd, i = h + dh, j = w + dw;
              if (e < 0 || i < 0 || i >= H || j < 0 || j >= W) continue;
              const int32_t u = (int32_t)(((int64_t)e * H + i) * W + j);
              if (labels[u] == k) unite(p, v, u);
            }
      }
  int32_t next = 0;
  for (int64_t v = 0; v < S; ++v) {
    if (!labels[v]) continue;                                // background keeps its 0
    const int32_t r = find(p, (int32_t)v);
    labels[v] = r == v ? ++next : labels[r];                 // a root comes before every other voxel of its set
  }
  *num = next;
}

template <typename F>
void run_tasks(int64_t tasks, int num_threads, F&& task) {
  int64_t nt = num_threads > 0 ? num_threads : (int64_t)std::thread::hardware_concurrency();
  if (nt < 1) nt = 1;
  if (nt > tasks) nt = tasks;
  std::atomic<int64_t> next(0);
  auto work = [&]() {
    for (int64_t i = next.fetch_add(1); i < tasks; i = next.fetch_add(1)) task(i);
  };
  std::vector<std::thread> th;
  for (int64_t i = 1; i < nt; ++i) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
}

}  // namespace

extern "C" int crn_voxel_components_cpu(const void* grid, const int64_t* strides, int dtype, int N, int D, int H, int W,
                                        int connectivity, int by_value, int32_t* labels, int64_t* num_components, int num_threads) {
  if (!vc_args_ok(grid, strides, dtype, N, D, H, W, connectivity, labels, num_components)) return CRN_EINVAL;
  const int level = vc_level(connectivity);
  const int64_t S = (int64_t)D * H * W;
  run_tasks(N, num_threads, [&](int64_t n) {
    if (dtype == VC_U8)
      label_grid((const uint8_t*)grid + n * strides[0], strides, D, H, W, level, by_value, labels + n * S, num_components + n);
    else
      label_grid((const int32_t*)grid + n * strides[0], strides, D, H, W, level, by_value, labels + n * S, num_components + n);
  });
  return CRN_OK;
}

extern "C" int crn_component_stats_cpu(const int32_t* labels, const void* grid, const int64_t* strides, int dtype, int N, int D,
                                       int H, int W, const int64_t* offsets, int64_t K, int64_t* size, int32_t* bbox,
                                       int64_t* first, int32_t* value, int num_threads) {
  if (!vc_stats_args_ok(labels, grid, strides, dtype, N, D, H, W, offsets, K, size, bbox, first, value)) return CRN_EINVAL;
  const int64_t S = (int64_t)D * H * W;
  run_tasks(N, num_threads, [&](int64_t n) {
    const int64_t c0 = offsets[n], c1 = offsets[n + 1];
    for (int64_t c = c0; c < c1; ++c) {
      size[c] = 0;
      first[c] = INT64_MAX;
      int32_t* b = bbox + 6 * c;
      b[0] = b[1] = b[2] = INT32_MAX;
      b[3] = b[4] = b[5] = 0;
    }
    const int32_t* lab = labels + n * S;
    for (int d = 0; d < D; ++d)
      for (int h = 0; h < H; ++h)
        for (int w = 0; w < W; ++w) {
          const int64_t v = ((int64_t)d * H + h) * W + w;
          const int32_t l = lab[v];
          if (l <= 0 || l > c1 - c0) continue;
          const int64_t c = c0 + l - 1;
          int32_t* b = bbox + 6 * c;
          ++size[c];
          if (v < first[c]) first[c] = v;
          if (d < b[0]) b[0] = d;
          if (h < b[1]) b[1] = h;
          if (w < b[2]) b[2] = w;
          if (d + 1 > b[3]) b[3] = d + 1;
          if (h + 1 > b[4]) b[4] = h + 1;
          if (w + 1 > b[5]) b[5] = w + 1;
        }
    if (grid)
      for (int64_t c = c0; c < c1; ++c) {
        if (first[c] == INT64_MAX) { value[c] = 0; continue; }
        const int64_t v = first[c];
        const int w = (int)(v % W), h = (int)((v / W) % H), d = (int)(v / ((int64_t)W * H));
        const int64_t off = n * strides[0] + d * strides[1] + h * strides[2] + w;
        value[c] = dtype == VC_U8 ? (int32_t)((const uint8_t*)grid)[off] : ((const int32_t*)grid)[off];
      }
  });
  return CRN_OK;
}
