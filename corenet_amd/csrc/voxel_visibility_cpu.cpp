// Voxel visibility from an eye on the host: the twin of voxel_visibility.hip, part of the product library.  Same
// contract (include/corenet_hip.h) and the same occluded and first, bit for bit: both run the integer
// walk of voxel_visibility_common.h over one occupancy bit per voxel.  Two phases, each spread over the planes (n, z) of
// all grids: pack the bits, then walk every voxel of the plane.
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

#include "../../include/corenet_hip.h"
#include "voxel_visibility_common.h"

namespace {

template <typename T>
void pack_plane(const T* g, const int64_t* st, int H, int W, int z, uint64_t* bits) {
  const int words = vv_words64(W);
  for (int y = 0; y < H; ++y) {
    const T* row = g + z * st[1] + y * st[2];
    uint64_t* out = bits + ((int64_t)z * H + y) * words;
    for (int w = 0; w < words; ++w) out[w] = 0;
    for (int x = 0; x < W; ++x)
      if (vv_occupied(row[x])) out[x >> 6] |= 1ull << (x & 63);
  }
}

void walk_plane(const uint64_t* bits, int D, int H, int W, int z, const int32_t* eye, bool count, uint8_t* occluded, int32_t* first) {
  const int words = vv_words64(W);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      VvWalk k = vv_start(x, y, z, eye);
      int32_t last = -1, steps = 0;
      while (vv_step(k, D, H, W)) {
        ++steps;
        if (vv_bit(bits, words, H, k.pos[0], k.pos[1], k.pos[2])) {
          last = (int32_t)(((int64_t)k.pos[2] * H + k.pos[1]) * W + k.pos[0]);
          if (!first) break;                                 // the mask alone: the first hit settles it
        }
      }
      const int64_t v = ((int64_t)z * H + y) * W + x;
      occluded[v] = last >= 0;
      if (first) first[v] = count ? steps : last;
    }
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

extern "C" int crn_voxel_visibility_cpu(const void* grid, const int64_t* strides, int dtype, int N, int D, int H, int W,
                                        const int32_t* eye_q, int flags, uint8_t* occluded, int32_t* first, int num_threads) {
  if (!vv_args_ok(grid, strides, dtype, N, D, H, W, eye_q, flags, CRN_VV_FLAT | CRN_VV_COUNT_STEPS, occluded)) return CRN_EINVAL;
  const bool count = (flags & CRN_VV_COUNT_STEPS) != 0;
  if (count && !first) return CRN_EINVAL;
  if (N == 0) return CRN_OK;
  const int64_t S = (int64_t)D * H * W, per_grid = (int64_t)D * H * vv_words64(W);
  std::vector<uint64_t> bits((size_t)(N * per_grid));
  run_tasks((int64_t)N * D, num_threads, [&](int64_t i) {
    const int64_t n = i / D;
    const int z = (int)(i - n * D);
    if (dtype == VV_U8)
      pack_plane((const uint8_t*)grid + n * strides[0], strides, H, W, z, bits.data() + n * per_grid);
    else
      pack_plane((const int32_t*)grid + n * strides[0], strides, H, W, z, bits.data() + n * per_grid);
  });
  run_tasks((int64_t)N * D, num_threads, [&](int64_t i) {
    const int64_t n = i / D;
    const int z = (int)(i - n * D);
    walk_plane(bits.data() + n * per_grid, D, H, W, z, eye_q + n * 3, count, occluded + n * S, first ? first + n * S : nullptr);
  });
  return CRN_OK;
}
