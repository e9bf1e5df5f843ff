// Exact squared Euclidean distance transform on the host: the twin of voxel_distance.hip, part of the product library.
// Same contract (include/corenet_hip.h) and the same d2 and index, bit for bit: both follow the
// separable recurrence -- nearest target of the row (ties to the lower w), then argmin_j g[j] + (i - j)^2 along h and
// along d (ties to the lower j).  The line passes walk outwards from i and stop once the squared step alone exceeds the
// best value so far: g >= 0, so nothing beyond can win or tie.  One grid per host thread.
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

#include "../../include/corenet_hip.h"
#include "voxel_distance_common.h"

namespace {

constexpr int32_t NT = CRN_VD_NO_TARGET;

// out[i] = min_j g[j] + (i - j)^2 over a line of L elements; win[i]: the lowest j that attains it (-1: none)
void line_pass(const int32_t* g, int L, int32_t* out, int32_t* win) {
  for (int i = 0; i < L; ++i) {
    int64_t best = NT;
    int bj = -1;
    for (int k = 0; k < L; ++k) {
      if ((int64_t)k * k > best) break;
      const int lo = i - k, hi = i + k;
      if (lo < 0 && hi >= L) break;
      if (hi < L && k > 0 && g[hi] != NT) {
        const int64_t c = (int64_t)g[hi] + (int64_t)k * k;
        if (c < best) { best = c; bj = hi; }
      }
      if (lo >= 0 && g[lo] != NT) {                          // lo is below every j seen so far: it takes a tie
        const int64_t c = (int64_t)g[lo] + (int64_t)k * k;
        if (c <= best) { best = c; bj = lo; }
      }
    }
    out[i] = bj < 0 ? NT : (int32_t)best;
    win[i] = bj;
  }
}

template <typename T>
void distance_grid(const T* g, const int64_t* st, int D, int H, int W, int mode, int32_t* d2, int32_t* index) {
  const int64_t HW = (int64_t)H * W;
  std::vector<int32_t> own;
  if (!index) {
    own.resize((size_t)(D * HW));
    index = own.data();
  }
  // row pass: index holds the winning w (-1: a row without target)
  for (int d = 0; d < D; ++d)
    for (int h = 0; h < H; ++h) {
      int32_t* r2 = d2 + d * HW + (int64_t)h * W;
      int32_t* ri = index + d * HW + (int64_t)h * W;
      int last = -1;
      for (int w = 0; w < W; ++w) {
        if (vd_target(g, st[1], st[2], D, H, W, d, h, w, mode)) last = w;
        ri[w] = last;
      }
      int next = -1;
      for (int w = W - 1; w >= 0; --w) {
        const int lo = ri[w];
        if (lo == w) next = w;
        int win = lo;
        if (next >= 0 && (lo < 0 || next - w < w - lo)) win = next;        // a tie goes to the lower w
        ri[w] = win;
        r2[w] = win < 0 ? NT : (int32_t)((int64_t)(win - w) * (win - w));
      }
    }
  const int L = H > D ? H : D;
  std::vector<int32_t> gin((size_t)L), iin((size_t)L), gout((size_t)L), win((size_t)L);
  // h pass: the winner keeps row j's w
  if (H > 1)
    for (int d = 0; d < D; ++d)
      for (int w = 0; w < W; ++w) {
        int32_t* c2 = d2 + d * HW + w;
        int32_t* ci = index + d * HW + w;
        for (int h = 0; h < H; ++h) { gin[h] = c2[(int64_t)h * W]; iin[h] = ci[(int64_t)h * W]; }
        line_pass(gin.data(), H, gout.data(), win.data());
        for (int h = 0; h < H; ++h) {
          c2[(int64_t)h * W] = gout[h];
          ci[(int64_t)h * W] = win[h] < 0 ? -1 : win[h] * W + iin[win[h]];
        }
      }
  // d pass (with H == 1 the row's w already is the plane index)
  if (D > 1)
    for (int64_t c = 0; c < HW; ++c) {
      for (int d = 0; d < D; ++d) { gin[d] = d2[d * HW + c]; iin[d] = index[d * HW + c]; }
      line_pass(gin.data(), D, gout.data(), win.data());
      for (int d = 0; d < D; ++d) {
        d2[d * HW + c] = gout[d];
        index[d * HW + c] = win[d] < 0 ? -1 : (int32_t)(win[d] * HW + iin[win[d]]);
      }
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

extern "C" int crn_voxel_distance_cpu(const void* grid, const int64_t* strides, int dtype, int N, int D, int H, int W, int mode,
                                      int32_t* d2, int32_t* index, int num_threads) {
  if (!vd_args_ok(grid, strides, dtype, N, D, H, W, mode, d2)) return CRN_EINVAL;
  if (N == 0) return CRN_OK;
  const int64_t S = (int64_t)D * H * W;
  run_tasks(N, num_threads, [&](int64_t n) {
    int32_t* idx = index ? index + n * S : nullptr;
    if (dtype == VD_U8)
      distance_grid((const uint8_t*)grid + n * strides[0], strides, D, H, W, mode, d2 + n * S, idx);
    else
      distance_grid((const int32_t*)grid + n * strides[0], strides, D, H, W, mode, d2 + n * S, idx);
  });
  return CRN_OK;
}
