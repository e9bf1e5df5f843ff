// Streaming evaluation labels on the host: the twin of eval_labels.hip, part of the product library.  Same contract
// (include/corenet_hip.h, eval_labels_common.h) and the same labels, cm and bad: every sum is an integer sum.  One
// (sample, depth slice) per task (std::thread workers pulling task ids, as in point_metrics_cpu.cpp); a worker counts
// into a matrix of its own and adds it to cm when it is done.
#include <atomic>
#include <cstdint>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/corenet_hip.h"
#include "eval_labels_common.h"

namespace {

template <int CT>
void slice(const float* scores, const int32_t* gt, const int32_t* scene_class, int b, int z, int C, int K, int H, int W, int64_t S,
           int m, int iz, int iy, int ix, int32_t* labels, int64_t* hist, int64_t* nbad) {
  const int64_t sc = scene_class ? (int64_t)scene_class[b] : 1;
  const int64_t mW = (int64_t)W * m, mH = (int64_t)H * m;
  const int64_t fine_b = (int64_t)b * S * m * m * m;
  const float* sb = scores + (int64_t)b * C * S + (int64_t)z * H * W;
  for (int y = 0; y < H; ++y) {
    const int64_t frow = fine_b + (((int64_t)z * m + iz) * mH + ((int64_t)y * m + iy)) * mW + ix;
    for (int x = 0; x < W; ++x) {
      const int64_t f = frow + (int64_t)x * m;
      const int64_t pred = (int64_t)el_argmax<CT>(sb + (int64_t)y * W + x, C, S) * sc;
      if (labels) labels[f] = (int32_t)pred;
      if (gt) {
        const int bin = el_bin((int64_t)gt[f] * sc, pred, K);
        if (bin >= 0) ++hist[bin]; else ++*nbad;
      }
    }
  }
}

}  // namespace

extern "C" int crn_eval_labels_cpu(const float* scores, const int32_t* gt, const int32_t* scene_class, int B, int C, int K, int D,
                                   int H, int W, int m, int n, int32_t* labels, int64_t* cm, int32_t* bad, int num_threads) {
  if (!el_args_ok(scores, gt, B, C, K, D, H, W, m, n, labels, cm, bad)) return CRN_EINVAL;
  const int64_t S = (int64_t)D * H * W, tasks = (int64_t)B * D;
  const int ix = n % m, iy = (n / m) % m, iz = (int)(n / ((int64_t)m * m));
  int64_t nt = num_threads > 0 ? num_threads : (int64_t)std::thread::hardware_concurrency();
  if (nt < 1) nt = 1;
  if (nt > tasks) nt = tasks;
  if (S * B < 65536) nt = 1;                                 // not worth a thread
  std::atomic<int64_t> next(0);
  std::mutex merge;
  auto work = [&]() {
    std::vector<int64_t> hist(gt ? (size_t)K * K : 0, 0);
    int64_t nbad = 0;
    for (int64_t t = next.fetch_add(1); t < tasks; t = next.fetch_add(1)) {
      const int b = (int)(t / D), z = (int)(t % D);
#define CRN_EL(CT) slice<CT>(scores, gt, scene_class, b, z, C, K, H, W, S, m, iz, iy, ix, labels, hist.data(), &nbad)
      if (C <= 2) CRN_EL(2); else if (C <= 4) CRN_EL(4); else if (C <= 8) CRN_EL(8);
      else if (C <= 16) CRN_EL(16); else CRN_EL(32);
#undef CRN_EL
    }
    if (gt) {
      std::lock_guard<std::mutex> lock(merge);
      for (size_t i = 0; i < hist.size(); ++i) cm[i] += hist[i];
      bad[0] = (int32_t)(bad[0] + nbad);
    }
  };
  std::vector<std::thread> th;
  for (int64_t i = 1; i < nt; ++i) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
  return CRN_OK;
}
