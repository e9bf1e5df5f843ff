// Score-level evaluation on the host: the twin of eval_scores.hip, part of the product library.  Same contract
// (include/corenet_hip.h), the same arithmetic (eval_scores_common.h) and the same table, sq and bad: every sum is an
// integer sum.  One (sample, depth slice) per task (std::thread workers pulling task ids, as in eval_labels_cpu.cpp); a
// worker counts into tables of its own and adds them to the outputs when it is done.
#include <math.h>

#include <atomic>
#include <cstdint>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/corenet_hip.h"
#include "eval_scores_common.h"

namespace {

template <int CT>
void slice(const float* scores, int from_logits, const int32_t* gt, const int32_t* scene_class, int b, int z, int C, int K, int H,
           int W, int64_t S, int m, int iz, int iy, int ix, int nbins, int64_t* table, int64_t* sq, int64_t* nbad) {
  const int64_t sc = scene_class ? (int64_t)scene_class[b] : 1;
  if (sc < 1 || (int64_t)(C - 1) * sc >= K) { *nbad += (int64_t)H * W; return; }
  const int isc = (int)sc;
  const int64_t mW = (int64_t)W * m, mH = (int64_t)H * m;
  const int64_t fine_b = (int64_t)b * S * m * m * m;
  const float* sb = scores + (int64_t)b * C * S + (int64_t)z * H * W;
  auto entry = [&](int row, int q, int y) {
    int64_t* e = table + ((int64_t)(row * nbins + es_bin(q, nbins)) * 2 + y) * 2;
    e[0] += 1; e[1] += q;
    sq[row * 2 + y] += es_sq(q, y);
  };
  for (int y = 0; y < H; ++y) {
    const int64_t frow = fine_b + (((int64_t)z * m + iz) * mH + ((int64_t)y * m + iy)) * mW + ix;
    for (int x = 0; x < W; ++x) {
      float p[CT];
      const float* s = sb + (int64_t)y * W + x;
      for (int c = 0; c < C; ++c) { p[c] = *s; s += S; }
      if (from_logits) es_softmax<CT>(p, C);
      const int64_t gg = (int64_t)gt[frow + (int64_t)x * m] * sc;
      bool ok = gg >= 0 && gg < K;
      for (int c = 0; c < C; ++c) ok = ok && es_p_ok(p[c]);
      if (!ok) { ++*nbad; continue; }
      const int gi = (int)gg;
      for (int c = 0; c < C; ++c) entry(c * isc, es_q(p[c]), gi == c * isc);
      entry(K, ES_ONE - es_q(p[0]), gi != 0);
    }
  }
}

template <int CT>
void softmax_rows(const float* in, int C, int64_t S, int64_t v0, int64_t v1, float* out) {
  for (int64_t v = v0; v < v1; ++v) {
    float x[CT];
    for (int c = 0; c < C; ++c) x[c] = in[(int64_t)c * S + v];
    es_softmax<CT>(x, C);
    for (int c = 0; c < C; ++c) out[(int64_t)c * S + v] = x[c];
  }
}

int64_t worker_count(int num_threads, int64_t tasks, int64_t work) {
  int64_t nt = num_threads > 0 ? num_threads : (int64_t)std::thread::hardware_concurrency();
  if (nt < 1) nt = 1;
  if (nt > tasks) nt = tasks;
  if (work < 65536) nt = 1;                                  // not worth a thread
  return nt;
}

}  // namespace

extern "C" int crn_eval_scores_cpu(const float* scores, int from_logits, const int32_t* gt, const int32_t* scene_class, int B,
                                   int C, int K, int D, int H, int W, int m, int n, int nbins, int64_t* table, int64_t* sq,
                                   int64_t* bad, int num_threads) {
  if (!es_args_ok(scores, gt, B, C, K, D, H, W, m, n, nbins, table, sq, bad)) return CRN_EINVAL;
  const int64_t S = (int64_t)D * H * W, tasks = (int64_t)B * D;
  const int ix = n % m, iy = (n / m) % m, iz = (int)(n / ((int64_t)m * m));
  const int64_t nt = worker_count(num_threads, tasks, S * B);
  const size_t E4 = (size_t)(K + 1) * nbins * 4, R2 = (size_t)(K + 1) * 2;
  std::atomic<int64_t> next(0);
  std::mutex merge;
  auto work = [&]() {
    std::vector<int64_t> tab(E4, 0), sqs(R2, 0);
    int64_t nbad = 0;
    for (int64_t t = next.fetch_add(1); t < tasks; t = next.fetch_add(1)) {
      const int b = (int)(t / D), z = (int)(t % D);
#define CRN_ES(CT) slice<CT>(scores, from_logits, gt, scene_class, b, z, C, K, H, W, S, m, iz, iy, ix, nbins, tab.data(), sqs.data(), &nbad)
      if (C <= 2) CRN_ES(2); else if (C <= 4) CRN_ES(4); else if (C <= 8) CRN_ES(8);
      else if (C <= 16) CRN_ES(16); else CRN_ES(32);
#undef CRN_ES
    }
    std::lock_guard<std::mutex> lock(merge);
    for (size_t i = 0; i < E4; ++i) table[i] += tab[i];
    for (size_t i = 0; i < R2; ++i) sq[i] += sqs[i];
    bad[0] += nbad;
  };
  std::vector<std::thread> th;
  for (int64_t i = 1; i < nt; ++i) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
  return CRN_OK;
}

extern "C" int crn_score_softmax_cpu(const float* logits, int B, int C, int64_t S, float* out, int num_threads) {
  if (!es_softmax_args_ok(logits, B, C, S, out)) return CRN_EINVAL;
  constexpr int64_t ROWS = 4096;
  const int64_t per = (S + ROWS - 1) / ROWS, tasks = (int64_t)B * per;
  const int64_t nt = worker_count(num_threads, tasks, S * B);
  std::atomic<int64_t> next(0);
  auto work = [&]() {
    for (int64_t t = next.fetch_add(1); t < tasks; t = next.fetch_add(1)) {
      const int64_t b = t / per, v0 = (t % per) * ROWS, v1 = v0 + ROWS < S ? v0 + ROWS : S;
      const float* in = logits + b * C * S;
      float* o = out + b * C * S;
#define CRN_ES(CT) softmax_rows<CT>(in, C, S, v0, v1, o)
      if (C <= 2) CRN_ES(2); else if (C <= 4) CRN_ES(4); else if (C <= 8) CRN_ES(8);
      else if (C <= 16) CRN_ES(16); else CRN_ES(32);
#undef CRN_ES
    }
  };
  std::vector<std::thread> th;
  for (int64_t i = 1; i < nt; ++i) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
  return CRN_OK;
}
