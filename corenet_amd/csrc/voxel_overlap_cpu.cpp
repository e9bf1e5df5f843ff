// Label overlaps of two voxel grids on the host: the twin of voxel_overlap.hip, part of the product library.  Same
// contract (include/corenet_hip.h) and the same tables and bad counts: integer adds only.  Plain loops:
// the chunks of CRN_VO_CHUNK voxels of all grids are handed to the threads in order; a thread counts into a table of its
// own and adds it to the grid's table when it moves to another grid or runs out of chunks.  Tables above VO_LOCAL_MAX
// entries are added to directly, one atomic per voxel run.
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

#include "../../include/corenet_hip.h"
#include "voxel_overlap_common.h"

namespace {

constexpr int64_t VO_LOCAL_MAX = 1 << 20;

inline void add64(int64_t* p, int64_t v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }

struct Local {
  int grid = -1;
  int64_t bad = 0;
  std::vector<int64_t> table;
};

template <typename TA, typename TB>
void count_chunk(const TA* a, const TB* b, const VoRows& rw, int64_t v, int64_t v1, int32_t na, int32_t nb, int64_t* local,
                 int64_t* shared, int64_t& bad) {
  int64_t r = v / rw.L;
  int x = (int)(v - r * rw.L);
  while (v < v1) {
    const int64_t left = v1 - v;
    const int len = left < rw.L - x ? (int)left : rw.L - x;
    const int64_t r1 = r / rw.R2, r2 = r - r1 * rw.R2;
    const TA* pa = a + r1 * rw.a1 + r2 * rw.a2 + x;
    const TB* pb = b + r1 * rw.b1 + r2 * rw.b2 + x;
    if (local) {
      for (int i = 0; i < len; ++i) {
        const uint32_t k = vo_key((int32_t)pa[i], (int32_t)pb[i], na, nb);
        if (k == VO_BAD) ++bad; else ++local[k];
      }
    } else {
      uint32_t key = 0;
      int64_t run = 0;
      for (int i = 0; i < len; ++i) {
        const uint32_t k = vo_key((int32_t)pa[i], (int32_t)pb[i], na, nb);
        if (k == key) { ++run; continue; }
        if (run) { if (key == VO_BAD) bad += run; else add64(shared + key, run); }
        key = k; run = 1;
      }
      if (run) { if (key == VO_BAD) bad += run; else add64(shared + key, run); }
    }
    v += len; ++r; x = 0;
  }
}

}  // namespace

extern "C" int crn_voxel_overlap_cpu(const void* a, const int64_t* strides_a, int dtype_a, const void* b, const int64_t* strides_b,
                                     int dtype_b, int N, int D, int H, int W, const int64_t* num_a, const int64_t* num_b,
                                     const int64_t* table_offsets, int64_t* table, int64_t* bad, int num_threads) {
  if (!vo_args_ok(a, strides_a, dtype_a, b, strides_b, dtype_b, N, D, H, W, num_a, num_b, table_offsets, table, bad)) return CRN_EINVAL;
  if (N == 0) return CRN_OK;
  for (int64_t i = 0; i < table_offsets[N]; ++i) table[i] = 0;
  for (int n = 0; n < N; ++n) bad[n] = 0;
  const VoRows rw = vo_rows(strides_a, strides_b, D, H, W);
  const int64_t S = (int64_t)D * H * W, chunks = (S + CRN_VO_CHUNK - 1) / CRN_VO_CHUNK, tasks = chunks * N;
  int64_t nt = num_threads > 0 ? num_threads : (int64_t)std::thread::hardware_concurrency();
  if (nt < 1) nt = 1;
  if (nt > tasks) nt = tasks;
  std::atomic<int64_t> next(0);
  auto work = [&]() {
    Local loc;
    auto flush = [&]() {
      if (loc.grid < 0) return;
      int64_t* dst = table + table_offsets[loc.grid];
      for (size_t i = 0; i < loc.table.size(); ++i)
        if (loc.table[i]) add64(dst + i, loc.table[i]);
      if (loc.bad) add64(bad + loc.grid, loc.bad);
      loc.bad = 0;
    };
    for (int64_t i = next.fetch_add(1); i < tasks; i = next.fetch_add(1)) {
      const int n = (int)(i / chunks);
      const int64_t v = (i - n * chunks) * CRN_VO_CHUNK, v1 = v + CRN_VO_CHUNK < S ? v + CRN_VO_CHUNK : S;
      const int64_t entries = vo_entries_ok(num_a[n], num_b[n], table_offsets[n + 1] - table_offsets[n]);
      if (n != loc.grid) {
        flush();
        loc.grid = n;
        loc.table.assign(entries > 0 && entries <= VO_LOCAL_MAX ? (size_t)entries : 0, 0);
      }
      if (entries < 0) { loc.bad += v1 - v; continue; }     // no table to count into: the chunk is bad
      const int32_t na = (int32_t)num_a[n], nb = (int32_t)num_b[n];
      int64_t* local = loc.table.empty() ? nullptr : loc.table.data();
      int64_t* shared = table + table_offsets[n];
      const char* ga = (const char*)a + n * strides_a[0] * (dtype_a == VO_U8 ? 1 : 4);
      const char* gb = (const char*)b + n * strides_b[0] * (dtype_b == VO_U8 ? 1 : 4);
      if (dtype_a == VO_U8) {
        if (dtype_b == VO_U8) count_chunk((const uint8_t*)ga, (const uint8_t*)gb, rw, v, v1, na, nb, local, shared, loc.bad);
        else count_chunk((const uint8_t*)ga, (const int32_t*)gb, rw, v, v1, na, nb, local, shared, loc.bad);
      } else {
        if (dtype_b == VO_U8) count_chunk((const int32_t*)ga, (const uint8_t*)gb, rw, v, v1, na, nb, local, shared, loc.bad);
        else count_chunk((const int32_t*)ga, (const int32_t*)gb, rw, v, v1, na, nb, local, shared, loc.bad);
      }
    }
    flush();
  };
  std::vector<std::thread> th;
  for (int64_t i = 1; i < nt; ++i) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
  return CRN_OK;
}
