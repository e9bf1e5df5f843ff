// Configuration histogram of voxel grids on the host: the twin of voxel_topology.hip, part of the product library.  Same
// contract (include/corenet_hip.h) and the same tables and bad counts: integer adds only.  Plain loops:
// the cell planes (grid n, d in 0 .. D) are handed to the threads in order; a thread turns the four voxel rows of a cell
// row into labels (zero-padded by one voxel on either side), counts into a table of its own and adds it to the grid's
// table when it moves to another grid or runs out of planes.  Bin 0 is derived at the end.
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

#include "../../include/corenet_hip.h"
#include "voxel_topology_common.h"

namespace {

inline void add64(int64_t* p, int64_t v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }

// out[1 .. W] <- the labels of row (d, h) of the grid, out[0] = out[W + 1] = 0; a row outside the grid is background.
// Bad voxels are added to *bad when the caller owns the row (count != 0).
template <typename T>
void label_row(const T* g, const int64_t* st, int D, int H, int W, int d, int h, int32_t L, int mask, int32_t* out, bool count,
               int64_t* bad) {
  out[0] = out[W + 1] = 0;
  if (d < 0 || d >= D || h < 0 || h >= H) {
    for (int w = 1; w <= W; ++w) out[w] = 0;
    return;
  }
  const T* p = g + d * st[1] + h * st[2];
  for (int w = 0; w < W; ++w) {
    bool b;
    out[w + 1] = vt_label((int32_t)p[w], L, mask, &b);
    if (b && count) ++*bad;
  }
}

template <typename T>
void count_plane(const T* g, const int64_t* st, int D, int H, int W, int d, int32_t L, int mask, std::vector<int32_t>& buf,
                 int64_t* local, int64_t* bad) {
  const int P = W + 2;
  buf.resize((size_t)4 * P);
  int32_t* r[2][2] = {{buf.data(), buf.data() + P}, {buf.data() + 2 * P, buf.data() + 3 * P}};   // [i][j]
  for (int h = 0; h <= H; ++h) {
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < 2; ++j)
        label_row(g, st, D, H, W, d - 1 + i, h - 1 + j, L, mask, r[i][j], i == 1 && j == 1, bad);   // every voxel is (1, 1) of one cell row
    for (int w = 0; w <= W; ++w) {
      int32_t v[8];
      int32_t any = 0;
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j)
          for (int k = 0; k < 2; ++k) any |= v[vt_row_shift(i, j) + k] = r[i][j][w + k];
      if (!any) continue;
      uint32_t code = 0;
      for (int b = 0; b < 8; ++b) code |= (uint32_t)(v[b] != 0) << b;
      ++local[code];
      if (L == 0) continue;                                  // mask grids and L == 0: row 0 is all there is
      for (int b = 0; b < 8; ++b) {                          // every distinct label once: at its first voxel
        if (!v[b]) continue;
        bool seen = false;
        for (int c = 0; c < b; ++c) seen |= v[c] == v[b];
        if (seen) continue;
        uint32_t lc = 0;
        for (int c = b; c < 8; ++c) lc |= (uint32_t)(v[c] == v[b]) << c;
        ++local[(int64_t)v[b] * 256 + lc];
      }
    }
  }
}

}  // namespace

extern "C" int crn_voxel_topology_cpu(const void* grid, const int64_t* strides, int dtype, int N, int D, int H, int W,
                                      int num_labels, int mask, int64_t* table, int64_t* bad, int num_threads) {
  if (!vt_args_ok(grid, strides, dtype, N, D, H, W, num_labels, mask, table, bad)) return CRN_EINVAL;
  if (N == 0) return CRN_OK;
  const int64_t entries = ((int64_t)num_labels + 1) * 256;
  for (int64_t i = 0; i < entries * N; ++i) table[i] = 0;
  for (int n = 0; n < N; ++n) bad[n] = 0;
  const int64_t planes = (int64_t)D + 1, tasks = planes * N;
  int64_t nt = num_threads > 0 ? num_threads : (int64_t)std::thread::hardware_concurrency();
  if (nt < 1) nt = 1;
  if (nt > tasks) nt = tasks;
  std::atomic<int64_t> next(0);
  auto work = [&]() {
    int cur = -1;
    int64_t nbad = 0;
    std::vector<int64_t> local((size_t)entries, 0);
    std::vector<int32_t> buf;
    auto flush = [&]() {
      if (cur < 0) return;
      int64_t* dst = table + cur * entries;
      for (int64_t i = 0; i < entries; ++i)
        if (local[i]) { add64(dst + i, local[i]); local[i] = 0; }
      if (nbad) add64(bad + cur, nbad);
      nbad = 0;
    };
    for (int64_t i = next.fetch_add(1); i < tasks; i = next.fetch_add(1)) {
      const int n = (int)(i / planes), d = (int)(i - n * planes);
      if (n != cur) { flush(); cur = n; }
      if (dtype == VT_U8) count_plane((const uint8_t*)grid + n * strides[0], strides, D, H, W, d, num_labels, mask, buf, local.data(), &nbad);
      else count_plane((const int32_t*)grid + n * strides[0], strides, D, H, W, d, num_labels, mask, buf, local.data(), &nbad);
    }
    flush();
  };
  std::vector<std::thread> th;
  for (int64_t i = 1; i < nt; ++i) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
  const int64_t cells = vt_cells(D, H, W);
  for (int64_t r = 0; r < (int64_t)N * (num_labels + 1); ++r) {
    int64_t s = 0;
    for (int c = 1; c < 256; ++c) s += table[r * 256 + c];
    table[r * 256] = cells - s;
  }
  return CRN_OK;
}
