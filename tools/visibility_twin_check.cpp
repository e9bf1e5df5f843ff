// A stand-alone run of the host twin of corenet_amd.voxel_visibility for the sanitizers: signed overflow in the 64-bit
// terms of the walk, and the bounds of the packed occupancy bits.  Not part of the library build, not run by pytest:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       tools/visibility_twin_check.cpp corenet_amd/csrc/voxel_visibility_cpu.cpp -o tools/_build/visibility_twin_check
//   tools/_build/visibility_twin_check
//
// Two cases: a (3, 5, 70) grid with the eye at every corner of the +-2^19 range (|delta| reaches 2^20, the terms 2^60),
// and a random 32^3 grid with eyes outside, inside and on the centre lattice.  It also checks that `first` points at
// an occupied voxel exactly where `occluded` is set, and that the mask without `first` is the same.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/corenet_hip.h"

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

static int run(int D, int H, int W, double density, const int32_t* eye, const char* what) {
  const size_t S = (size_t)D * H * W;
  std::vector<uint8_t> grid(S), occ(S), occ_only(S);
  std::vector<int32_t> first(S), steps(S);
  for (auto& g : grid) g = (rnd() & 0xffff) < density * 65536.0;
  const int64_t st[4] = {(int64_t)S, (int64_t)H * W, W, 1};
  int rc = crn_voxel_visibility_cpu(grid.data(), st, 1, 1, D, H, W, eye, 0, occ.data(), first.data(), 2);
  if (rc == CRN_OK) rc = crn_voxel_visibility_cpu(grid.data(), st, 1, 1, D, H, W, eye, 0, occ_only.data(), nullptr, 2);
  if (rc == CRN_OK) rc = crn_voxel_visibility_cpu(grid.data(), st, 1, 1, D, H, W, eye, CRN_VV_COUNT_STEPS, occ.data(), steps.data(), 2);
  if (rc != CRN_OK) { std::printf("%s: status %d\n", what, rc); return 1; }
  size_t hidden = 0;
  int64_t total = 0;
  for (size_t v = 0; v < S; ++v) {
    const bool ok = occ[v] == occ_only[v] && (first[v] >= 0) == (occ[v] != 0) && (first[v] < 0 || (first[v] < (int64_t)S && grid[first[v]])) &&
                    steps[v] >= 0 && steps[v] <= D + H + W;
    if (!ok) { std::printf("%s: voxel %zu inconsistent\n", what, v); return 1; }
    hidden += occ[v];
    total += steps[v];
  }
  std::printf("%s: %zu of %zu voxels occluded, %lld steps\n", what, hidden, S, (long long)total);
  return 0;
}

int main() {
  int bad = 0;
  for (int c = 0; c < 8; ++c) {
    const int32_t e[3] = {(c & 1) ? CRN_VV_MAX_EYE : -CRN_VV_MAX_EYE, (c & 2) ? CRN_VV_MAX_EYE : -CRN_VV_MAX_EYE,
                          (c & 4) ? CRN_VV_MAX_EYE : -CRN_VV_MAX_EYE};
    bad += run(3, 5, 70, 0.1, e, "range limit");
  }
  const int32_t eyes[4][3] = {{16 * 256, 16 * 256, -28 * 256 + 77}, {10 * 256 + 3, 20 * 256 + 99, 7 * 256 + 200},
                              {40 * 256 + 128, -3 * 256 + 128, 12 * 256 + 128}, {CRN_VV_MAX_EYE, 0, -CRN_VV_MAX_EYE}};
  for (const auto& e : eyes) bad += run(32, 32, 32, 0.05, e, "32^3");
  const int32_t beyond[3] = {CRN_VV_MAX_EYE + 1, 0, 0};
  uint8_t g = 0, o = 0;
  const int64_t st1[4] = {1, 1, 1, 1};
  if (crn_voxel_visibility_cpu(&g, st1, 1, 1, 1, 1, 1, beyond, 0, &o, nullptr, 1) != CRN_EINVAL) { std::printf("an eye beyond the range was accepted\n"); ++bad; }
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad ? 1 : 0;
}
