#!/usr/bin/env python
"""Voxel connected components (corenet_amd.voxel_components): the labelling kernels with and without
component_stats, against the library's single-threaded host twin and, where scipy is importable, scipy.ndimage.label.

  python tools/bench_components.py [--iters 10] [--small]      # device-event times, JSON lines

Workloads: 4 x 128^3 and 52 x 256^3 semantic label grids (int32) -- the two fixture scenes voxelized at that resolution
and tiled -- with 6-connectivity by value, and one adversarial grid: a 256^3 3-D checkerboard (uint8), every foreground
voxel its own component at 6-connectivity.  --small leaves the 52 x 256^3 workload out.

Per case: milliseconds (median, min, max over --iters runs after two warm-up runs), voxels/s, the bytes per voxel the six
launches move by construction (counted from the kernel structure below, not from hardware counters) against the
algorithmic minimum (grid read once + 4 B label written), and the share of the HBM rate each implies.  The host figures
are per grid: the twin labels one grid on one thread, scipy.ndimage.label one grid of the binary mask per class."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch as t

HBM_MEASURED = 6.29e12        # bytes/s, float4 copy on this chip (the spec rate is 8.0e12)
HBM_SPEC = 8.0e12
# bytes per voxel by construction: brick (grid read, 4 B parent written), flatten (parent read, label written), number
# (label read), relabel (label read, number gathered, label written); the seam pass touches the brick faces only and the
# root walks of flatten and relabel mostly hit parents that are already in cache
COUNTED_EXTRA = 4 + 4 + 4 + 4 + 4 + 4 + 4
STATS_EXTRA = 4               # component_stats reads the labels once


def timed(fn, iters, warm=2):
  for _ in range(warm):
    out = fn()
  t.cuda.synchronize()
  ts = []
  for _ in range(iters):
    e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    t.cuda.synchronize()
    ts.append(e0.elapsed_time(e1))
  return float(np.median(ts)), min(ts), max(ts), out


def host_ms(fn, repeats=3):
  best = float("inf")
  for _ in range(repeats):
    t0 = time.perf_counter()
    fn()
    best = min(best, (time.perf_counter() - t0) * 1e3)
  return best


def fixture_labels(resolution):
  from corenet_amd import pipeline
  from corenet_amd.data import batched_example as B, dataset as D
  root = os.path.join(ROOT, "tests", "golden", "n2_dataset")
  ds = D.CoReNetDatasetImpl(os.path.join(root, "dataset.json"), os.path.join(root, "meshes"))
  return pipeline.voxelize_batch(B.batch([ds[0], ds[1]]), "semantic", resolution=(resolution,) * 3).grid


def report(name, grid, connectivity, iters, M):
  n, voxels = grid.shape[0], grid.numel()
  item = grid.element_size()
  med, lo, hi, comps = timed(lambda: M.connected_components(grid, connectivity), iters)
  smed, slo, shi, _ = timed(lambda: M.component_stats(M.connected_components(grid, connectivity), grid), iters)
  one = grid[:1].cpu()
  threads = t.get_num_threads()
  t.set_num_threads(1)
  twin = host_ms(lambda: M.connected_components(one, connectivity))
  twin_stats = host_ms(lambda: M.component_stats(M.connected_components(one, connectivity), one))
  t.set_num_threads(threads)
  res = {"grids": n, "shape": list(grid.shape[1:]), "dtype": str(grid.dtype), "connectivity": connectivity,
         "occupancy": float((grid > 0).float().mean()), "components": int(comps.num_components.sum()),
         "labels_ms_median": med, "labels_ms_min": lo, "labels_ms_max": hi, "voxels_per_s": voxels / (med * 1e-3),
         "labels_and_stats_ms_median": smed, "labels_and_stats_ms_min": slo, "labels_and_stats_ms_max": shi,
         "voxels_per_s_with_stats": voxels / (smed * 1e-3),
         "min_bytes_per_voxel": item + 4, "counted_bytes_per_voxel": item + COUNTED_EXTRA,
         "counted_bytes_per_voxel_with_stats": item + COUNTED_EXTRA + STATS_EXTRA,
         "hbm_share_of_counted_bytes_vs_6.29TBps": (item + COUNTED_EXTRA) * voxels / (med * 1e-3) / HBM_MEASURED,
         "hbm_share_of_counted_bytes_vs_8TBps_spec": (item + COUNTED_EXTRA) * voxels / (med * 1e-3) / HBM_SPEC,
         "hbm_floor_ms_at_6.29TBps": (item + 4) * voxels / HBM_MEASURED * 1e3,
         "time_over_hbm_floor": med / ((item + 4) * voxels / HBM_MEASURED * 1e3),
         "gpu_ms_per_grid": med / n, "twin_1_thread_ms_per_grid": twin, "twin_1_thread_ms_per_grid_with_stats": twin_stats,
         "twin_over_gpu_per_grid": twin / (med / n)}
  try:
    from scipy import ndimage
  except ImportError:
    res["scipy_ms_per_grid"] = None
  else:
    a = one[0].numpy()
    structure = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])
    values = [int(v) for v in np.unique(a) if v > 0]
    res["scipy_ms_per_grid"] = host_ms(lambda: [ndimage.label(a == v, structure) for v in values], repeats=2)
    res["scipy_over_gpu_per_grid"] = res["scipy_ms_per_grid"] / (med / n)
  print(json.dumps({name: res}), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=10)
  ap.add_argument("--small", action="store_true")
  a = ap.parse_args()
  if not t.cuda.is_available():
    raise SystemExit("bench_components needs a GPU: it measures the kernels")
  from corenet_amd import voxel_components as M
  print(json.dumps({"bricks": M.component_bricks(), "iters": a.iters}), flush=True)
  g128 = fixture_labels(128)
  report("fixture_4x128", g128.repeat(2, 1, 1, 1).contiguous(), 6, a.iters, M)
  del g128
  if not a.small:
    g256 = fixture_labels(256)
    report("fixture_52x256", g256.repeat(26, 1, 1, 1).contiguous(), 6, a.iters, M)
    del g256
    t.cuda.empty_cache()
  d, h, w = t.meshgrid(t.arange(256), t.arange(256), t.arange(256), indexing="ij")
  board = (((d + h + w) % 2) == 0).to(t.uint8)[None].cuda()
  report("checkerboard_1x256", board, 6, a.iters, M)


if __name__ == "__main__":
  main()
