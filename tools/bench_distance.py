#!/usr/bin/env python
"""Exact Euclidean distance transform (corenet_amd.voxel_distance): the three passes per target mode,
with and without the index, against the library's single-threaded host twin and, where scipy is importable,
scipy.ndimage.distance_transform_edt.

  python tools/bench_distance.py [--iters 10] [--small]        # device-event times, JSON lines
  rocprofv3 --kernel-trace --output-format csv -d DIR -o vd -- python tools/bench_distance.py --trace fixture_52x256
  python tools/bench_distance.py --split DIR/.../vd_kernel_trace.csv          # per-kernel split of that run

Workloads: those of tools/bench_components.py -- 4 x 128^3 and 52 x 256^3 semantic label grids (int32, the two fixture
scenes voxelized and tiled) and a 256^3 3-D checkerboard (uint8) -- plus one 256^3 grid with a single target voxel in a
corner: every row, column and plane that holds a target holds it far away, the worst case for row skipping in the d pass
and for the twin's early exit.  --small leaves the 52 x 256^3 workload out.

Per case and mode: milliseconds (median, min, max over --iters runs after two warm-up runs) without and with the index;
the bytes per voxel the passes move by construction (not a hardware counter): the row pass reads the grid and writes,
reads back and rewrites 4 B, each line pass reads and writes 4 B, the index adds 4 B in the row pass and a gathered read
and a write per line pass; the algorithmic minimum is the grid read once and 4 B (8 B) written; the share of the 6.29 TB/s
measured copy rate each implies; the (i, j) pairs per column the line passes execute against all pairs -- rows (planes) j
without a target in the 64 columns of a workgroup are skipped (after the row pass a row has a target everywhere or
nowhere, so this count is exact), and a wave ends its walk once the squared step reaches its largest value (estimated
from the final values: a lower estimate).  The host figures are per grid, one grid on one thread."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch as t

HBM_MEASURED = 6.29e12        # bytes/s, float4 copy on this chip (the spec rate is 8.0e12)
MODES = ("foreground", "background", "surface")


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


def host_ms(fn, repeats=2):
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


def counted_bytes(item, passes, index):
  return item + 12 + 8 * passes + (4 + 8 * passes if index else 0)


def _window_pairs(values, active, R):
  """values [M, L, C] (line axis in the middle, C columns in workgroup order), active bool [M, L]: the pairs a pass runs
  when every wave (R outputs x 64 columns) walks the active rows within floor(sqrt(its largest final value)) of its
  outputs.  A lower estimate: the kernel's bound starts open and is refreshed every 16 rows."""
  M, L, C = values.shape
  if L % R or C % 64:
    return None
  top = values.reshape(M, L // R, R, C // 64, 64).amax((2, 4)).to(t.float64)          # [M, chunks, groups]
  rad = top.sqrt().floor().clamp(max=L).to(t.int64)
  i0 = (t.arange(L // R, device=values.device) * R)[None, :, None]
  lo, hi = (i0 - rad).clamp(min=0), (i0 + R - 1 + rad).clamp(max=L - 1)
  cs = t.cat([t.zeros((M, 1), dtype=t.int64, device=values.device), active.to(t.int64).cumsum(1)], 1)   # [M, L + 1]
  count = t.gather(cs[:, :, None].expand(M, L + 1, top.shape[2]), 1, hi + 1) - t.gather(cs[:, :, None].expand(M, L + 1, top.shape[2]), 1, lo)
  return int(count.sum()) * R * 64


def pairs(d2, M):
  """(i, j) pairs per column of the two line passes, from the result of a call (its zeros are the targets): after row
  skipping alone (exact), a lower estimate with the early exit, and all pairs."""
  N, D, H, W = d2.shape
  R = M.distance_tiles()[0]
  target = d2 == 0
  row_any = target.any(-1)                                    # [N, D, H]
  plane_any = row_any.any(-1)                                 # [N, D]
  skipped = int(row_any.sum()) * H * W + int(plane_any.sum()) * D * H * W
  after_h = M.squared_distance_to(target.reshape(N * D, 1, H, W).to(t.uint8)).d2      # every plane a grid of its own
  ph = _window_pairs(after_h.reshape(N * D, H, W), row_any.reshape(N * D, H), R)
  pd = _window_pairs(d2.reshape(N, D, H * W), plane_any, R)
  return skipped, (None if ph is None or pd is None else ph + pd), N * D * H * W * (H + D)


def workloads(small, only=None):
  def want(name):
    return only is None or only == name
  if want("fixture_4x128"):
    yield "fixture_4x128", fixture_labels(128).repeat(2, 1, 1, 1).contiguous()
  if want("fixture_52x256") and not (small and only is None):
    yield "fixture_52x256", fixture_labels(256).repeat(26, 1, 1, 1).contiguous()
    t.cuda.empty_cache()
  if want("checkerboard_1x256"):
    d, h, w = t.meshgrid(t.arange(256), t.arange(256), t.arange(256), indexing="ij")
    yield "checkerboard_1x256", (((d + h + w) % 2) == 0).to(t.uint8)[None].cuda()
  if want("single_voxel_1x256"):
    g = t.zeros((1, 256, 256, 256), dtype=t.uint8)
    g[0, 0, 0, 0] = 1
    yield "single_voxel_1x256", g.cuda()


def report(name, grid, iters, M, host_modes):
  n, voxels, item = grid.shape[0], grid.numel(), grid.element_size()
  passes = sum(1 for s in grid.shape[1:3] if s > 1)
  res = {"grids": n, "shape": list(grid.shape[1:]), "dtype": str(grid.dtype), "occupancy": float((grid > 0).float().mean())}
  for mode in MODES:
    med, lo, hi, out = timed(lambda: M.squared_distance_to(grid, mode), iters)
    imed, ilo, ihi, _ = timed(lambda: M.squared_distance_to(grid, mode, return_index=True), iters)
    done, early, total = pairs(out.d2, M)
    del out, _
    floor = (item + 4) * voxels / HBM_MEASURED * 1e3
    r = {"ms_median": med, "ms_min": lo, "ms_max": hi, "index_ms_median": imed, "index_ms_min": ilo, "index_ms_max": ihi,
         "voxels_per_s": voxels / (med * 1e-3), "min_bytes_per_voxel": item + 4, "counted_bytes_per_voxel": counted_bytes(item, passes, False),
         "counted_bytes_per_voxel_with_index": counted_bytes(item, passes, True),
         "hbm_share_of_counted_bytes_vs_6.29TBps": counted_bytes(item, passes, False) * voxels / (med * 1e-3) / HBM_MEASURED,
         "hbm_share_of_counted_bytes_with_index": counted_bytes(item, passes, True) * voxels / (imed * 1e-3) / HBM_MEASURED,
         "hbm_floor_ms_at_6.29TBps": floor, "time_over_hbm_floor": med / floor,
         "index_time_over_hbm_floor": imed / ((item + 8) * voxels / HBM_MEASURED * 1e3),
         "pairs_after_row_skipping": done, "pairs_with_early_exit_lower_estimate": early, "pairs_without_skipping": total,
         "pairs_share_after_row_skipping": done / total, "pairs_share_with_early_exit": None if early is None else early / total, "gpu_ms_per_grid": med / n}
    if mode in host_modes:
      one = grid[:1].cpu()
      threads = t.get_num_threads()
      t.set_num_threads(1)
      r["twin_1_thread_ms_per_grid"] = host_ms(lambda: M.squared_distance_to(one, mode), repeats=2 if one.numel() <= 128 ** 3 else 1)
      t.set_num_threads(threads)
      r["twin_over_gpu_per_grid"] = r["twin_1_thread_ms_per_grid"] / (med / n)
      try:
        from scipy import ndimage
      except ImportError:
        r["scipy_ms_per_grid"] = None
      else:
        a = one[0].numpy() > 0
        inv = a if mode == "background" else ~a              # edt measures the distance to the zeros
        if mode != "surface":
          r["scipy_ms_per_grid"] = host_ms(lambda: ndimage.distance_transform_edt(inv), repeats=1)
          r["scipy_over_gpu_per_grid"] = r["scipy_ms_per_grid"] / (med / n)
    res[mode] = r
  print(json.dumps({name: res}), flush=True)


def split(path):
  """Per-kernel durations of a rocprofv3 --kernel-trace csv: calls, median and total microseconds of the vd_ kernels."""
  by = {}
  with open(path, newline="") as f:
    for row in csv.DictReader(f):
      k = row["Kernel_Name"]
      if "vd_" in k:
        by.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
  for k, v in sorted(by.items()):
    print(json.dumps({"kernel": k, "calls": len(v), "us_median": float(np.median(v)), "us_min": min(v), "us_total": sum(v)}), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=10)
  ap.add_argument("--small", action="store_true")
  ap.add_argument("--trace", default=None, help="run one workload three times per mode and form, nothing else (for rocprofv3)")
  ap.add_argument("--split", default=None, help="summarise a rocprofv3 kernel-trace csv")
  a = ap.parse_args()
  if a.split:
    return split(a.split)
  if not t.cuda.is_available():
    raise SystemExit("bench_distance needs a GPU: it measures the kernels")
  from corenet_amd import voxel_distance as M
  if a.trace:
    for name, grid in workloads(False, a.trace):
      for mode in MODES:
        for index in (False, True):
          for _ in range(3):
            M.squared_distance_to(grid, mode, return_index=index)
      t.cuda.synchronize()
    return
  print(json.dumps({"tiles": M.distance_tiles(), "iters": a.iters}), flush=True)
  for name, grid in workloads(a.small):
    # the twin and scipy on one 256^3 grid take seconds per mode: foreground everywhere, all modes on the small fixture
    report(name, grid, a.iters, M, MODES if name == "fixture_4x128" else ("foreground",))


if __name__ == "__main__":
  main()
