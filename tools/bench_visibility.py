#!/usr/bin/env python
"""Voxel visibility from the camera (corenet_amd.voxel_visibility): the pack and walk passes with and
without `first`, through the coarse map and flat, against the library's host twin.

  python tools/bench_visibility.py [--iters 10] [--small] [--out profiles/r14_visibility_bench.txt]
  rocprofv3 --kernel-trace --output-format csv -d DIR -o vv -- python tools/bench_visibility.py --trace fixture_52x256
  python tools/bench_visibility.py --split DIR/.../vv_kernel_trace.csv [--out ...]     # per-kernel split of that run

Workloads: those of tools/bench_distance.py -- 4 x 128^3 and 52 x 256^3 semantic label grids (int32, the two fixture
scenes voxelized and tiled), a 256^3 3-D checkerboard (uint8) and one 256^3 grid with a single occupied voxel -- seen by
the documented camera: the eye 0.8667 grid edges in front of the centre of the z = 0 face.  --small leaves the
52 x 256^3 workload out.

Per case: milliseconds (median, min, max over --iters runs after two warm-up runs, device events) of occlusion() without
and with first, in the coarse and the flat form; the share of occluded voxels; the steps of all walks to the grid
boundary, which the host twin counts on one grid (the work of the runs with first; without first a walk ends at its
first hit, so that is an upper bound there) and steps per second from them; the bytes the passes move by construction
(not a hardware counter): the grid read once, the packed fine bits and the coarse map written, the coarse map staged
once per workgroup of the walk pass, 1 B (5 B with first) written per voxel, and for the flat form one 8 B word looked
up per step, from L2; the twin on one grid with 1 and 16 threads."""
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

EYE_IN_EDGES = (0.5, 0.5, -0.8666666)      # the documented camera, in grid edges


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
  return {"ms_median": float(np.median(ts)), "ms_min": min(ts), "ms_max": max(ts)}, out


def host_ms(fn):
  t0 = time.perf_counter()
  out = fn()
  return (time.perf_counter() - t0) * 1e3, out


def fixture_labels(resolution):
  from corenet_amd import pipeline
  from corenet_amd.data import batched_example as B, dataset as D
  root = os.path.join(ROOT, "tests", "golden", "n2_dataset")
  ds = D.CoReNetDatasetImpl(os.path.join(root, "dataset.json"), os.path.join(root, "meshes"))
  return pipeline.voxelize_batch(B.batch([ds[0], ds[1]]), "semantic", resolution=(resolution,) * 3).grid


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
    g[0, 128, 128, 128] = 1
    yield "single_voxel_1x256", g.cuda()


def eye_of(grid):
  return [e * s for e, s in zip(EYE_IN_EDGES, (grid.shape[3], grid.shape[2], grid.shape[1]))]


def report(name, grid, iters, M, emit):
  brick, cap, wg_words = M.visibility_tiles()
  n, voxels, item = grid.shape[0], grid.numel(), grid.element_size()
  D, H, W = grid.shape[1:]
  eye = eye_of(grid)
  words = (W + 63) // 64
  fine = n * D * H * words * 8
  bricks = ((D + brick - 1) // brick) * ((H + brick - 1) // brick) * ((W + brick - 1) // brick)
  coarse = n * (((bricks + 31) // 32 + 3) // 4 * 4) * 4                     # 32-bit words, a multiple of 4 per grid
  groups = n * -(-(D * H * words) // wg_words)
  res = {"grids": n, "shape": [D, H, W], "dtype": str(grid.dtype), "eye": eye, "occupancy": float((grid > 0).float().mean()),
         "packed_fine_bytes": fine, "packed_coarse_bytes": coarse, "coarse_fits_lds": coarse // n <= cap,
         "coarse_bytes_staged_by_all_workgroups": groups * (coarse // n), "grid_bytes_read": voxels * item}
  for form, flags in (("coarse", 0), ("flat", M.FLAT)):
    for first in (False, True):
      r, out = timed(lambda: M.occlusion(grid, eye, return_first=first, flags=flags), iters)
      r["output_bytes"] = voxels * (5 if first else 1)
      res[form + ("_first" if first else "")] = r
  res["occluded_share"] = float(out.occluded.float().mean())
  del out
  one = grid[:1].cpu()
  threads = t.get_num_threads()
  t.set_num_threads(1)
  res["twin_1_thread_ms_per_grid_first"], _ = host_ms(lambda: M.occlusion(one, eye, return_first=True))
  t.set_num_threads(16)
  res["twin_16_threads_ms_per_grid_first"], _ = host_ms(lambda: M.occlusion(one, eye, return_first=True))
  res["twin_16_threads_ms_per_grid"], _ = host_ms(lambda: M.occlusion(one, eye))
  _, steps = host_ms(lambda: M.walk_steps(one, eye))
  t.set_num_threads(threads)
  # every workload tiles one or two scenes: the first grid and the second stand for all even and odd ones
  per_grid = [int(steps.sum())]
  if n > 1:
    per_grid.append(int(M.walk_steps(grid[1:2].cpu(), eye).sum()))
  total = sum(per_grid[i % len(per_grid)] for i in range(n))
  res["steps_to_the_boundary"] = total
  res["steps_per_voxel"] = total / voxels
  res["flat_lookup_bytes_first"] = total * 8
  for form in ("coarse", "flat"):
    res[form + "_first"]["steps_per_s"] = total / (res[form + "_first"]["ms_median"] * 1e-3)
  res["twin_1_thread_steps_per_s_first"] = per_grid[0] / (res["twin_1_thread_ms_per_grid_first"] * 1e-3)
  res["twin_16_threads_steps_per_s_first"] = per_grid[0] / (res["twin_16_threads_ms_per_grid_first"] * 1e-3)
  res["twin_1_thread_over_gpu_per_grid_first"] = res["twin_1_thread_ms_per_grid_first"] / (res["coarse_first"]["ms_median"] / n)
  emit({name: res})


def split(path, emit):
  """Per-kernel durations of a rocprofv3 --kernel-trace csv: calls, median and total microseconds of the vv_ kernels."""
  by = {}
  with open(path, newline="") as f:
    for row in csv.DictReader(f):
      k = row["Kernel_Name"]
      if "vv_" in k:
        by.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
  for k, v in sorted(by.items()):
    emit({"kernel": k, "calls": len(v), "us_median": float(np.median(v)), "us_min": min(v), "us_total": sum(v)})


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=10)
  ap.add_argument("--small", action="store_true")
  ap.add_argument("--trace", default=None, help="run one workload three times per form, nothing else (for rocprofv3)")
  ap.add_argument("--split", default=None, help="summarise a rocprofv3 kernel-trace csv")
  ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
  a = ap.parse_args()

  def emit(obj):
    line = json.dumps(obj)
    print(line, flush=True)
    if a.out:
      with open(a.out, "a") as f:
        f.write(line + "\n")
  if a.split:
    return split(a.split, emit)
  if not t.cuda.is_available():
    raise SystemExit("bench_visibility needs a GPU: it measures the kernels")
  from corenet_amd import voxel_visibility as M
  if a.trace:
    for name, grid in workloads(False, a.trace):
      eye = eye_of(grid)
      for flags in (0, M.FLAT):
        for first in (False, True):
          for _ in range(3):
            M.occlusion(grid, eye, return_first=first, flags=flags)
      t.cuda.synchronize()
    return
  emit({"tiles": M.visibility_tiles(), "iters": a.iters})
  for name, grid in workloads(a.small):
    report(name, grid, a.iters, M, emit)


if __name__ == "__main__":
  main()
