#!/usr/bin/env python
"""Configuration histogram (corenet_amd.voxel_topology): the native call against the torch formulation
on the same tensors and the floor of reading the grids once.

  python tools/bench_topology.py [--iters 10] [--small]      # device-event times, JSON lines

Workloads: 4 x 128^3 and 52 x 256^3 semantic label grids -- the two fixture scenes voxelized at that resolution and
tiled, so with the fixture's share of background -- as int32 and as uint8, and one adversarial grid: a 256^3 checkerboard
of four labels with no two equal neighbours on any axis, so that every cell is mixed and ends every run.  --small leaves
the 52 x 256^3 workloads out.

Per case: milliseconds (median, min, max over --iters runs after two warm-up runs) of
  native   crn_voxel_topology alone (two memsets, the counting kernel, the kernel that derives bin 0);
  torch    per grid and row: the zero-padded mask, eight shifted slices combined by shift-or into the cell codes, bincount;
           checked equal to the kernel's table in the same run;
the floor of reading the grids once, at the 6.29 TB/s copy rate of profiles/r15_overlap_bench.txt and at the rate of a
device-to-device copy of 1 GiB measured in this run (read plus write bytes over time), and the twin on one thread for ONE
grid (best of 3)."""
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


def copy_rate(iters):
  src = t.ones(1 << 28, dtype=t.int32, device="cuda")
  dst = t.empty_like(src)
  med = timed(lambda: dst.copy_(src), iters)[0]
  return 2 * src.numel() * 4 / (med * 1e-3)


def fixture_grids(resolution, tile):
  from corenet_amd import pipeline
  from corenet_amd.data import batched_example as B, dataset as D
  root = os.path.join(ROOT, "tests", "golden", "n2_dataset")
  ds = D.CoReNetDatasetImpl(os.path.join(root, "dataset.json"), os.path.join(root, "meshes"))
  sem = pipeline.voxelize_batch(B.batch([ds[0], ds[1]]), "semantic", resolution=(resolution,) * 3).grid
  return sem.to(t.int32).repeat(tile, 1, 1, 1).contiguous()


def torch_table(grid, L):
  """int64 [N, L + 1, 256] through torch alone."""
  N, D, H, W = grid.shape
  out = []
  for n in range(N):
    for row in range(L + 1):
      mask = t.nn.functional.pad((grid[n] != 0) if row == 0 else (grid[n] == row), (1, 1, 1, 1, 1, 1)).to(t.uint8)
      code = t.zeros((D + 1, H + 1, W + 1), dtype=t.uint8, device=grid.device)
      for i in (0, 1):
        for j in (0, 1):
          for k in (0, 1):
            code |= mask[i:i + D + 1, j:j + H + 1, k:k + W + 1] << (4 * i + 2 * j + k)
      out.append(t.bincount(code.reshape(-1), minlength=256))
  return t.stack(out).reshape(N, L + 1, 256)


def report(name, grid, L, iters, M, rate):
  from corenet_amd.backend import default_backend
  N, voxels = grid.shape[0], grid.numel()
  table = t.empty((N, L + 1, 256), dtype=t.int64, device=grid.device)
  bad = t.empty(N, dtype=t.int64, device=grid.device)
  be = default_backend()
  nmed, nlo, nhi, _ = timed(lambda: be.voxel_topology(grid, L, False, table, bad), iters)
  tmed, tlo, thi, ref = timed(lambda: torch_table(grid, L), iters)
  assert t.equal(ref, table) and int(bad.sum()) == 0
  one = grid[:1].cpu()
  threads = t.get_num_threads()
  t.set_num_threads(1)
  twin = host_ms(lambda: M.configuration_histogram(one, L))
  t.set_num_threads(threads)
  nbytes = grid.element_size() * voxels
  floor, floor_here = nbytes / HBM_MEASURED * 1e3, nbytes / rate * 1e3
  res = {"grids": N, "shape": list(grid.shape[1:]), "dtype": str(grid.dtype), "num_labels": L,
         "background_share": float((grid == 0).sum()) / voxels, "full_cell_share": float(table[:, 0, 255].sum()) / float(table[:, 0].sum()),
         "native_ms_median": nmed, "native_ms_min": nlo, "native_ms_max": nhi,
         "torch_ms_median": tmed, "torch_ms_min": tlo, "torch_ms_max": thi, "torch_over_native": tmed / nmed,
         "bytes_per_voxel": grid.element_size(), "hbm_floor_ms_at_6.29TBps": floor, "native_over_hbm_floor": nmed / floor,
         "hbm_floor_ms_at_this_runs_copy_rate": floor_here, "native_over_this_runs_floor": nmed / floor_here,
         "read_rate_TBps": nbytes / (nmed * 1e-3) / 1e12, "gpu_ms_per_grid": nmed / N, "twin_1_thread_ms_per_grid": twin}
  print(json.dumps({name: res}), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=10)
  ap.add_argument("--small", action="store_true")
  args = ap.parse_args()
  if not t.cuda.is_available():
    raise SystemExit("bench_topology needs a GPU: it measures the kernel")
  from corenet_amd import voxel_topology as M
  rate = copy_rate(args.iters)
  print(json.dumps({"tiles": M.topology_tiles()._asdict(), "iters": args.iters, "copy_rate_TBps_this_run": rate / 1e12}), flush=True)
  for name, resolution, tile in (("fixture_4x128", 128, 2), ("fixture_52x256", 256, 26)):
    if args.small and resolution == 256:
      continue
    grid = fixture_grids(resolution, tile)
    L = int(grid.max())
    report(name + "_int32", grid, L, args.iters, M, rate)
    report(name + "_uint8", grid.to(t.uint8), L, args.iters, M, rate)
    del grid
    t.cuda.empty_cache()
  d, h, w = t.meshgrid(t.arange(256), t.arange(256), t.arange(256), indexing="ij")
  board = (1 + (d + h + w) % 2 + 2 * ((d + h) % 2))[None].to(t.int32).cuda()
  report("adversarial_1x256_int32", board, 4, args.iters, M, rate)


if __name__ == "__main__":
  main()
