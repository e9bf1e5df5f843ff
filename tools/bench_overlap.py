#!/usr/bin/env python
"""Label overlaps (corenet_amd.voxel_overlap): the counting kernel and the whole label_overlaps call,
against the torch formulation on the same tensors and the library's single-threaded host twin.

  python tools/bench_overlap.py [--iters 10] [--small]      # device-event times, JSON lines

Workloads: the connected components (6-connectivity, by value) of 4 x 128^3 and 52 x 256^3 semantic label grids -- the
two fixture scenes voxelized at that resolution and tiled -- against their instance ground truth (mesh index + 1), both
int32: the LDS path.  One adversarial pair on the global path: 256^3 voxels, a = (d + h + w) mod 200 and
b = (3 d + 5 h + 7 w) mod 150, so no two neighbours along w share a pair and every voxel is one 64-bit atomic into a
table of 30000 entries.  --small leaves the 52 x 256^3 workload out.

Per case: milliseconds (median, min, max over --iters runs after two warm-up runs) of
  count            the native call alone (two memsets and the kernel): what DESIGN section 20 prices against HBM;
  label_overlaps   the whole call with num_a / num_b given: the read-back of num, the kernel, torch.nonzero and the CSR;
  torch            per grid, bincount(a.long() * (num_b + 1) + b.long(), minlength = table size): int64 keys, as
                   voxel_metrics.confusion_matrix builds them;
the floor of reading both grids once at the measured copy rate, and the twin on one thread for ONE grid (best of 3)."""
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


def fixture_pair(resolution, tile):
  """(component labels int32 [2 * tile, r, r, r], instance ground truth, num_components, meshes per scene)."""
  from corenet_amd import pipeline, voxel_components
  from corenet_amd.data import batched_example as B, dataset as D
  root = os.path.join(ROOT, "tests", "golden", "n2_dataset")
  ds = D.CoReNetDatasetImpl(os.path.join(root, "dataset.json"), os.path.join(root, "meshes"))
  ex = B.batch([ds[0], ds[1]])
  sem = pipeline.voxelize_batch(ex, "semantic", resolution=(resolution,) * 3).grid
  inst = B.voxelize(ex, (resolution,) * 3, B.voxel_content_mesh_index, image_resolution_multiplier=8).grid
  comps = voxel_components.connected_components(sem.repeat(tile, 1, 1, 1).contiguous(), 6)
  meshes = t.tensor([len(v) for v in ex.mesh_num_tri], dtype=t.int64, device=sem.device).repeat(tile)
  return comps.labels, inst.repeat(tile, 1, 1, 1).contiguous(), comps.num_components, meshes


def report(name, a, b, num_a, num_b, iters, M):
  from corenet_amd.backend import default_backend
  N, voxels = a.shape[0], a.numel()
  host = t.stack([num_a, num_b]).cpu()
  entries = ((host[0] + 1) * (host[1] + 1)).tolist()
  offsets = t.zeros(N + 1, dtype=t.int64)
  offsets[1:] = t.cumsum(t.tensor(entries), 0)
  table = t.empty(int(offsets[N]), dtype=t.int64, device=a.device)
  bad = t.empty(N, dtype=t.int64, device=a.device)
  be = default_backend()
  cmed, clo, chi, _ = timed(lambda: be.voxel_overlap(a, b, num_a, num_b, offsets, table, bad), iters)
  wmed, wlo, whi, ov = timed(lambda: M.label_overlaps(a, b, num_a, num_b), iters)
  widths = (host[1] + 1).tolist()

  def torch_tables():
    return [t.bincount(a[n].flatten().long() * widths[n] + b[n].flatten().long(), minlength=entries[n]) for n in range(N)]
  tmed, tlo, thi, tabs = timed(torch_tables, iters)
  assert t.equal(t.cat(tabs), table) and int(bad.sum()) == 0 and int(ov.count.sum()) == voxels
  one_a, one_b, one_na, one_nb = a[:1].cpu(), b[:1].cpu(), num_a[:1].cpu(), num_b[:1].cpu()
  threads = t.get_num_threads()
  t.set_num_threads(1)
  twin = host_ms(lambda: M.label_overlaps(one_a, one_b, one_na, one_nb))
  t.set_num_threads(threads)
  floor = (a.element_size() + b.element_size()) * voxels / HBM_MEASURED * 1e3
  lds = M.overlap_tiles()[1]
  res = {"grids": N, "shape": list(a.shape[1:]), "dtypes": [str(a.dtype), str(b.dtype)],
         "table_entries_max": max(entries), "path": "lds" if max(entries) <= lds else "global" if min(entries) > lds else "mixed",
         "pairs": int(ov.count.numel()), "background_share": float(ov.count[(ov.a == 0) & (ov.b == 0)].sum()) / voxels,
         "count_ms_median": cmed, "count_ms_min": clo, "count_ms_max": chi,
         "label_overlaps_ms_median": wmed, "label_overlaps_ms_min": wlo, "label_overlaps_ms_max": whi,
         "torch_bincount_ms_median": tmed, "torch_bincount_ms_min": tlo, "torch_bincount_ms_max": thi,
         "bytes_per_voxel": a.element_size() + b.element_size(), "hbm_floor_ms_at_6.29TBps": floor,
         "count_over_hbm_floor": cmed / floor, "read_rate_TBps": (a.element_size() + b.element_size()) * voxels / (cmed * 1e-3) / 1e12,
         "torch_over_count": tmed / cmed, "torch_over_label_overlaps": tmed / wmed,
         "gpu_count_ms_per_grid": cmed / N, "twin_1_thread_ms_per_grid": twin, "twin_over_gpu_per_grid": twin / (cmed / N)}
  print(json.dumps({name: res}), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=10)
  ap.add_argument("--small", action="store_true")
  args = ap.parse_args()
  if not t.cuda.is_available():
    raise SystemExit("bench_overlap needs a GPU: it measures the kernel")
  from corenet_amd import voxel_overlap as M
  print(json.dumps({"tiles": M.overlap_tiles(), "iters": args.iters}), flush=True)
  report("fixture_4x128", *fixture_pair(128, 2), args.iters, M)
  if not args.small:
    report("fixture_52x256", *fixture_pair(256, 26), args.iters, M)
    t.cuda.empty_cache()
  d, h, w = t.meshgrid(t.arange(256), t.arange(256), t.arange(256), indexing="ij")
  a = ((d + h + w) % 200).to(t.int32)[None].cuda()
  b = ((3 * d + 5 * h + 7 * w) % 150).to(t.int32)[None].cuda()
  report("adversarial_1x256", a, b, t.tensor([199], device="cuda"), t.tensor([149], device="cuda"), args.iters, M)


if __name__ == "__main__":
  main()
