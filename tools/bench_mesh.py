#!/usr/bin/env python
"""Marching cubes (corenet_amd.visualization) on near-binary synthetic grids: a clipped signed distance of seeded random
ellipsoids, the shape of a predicted pmf.

  python tools/bench_mesh.py [--iters 10]          # device-event time per call, active-cell fraction, host twin time
  rocprofv3 --kernel-trace --stats -d DIR -o mc -- python tools/bench_mesh.py --iters 5     # per-pass kernel times

Workloads: 4 objects at 128^3 (h7 eval), 52 objects at 256^3 (m7 x2 super-resolution at B = 4).  The count pass reads
the grid once (4 bytes per sample); its share of the 6.3 TB/s achievable HBM rate is derived from the kernel trace
(tools/bench_mesh.py --stats DIR/mc_kernel_stats.csv)."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch as t

WORKLOADS = [("h7_eval_4x128", 4, 128), ("m7_x2_52x256", 52, 256)]


def fields(n, size, seed):
  import mesh_check as MC
  distinct = min(n, 4)
  base = t.from_numpy(MC.ellipsoid_fields(distinct, size, seed)).cuda()
  g = t.empty(n, size, size, size, device="cuda")
  for i in range(n):
    g[i] = base[i % distinct].roll(shifts=(i, 2 * i, 3 * i), dims=(0, 1, 2))
  return g


def active_fraction(g):
  p = t.nn.functional.pad((g > 0.5).float(), [1] * 6)[:, None]
  mx = t.nn.functional.max_pool3d(p, 2, 1)
  mn = -t.nn.functional.max_pool3d(-p, 2, 1)
  return float((mx != mn).float().mean())


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=10)
  ap.add_argument("--stats", help="summarise a rocprofv3 kernel_stats.csv of a run of this script instead")
  a = ap.parse_args()
  if a.stats:
    rows = list(csv.DictReader(open(a.stats)))
    out = {}
    for r in rows:
      if "mc_" in r["Name"] or "box_filter" in r["Name"]:
        out[r["Name"].split("(")[0]] = {"calls": int(r["Calls"]), "avg_ms": float(r["AverageNs"]) / 1e6,
                                        "min_ms": float(r["MinNs"]) / 1e6, "max_ms": float(r["MaxNs"]) / 1e6}
    print(json.dumps(out, indent=1))
    return
  from corenet_amd.visualization import marching_cubes
  res = {}
  for name, n, size in WORKLOADS:
    g = fields(n, size, seed=7)
    for _ in range(2):
      m = marching_cubes(g)
    t.cuda.synchronize()
    ts = []
    for _ in range(a.iters):
      e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
      e0.record()
      m = marching_cubes(g)
      e1.record()
      t.cuda.synchronize()
      ts.append(e0.elapsed_time(e1))
    res[name] = {"objects": n, "size": size, "ms_per_call_median": float(np.median(ts)), "ms_min": min(ts),
                 "ms_max": max(ts), "active_cell_fraction": active_fraction(g),
                 "vertices": int(m.num_vertices.sum()), "faces": int(m.num_faces.sum()),
                 "count_pass_bytes": 4 * g.numel()}
    print(json.dumps({name: res[name]}), flush=True)
    del g, m
    t.cuda.empty_cache()
  one = fields(1, 256, seed=7).cpu()
  t.set_num_threads(16)
  marching_cubes(one)
  t0 = time.perf_counter()
  m = marching_cubes(one)
  res["host_twin_1x256_s"] = time.perf_counter() - t0
  print(json.dumps({"host_twin_1x256_s": res["host_twin_1x256_s"], "threads_used": 1,
                    "note": "the host twin runs one object per thread"}), flush=True)


if __name__ == "__main__":
  main()
