#!/usr/bin/env python
"""Surface metrics (corenet_amd.mesh_metrics): the brute-force nearest-neighbour kernel, the whole
surface_metrics_for_batch on the fixture scenes, and the obvious PyTorch baseline on the same inputs.

  python tools/bench_point_metrics.py [--iters 10]      # device-event times, JSON lines
  rocprofv3 --kernel-trace --stats -d DIR -o pm -- python tools/bench_point_metrics.py --iters 5     # per-kernel times

Workloads of `nearest`: 4 objects x 16384 queries x 16384 candidates (h7 eval batch) and 52 x 16384 x 16384 (m7 x2 at
B = 4), points uniform in the unit cube.  The pair rate counts 8 flops per (query, candidate) pair (3 subtractions, 3
products, 2 sums; the compare and the two selects that keep (d2, index) are not counted) against the 157.3 TFLOP/s fp32
vector peak, which is an FMA rate: without contraction, as the contract demands, half of it is the ceiling.
Baseline: torch.cdist(a_n, b_n).min(1) per object, queries in chunks of 4096 (a 4096 x 16384 float32 matrix each)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch as t

WORKLOADS = [("h7_eval_4x16384", 4, 16384), ("m7_x2_52x16384", 52, 16384)]
FP32_VECTOR_PEAK = 157.3e12


def timed(fn, iters):
  for _ in range(2):
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


def cdist_baseline(a, b, n, s, chunk=4096):
  d, i = [], []
  for k in range(n):
    bn = b[k * s:(k + 1) * s]
    for c in range(0, s, chunk):
      m = t.cdist(a[k * s + c:k * s + c + chunk], bn).min(1)
      d.append(m.values)
      i.append(m.indices)
  return t.cat(d), t.cat(i)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=10)
  a = ap.parse_args()
  from corenet_amd import evaluation_results as ER, mesh_metrics as MM, pipeline
  from corenet_amd.data import batched_example as B, dataset as D
  for name, n, s in WORKLOADS:
    g = t.Generator(device="cuda").manual_seed(1)
    pa = t.rand((n * s, 3), device="cuda", generator=g)
    pb = t.rand((n * s, 3), device="cuda", generator=g)
    off = t.arange(n + 1, dtype=t.int64) * s
    med, lo, hi, (d2, idx) = timed(lambda: MM.nearest_distances(pa, off, pb, off), a.iters)
    bmed, blo, bhi, (bd, bi) = timed(lambda: cdist_baseline(pa, pb, n, s), max(2, a.iters // 2))
    pairs = n * s * s
    res = {"objects": n, "points_per_side": s, "pairs": pairs, "nearest_ms_median": med, "nearest_ms_min": lo,
           "nearest_ms_max": hi, "pairs_per_s": pairs / (med * 1e-3), "tflops_at_8_per_pair": 8 * pairs / (med * 1e-3) / 1e12,
           "share_of_fp32_vector_peak": 8 * pairs / (med * 1e-3) / FP32_VECTOR_PEAK, "cdist_min_ms_median": bmed,
           "cdist_min_ms_min": blo, "cdist_min_ms_max": bhi, "baseline_over_kernel": bmed / med,
           "index_agreement_with_cdist": float((idx.long() == bi).float().mean()),
           "max_abs_dist_difference": float((d2.sqrt() - bd).abs().max())}
    print(json.dumps({name: res}), flush=True)
    del pa, pb, d2, idx, bd, bi
    t.cuda.empty_cache()
  # end to end on the two fixture scenes, semantic, 128^3, pmf near the ground truth
  root = os.path.join(ROOT, "tests", "golden", "n2_dataset")
  ds = D.CoReNetDatasetImpl(os.path.join(root, "dataset.json"), os.path.join(root, "meshes"))
  ex = pipeline.voxelize_batch(B.batch([ds[0], ds[1]]), "semantic")
  nc = 4
  noise = t.randn((2, nc) + tuple(ex.grid.shape[1:]), generator=t.Generator().manual_seed(7)) * 0.3
  onehot = t.nn.functional.one_hot(ex.grid.to(t.int64).clamp(0, nc - 1), nc).permute(0, 4, 1, 2, 3).float()
  pmf = (noise.cuda() + 2 * onehot).softmax(1)
  for src in ("mesh", "grid"):
    med, lo, hi, rows = timed(lambda: ER.surface_metrics_for_batch(pmf, ex, "semantic", gt_source=src), a.iters)
    print(json.dumps({"surface_metrics_for_batch_fixture_2x3x128_" + src: {
        "ms_median": med, "ms_min": lo, "ms_max": hi, "num_samples": 16384,
        "chamfer_l1": rows.metrics.chamfer_l1.tolist(), "fscore_at_0.01": rows.metrics.fscore[:, 0].tolist()}}), flush=True)


if __name__ == "__main__":
  main()
