#!/usr/bin/env python
"""Point-to-triangle distances (corenet_amd.mesh_metrics.point_triangle_distances): the brute-force
kernel, surface_metrics_for_batch on the fixture scenes in both distance modes, and a chunked PyTorch implementation of
the same distance on the same inputs.

  python tools/bench_point_triangle.py [--iters 10]      # device-event times, JSON lines

Workloads: 4 objects x 16384 queries x 65536 triangles (an eval batch of h7 against marching-cubes surfaces at 128^3) and
52 x 16384 x 65536, queries uniform in the unit cube, triangles with edges up to about 0.1 anywhere in it.
Baseline: the closest-point region walk written with torch.where on a [queries, triangles] grid, 2048 x 4096 pairs a
chunk, minimum and argmin per chunk; the same number of timed runs as the kernel, after one warm-up.  On the large
workload the baseline is timed on 4 of the 52 objects and scaled."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch as t

WORKLOADS = [("h7_eval_4x16384x65536", 4, 16384, 65536), ("m7_x2_52x16384x65536", 52, 16384, 65536)]


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


def torch_point_triangle(p, tri):
  """(d2 [Q], index [Q]) of p [Q, 3] against tri [T, 3, 3]: Ericson's region walk with torch.where."""
  a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
  ab, ac = b - a, c - a
  p = p[:, None, :]
  ap, bp, cp = p - a, p - b, p - c
  d1, d2, d3, d4, d5, d6 = ((ab * ap).sum(-1), (ac * ap).sum(-1), (ab * bp).sum(-1), (ac * bp).sum(-1), (ab * cp).sum(-1),
                            (ac * cp).sum(-1))
  vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
  den = va + vb + vc
  q = a + ab * (vb / den)[..., None] + ac * (vc / den)[..., None]
  w = ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None]
  q = t.where(((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0))[..., None], b + (c - b) * w, q)
  q = t.where(((vb <= 0) & (d2 >= 0) & (d6 <= 0))[..., None], a + ac * (d2 / (d2 - d6))[..., None], q)
  q = t.where(((d6 >= 0) & (d5 <= d6))[..., None], c, q)
  q = t.where(((vc <= 0) & (d1 >= 0) & (d3 <= 0))[..., None], a + ab * (d1 / (d1 - d3))[..., None], q)
  q = t.where(((d3 >= 0) & (d4 <= d3))[..., None], b, q)
  q = t.where(((d1 <= 0) & (d2 <= 0))[..., None], a, q)
  return ((p - q) ** 2).sum(-1).min(1)


def torch_baseline(p, tri, n, s, nt, qc=2048, tc=4096):
  d, i = [], []
  for k in range(n):
    for q0 in range(0, s, qc):
      pq = p[k * s + q0:k * s + q0 + qc]
      best = t.full((pq.shape[0],), float("inf"), device=p.device)
      arg = t.full((pq.shape[0],), -1, dtype=t.int64, device=p.device)
      for t0 in range(0, nt, tc):
        m = torch_point_triangle(pq, tri[k * nt + t0:k * nt + t0 + tc])
        less = m.values < best
        best, arg = t.where(less, m.values, best), t.where(less, m.indices + t0, arg)
      d.append(best)
      i.append(arg)
  return t.cat(d), t.cat(i)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=10)
  a = ap.parse_args()
  from corenet_amd import evaluation_results as ER, mesh_metrics as MM, pipeline
  from corenet_amd.data import batched_example as B, dataset as D
  for name, n, s, nt in WORKLOADS:
    g = t.Generator(device="cuda").manual_seed(1)
    p = t.rand((n * s, 3), device="cuda", generator=g)
    v0 = t.rand((n * nt, 1, 3), device="cuda", generator=g)
    tri = t.cat([v0, v0 + (t.rand((n * nt, 2, 3), device="cuda", generator=g) - 0.5) * 0.1], 1).contiguous()
    p_off, t_off = t.arange(n + 1, dtype=t.int64) * s, t.arange(n + 1, dtype=t.int64) * nt
    med, lo, hi, (d2, idx) = timed(lambda: MM.point_triangle_distances(p, p_off, tri, t_off), a.iters)
    nb = min(n, 4)
    bmed, blo, bhi, (bd, bi) = timed(lambda: torch_baseline(p, tri, nb, s, nt), a.iters, warm=1)
    pairs = n * s * nt
    same = slice(0, nb * s)
    res = {"objects": n, "queries_per_object": s, "triangles_per_object": nt, "pairs": pairs,
           "splits": MM.point_triangle_splits(n, s, nt), "point_triangle_ms_median": med, "point_triangle_ms_min": lo,
           "point_triangle_ms_max": hi, "pairs_per_s": pairs / (med * 1e-3), "torch_objects_timed": nb,
           "torch_ms_median_scaled_to_all_objects": bmed * n / nb, "torch_ms_min_scaled": blo * n / nb,
           "torch_ms_max_scaled": bhi * n / nb, "torch_over_kernel": bmed * n / nb / med,
           "index_agreement_with_torch": float((idx[same].long() == bi).float().mean()),
           "max_abs_dist_difference": float((d2[same].sqrt() - bd.sqrt()).abs().max())}
    print(json.dumps({name: res}), flush=True)
    del p, tri, v0, d2, idx, bd, bi
    t.cuda.empty_cache()
  # end to end on the two fixture scenes, semantic, 128^3, pmf near the ground truth (as tools/bench_point_metrics.py)
  root = os.path.join(ROOT, "tests", "golden", "n2_dataset")
  ds = D.CoReNetDatasetImpl(os.path.join(root, "dataset.json"), os.path.join(root, "meshes"))
  ex = pipeline.voxelize_batch(B.batch([ds[0], ds[1]]), "semantic")
  nc = 4
  noise = t.randn((2, nc) + tuple(ex.grid.shape[1:]), generator=t.Generator().manual_seed(7)) * 0.3
  onehot = t.nn.functional.one_hot(ex.grid.to(t.int64).clamp(0, nc - 1), nc).permute(0, 4, 1, 2, 3).float()
  pmf = (noise.cuda() + 2 * onehot).softmax(1)
  for src in ("mesh", "grid"):
    for mode in ("points", "triangles"):
      med, lo, hi, rows = timed(lambda: ER.surface_metrics_for_batch(pmf, ex, "semantic", gt_source=src, distance=mode), a.iters)
      out = {"ms_median": med, "ms_min": lo, "ms_max": hi, "num_samples": 16384, "chamfer_l1": rows.metrics.chamfer_l1.tolist(),
             "fscore_at_0.01": rows.metrics.fscore[:, 0].tolist()}
      if mode == "triangles":
        out["normal_consistency"] = rows.metrics.normal_consistency.tolist()
      print(json.dumps({f"surface_metrics_for_batch_fixture_2x3x128_{src}_{mode}": out}), flush=True)


if __name__ == "__main__":
  main()
