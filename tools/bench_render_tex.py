#!/usr/bin/env python
"""Cost of diffuse textures in the batched renderer (corenet_amd.visualization.render.render_batch) on one synthetic
batch: 8 bumpy spheres of 12,800 triangles each (102,400 triangles in shared buffers, per-vertex normals, longitude /
latitude texture coordinates repeated 4 x 2 times, one material per sphere), 80 images of 384^2 = 8 spheres x 10
cameras, each image drawing one sphere that fills most of it.

  python tools/bench_render_tex.py [--iters 20] [--warmup 3] [--variants untextured,tex128,tex1024]

Variants: untextured (no texture arguments: the untextured kernel), tex128 and tex1024 (every material textured from
an 8-layer array of random bytes, 128^2 or 1024^2 texels per layer).  Each timed iteration is one render_batch call with
a device synchronise before and after; the variants alternate inside every iteration, so drift hits them alike.  Prints
one JSON line: per variant the median, minimum and maximum in ms."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch as t

OBJECTS, CAMERAS, LON, LAT, SIZE = 8, 10, 160, 40, (384, 384)


def sphere(seed):
  """-> triangles [2 LON LAT, 3, 3], normals, tex_coords [.., 3, 2] of a sphere whose radius varies by +-10 %."""
  rng = np.random.RandomState(seed)
  lon = np.linspace(0, 2 * math.pi, LON + 1)
  lat = np.linspace(-0.5 * math.pi, 0.5 * math.pi, LAT + 1)
  LO, LA = np.meshgrid(lon, lat, indexing="ij")
  k = rng.randint(2, 6, 2)
  r = 0.5 * (1 + 0.1 * np.sin(k[0] * LO) * np.cos(k[1] * LA))
  P = np.stack([r * np.cos(LA) * np.cos(LO), r * np.sin(LA), r * np.cos(LA) * np.sin(LO)], -1)
  N = P / np.linalg.norm(P, axis=-1, keepdims=True)
  UV = np.stack([LO / (2 * math.pi) * 4, (LA / math.pi + 0.5) * 2], -1)
  i, j = np.meshgrid(np.arange(LON), np.arange(LAT), indexing="ij")
  corners = [(i, j), (i + 1, j), (i + 1, j + 1), (i, j), (i + 1, j + 1), (i, j + 1)]
  pick = lambda A: np.stack([A[a, b] for a, b in corners], 2).reshape(-1, 3, A.shape[-1]).astype(np.float32)
  return pick(P), pick(N), pick(UV)


def scene():
  from corenet_amd.geometry import transformations as T
  from corenet_amd.visualization import camera_util as C
  from corenet_amd.visualization import render as R
  parts = [sphere(s) for s in range(OBJECTS)]
  n = parts[0][0].shape[0]
  tri, nrm, uv = (t.from_numpy(np.concatenate([p[q] for p in parts])).cuda() for q in range(3))
  mids = t.arange(OBJECTS, dtype=t.int32).repeat_interleave(n).cuda()
  mats = R.make_materials(t.from_numpy(np.random.RandomState(100).rand(OBJECTS, 3).astype(np.float32) * 0.5 + 0.5)).cuda()
  proj = C.perspective_projection(1.0, znear=0.1, zfar=10)
  ranges, vps = [], []
  for o in range(OBJECTS):
    for c in range(CAMERAS):
      a = 2 * math.pi * c / CAMERAS
      eye = (1.1 * math.cos(a), 0.5 * math.sin(3 * a), 1.1 * math.sin(a))
      ranges.append([o * n, (o + 1) * n])
      vps.append(t.matmul(proj, T.look_at_lh(eye, (0, 0, 0), (0, 1, 0))))
  return tri, nrm, uv, mids, mats, ranges, t.stack(vps)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--variants", default="untextured,tex128,tex1024")
  a = ap.parse_args()
  if a.iters < 10:
    ap.error("--iters must be at least 10")
  from corenet_amd.visualization import render as R
  if not t.cuda.is_available():
    sys.exit("bench_render_tex: needs a GPU")
  tri, nrm, uv, mids, mats, ranges, vps = scene()
  calls = {}
  for v in a.variants.split(","):
    kw = {}
    if v != "untextured":
      side = {"tex128": 128, "tex1024": 1024}[v]
      g = t.Generator().manual_seed(side)
      kw = dict(tex_coords=uv, textures=t.randint(0, 256, (OBJECTS, side, side, 3), generator=g, dtype=t.uint8).cuda(),
                texture_indices=t.arange(OBJECTS))
    calls[v] = (lambda kw: lambda: R.render_batch(tri, mids, mats, ranges, vps, SIZE, normals=nrm, **kw))(kw)
  covered = None
  for v, fn in calls.items():
    for _ in range(a.warmup):
      img = fn()
    t.cuda.synchronize()
    covered = float(img.any(-1).float().mean())
  ms = {v: [] for v in calls}
  for _ in range(a.iters):
    for v, fn in calls.items():
      t.cuda.synchronize()
      t0 = time.perf_counter()
      fn()
      t.cuda.synchronize()
      ms[v].append((time.perf_counter() - t0) * 1e3)
  res = {"images": len(ranges), "image": list(SIZE), "triangles": int(tri.shape[0]),
         "drawn_per_batch": int(sum(r[1] - r[0] for r in ranges)), "covered_fraction": round(covered, 3),
         "iters": a.iters, "warmup": a.warmup}
  for v, x in ms.items():
    x = sorted(x)
    res[v] = {"median_ms": round(x[len(x) // 2], 4), "min_ms": round(x[0], 4), "max_ms": round(x[-1], 4)}
  print(json.dumps(res), flush=True)


if __name__ == "__main__":
  main()
