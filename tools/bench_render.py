#!/usr/bin/env python
"""Rendering of one h7 eval batch's qualitative panels (corenet_amd.evaluation_results.visualize_output): B = 4 scenes
of the fixture dataset (2 and 3 objects, semantic task, 4 classes) voxelized at 128^3, a pmf near the ground truth
(softmax of 2 * one-hot + 0.3 * noise), 384^2
images, five cameras x four 3D panels (marching cubes, ground-truth meshes, predicted and ground-truth label grids).

  python tools/bench_render.py [--iters 10] [--warmup 3] [--png DIR]   # ms per pass and in total (device sync around each)
  rocprofv3 --kernel-trace --stats -d DIR -o render -- python tools/bench_render.py --iters 5     # per-kernel times

Passes timed on their own: marching cubes of the 4 x 3 predicted class grids, voxel faces of the 8 label grids, the batched
render of the 80 panel images from the concatenated buffers; then visualize_output end to end (which adds the
boxes, the host-side cameras, the input-image resize and the row assembly).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch as t

NC = 4      # classes of the fixture dataset, void included


def batch(B):
  from corenet_amd import pipeline
  from corenet_amd.data import batched_example as BE, dataset as D
  root = os.path.join(ROOT, "tests", "golden", "n2_dataset")
  ds = D.CoReNetDatasetImpl(os.path.join(root, "dataset.json"), os.path.join(root, "meshes"))
  els = [ds[i % len(ds)] for i in range(B)]
  ex = pipeline.voxelize_batch(BE.batch(els), "semantic")
  g = t.Generator(device="cuda").manual_seed(0)
  noise = t.randn((B, NC) + tuple(ex.grid.shape[1:]), device="cuda", generator=g) * 0.3
  onehot = t.nn.functional.one_hot(ex.grid.to(t.int64).clamp(0, NC - 1), NC).permute(0, 4, 1, 2, 3).float()
  return (noise + 2 * onehot).softmax(1), ex


def render_inputs(pmf, ex, grids):
  """The buffers visualize_output builds for its one render call: per scene 4 triangle ranges x 5 cameras ->
  (triangles, normals, material_ids, materials, ranges, view_projections, normal_modes, triangle counts)."""
  from corenet_amd.visualization import camera_util as C
  from corenet_amd.visualization import render as R
  from corenet_amd.visualization.colors import DEFAULT_COLOR_PALETTE
  from corenet_amd.visualization.marching_cubes import to_marching_cubes
  B = pmf.shape[0]
  pal = t.as_tensor(DEFAULT_COLOR_PALETTE)
  v2x_inv = ex.v2x_transform[0].cpu().inverse()
  objs = pmf[:, 1:].reshape((B * (NC - 1),) + tuple(pmf.shape[2:]))
  mc_tri, mc_nrm, mc_cnt = to_marching_cubes(objs)
  faces = R.voxel_faces(grids, pal, v2x_inv)
  T_mc, T_gt = mc_tri.shape[0], ex.vertices.shape[0]
  tri = t.cat([mc_tri * (1 / 128.0), ex.vertices, faces.triangles], 0)
  nrm = t.cat([mc_nrm, t.zeros_like(ex.vertices), faces.normals], 0)
  mats = t.cat([R.voxel_materials(pal), R.make_materials(pal[1:2])], 0)
  mid = t.cat([t.full((T_mc + T_gt,), pal.shape[0], dtype=t.int32, device="cuda"), faces.material_ids], 0)
  mc_cnt, gt_cnt, vx_cnt = mc_cnt.cpu().long().reshape(B, NC - 1).sum(1), [int(n.sum()) for n in ex.mesh_num_tri], faces.num_triangles.cpu()
  st = lambda c: (t.cumsum(t.as_tensor(c), 0) - t.as_tensor(c)).tolist()
  mc0, gt0, vx0 = st(mc_cnt), [s + T_mc for s in st(gt_cnt)], [s + T_mc + T_gt for s in st(vx_cnt)]
  ranges, vps, modes = [], [], []
  for b in range(B):
    box = tri[gt0[b]:gt0[b] + gt_cnt[b]].reshape(-1, 3)
    cams = [ex.camera_transform[b].cpu()] + [C.get_default_camera_for_mesh(box.reshape(-1, 3, 3)) for _ in range(4)]
    for cam in cams:
      for r, m in (((mc0[b], mc0[b] + int(mc_cnt[b])), 1), ((gt0[b], gt0[b] + gt_cnt[b]), 0),
                   ((vx0[b], vx0[b] + int(vx_cnt[b])), 2), ((vx0[B + b], vx0[B + b] + int(vx_cnt[B + b])), 2)):
        ranges.append(r)
        vps.append(cam)
        modes.append(m)
  counts = {"marching_cubes": T_mc, "gt_meshes": T_gt, "voxel_faces": int(vx_cnt.sum()),
            "drawn_per_batch": int(sum(r[1] - r[0] for r in ranges))}
  return tri, nrm, mid, mats, ranges, t.stack(vps), modes, counts


def timed(fn, iters, warmup):
  for _ in range(warmup):
    fn()
  t.cuda.synchronize()
  ms = []
  for _ in range(iters):
    t0 = time.perf_counter()
    fn()
    t.cuda.synchronize()
    ms.append((time.perf_counter() - t0) * 1e3)
  ms.sort()
  return ms[len(ms) // 2], ms[0]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=10)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--batch", type=int, default=4)
  ap.add_argument("--png", default=None, help="also write QualitativeResults' PNG of the first scene into this directory")
  a = ap.parse_args()
  from corenet_amd import evaluation_results as ER
  from corenet_amd.visualization import camera_util as C
  from corenet_amd.visualization import render as R
  from corenet_amd.visualization.colors import DEFAULT_COLOR_PALETTE
  from corenet_amd.visualization.marching_cubes import marching_cubes, to_marching_cubes
  pmf, ex = batch(a.batch)
  B = a.batch
  pred, gt = ER.extract_labels(pmf, ex, "semantic")
  grids = t.cat([pred, gt.to(t.int32)], 0).contiguous()
  v2x_inv = ex.v2x_transform[0].cpu().inverse()
  pal = t.as_tensor(DEFAULT_COLOR_PALETTE)
  res = {"batch": B, "grid": list(ex.grid.shape[1:]), "image": [384, 384], "images": B * 20}
  objs = pmf[:, 1:].reshape((B * (NC - 1),) + tuple(pmf.shape[2:]))
  res["mc_ms"], _ = timed(lambda: marching_cubes(objs, 0.5, matrices=v2x_inv.cuda()), a.iters, a.warmup)
  res["faces_ms"], _ = timed(lambda: R.voxel_faces(grids, pal, v2x_inv, box_matrices=v2x_inv), a.iters, a.warmup)
  tri, nrm, mid, mats, ranges, vps, modes, res["triangles"] = render_inputs(pmf, ex, grids)
  res["render_ms"], _ = timed(lambda: R.render_batch(tri, mid, mats, ranges, vps, (384, 384), normals=nrm,
                                                     normal_modes=modes), a.iters, a.warmup)
  res["visualize_output_ms"], res["visualize_output_min_ms"] = timed(lambda: ER.visualize_output(pmf, ex, "semantic"),
                                                                     a.iters, a.warmup)
  res["iters"], res["warmup"] = a.iters, a.warmup
  print(json.dumps(res), flush=True)
  if a.png:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import render_scenes
    render_scenes.write_qualitative(pmf, ex, a.png)


if __name__ == "__main__":
  main()
