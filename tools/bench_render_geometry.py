#!/usr/bin/env python
"""The geometry raster (render.render_geometry, crn_render_raster_geometry) beside the colour raster on the workload of
tools/bench_render.py: B = 4 fixture scenes voxelized at 128^3, 384^2 images, the 80 panel images of visualize_output;
then the image-space metric built on it (evaluation_results.reprojection_metrics_for_batch) end to end on the same batch.

  python tools/bench_render_geometry.py [--iters 20] [--warmup 3]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o geom -- \
      python tools/bench_render_geometry.py --only-raster               # per-kernel times of the 80-image workload

Both rasters are timed through the C ABI with device events on buffers binned once: one sample is crn_render_bin followed
by the raster call (fill + raster kernel), so the two differ in the raster kernel alone; crn_render_bin alone is timed
too.  Every figure is the median over --iters samples with the smallest and largest beside it, the run-to-run spread a
difference has to exceed.  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch as t

import bench_render


def event_ms(fn, iters, warmup):
  """[median, min, max] ms of fn's device work over iters samples."""
  for _ in range(warmup):
    fn()
  t.cuda.synchronize()
  ms = []
  for _ in range(iters):
    a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    ms.append(a.elapsed_time(b))
  ms.sort()
  return [round(ms[len(ms) // 2], 4), round(ms[0], 4), round(ms[-1], 4)]


def raster_calls(tri, nrm, mid, mats, ranges, vps, modes, size):
  """(bin, colour, geometry): functions that queue crn_render_bin alone, followed by crn_render_raster, and followed by
  crn_render_raster_geometry with all four outputs, on one set of buffers."""
  import numpy as np
  from corenet_amd import _lib as L
  from corenet_amd.visualization import render as R
  H, W = size
  lib = L.lib()
  rg, cams = R._ranges_and_cameras(ranges, vps, H, W, tri.shape[0])
  I = rg.shape[0]
  rec, num_inst, max_len = R._image_records(rg, cams, False)
  rec.view(np.int32)[:, 32] = np.asarray(modes)
  for i in range(I):
    rec[i, 16:19] = rec[i, 19:22] = R.camera_position(cams[i]).numpy()
  rec[:, 22:25], rec[:, 25:28] = 1.0, 0.2
  images, records, counts, offsets, bins, s = R._bin(lib, tri, t.from_numpy(rec), I, H, W, max_len, num_inst)
  rgb = t.empty((I, H, W, 3), dtype=t.uint8, device="cuda")
  idx = t.empty((I, H, W), dtype=t.int32, device="cuda")
  bary = t.empty((I, H, W, 3), dtype=t.float32, device="cuda")
  depth, z = t.empty((I, H, W), dtype=t.float32, device="cuda"), t.empty((I, H, W), dtype=t.float32, device="cuda")

  def bin_():
    lib.crn_render_bin(tri.data_ptr(), images.data_ptr(), I, H, W, max_len, num_inst, records.data_ptr(),
                       counts.data_ptr(), offsets.data_ptr(), s)

  def colour():
    bin_()
    lib.crn_render_raster(tri.data_ptr(), nrm.data_ptr(), mid.data_ptr(), mats.data_ptr(), mats.shape[0],
                          images.data_ptr(), I, H, W, max_len, records.data_ptr(), counts.data_ptr(), offsets.data_ptr(),
                          bins.data_ptr(), rgb.data_ptr(), s)

  def geometry():
    bin_()
    lib.crn_render_raster_geometry(tri.data_ptr(), images.data_ptr(), I, H, W, max_len, records.data_ptr(),
                                   counts.data_ptr(), offsets.data_ptr(), bins.data_ptr(), idx.data_ptr(), bary.data_ptr(),
                                   depth.data_ptr(), z.data_ptr(), s)
  return bin_, colour, geometry, {"images": I, "list_entries": int(bins.numel())}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=3)
  ap.add_argument("--batch", type=int, default=4)
  ap.add_argument("--only-raster", action="store_true", help="skip the metric: a kernel trace then holds the 80-image "
                  "workload alone")
  a = ap.parse_args()
  from corenet_amd import evaluation_results as ER
  pmf, ex = bench_render.batch(a.batch)
  pred, gt = ER.extract_labels(pmf, ex, "semantic")
  grids = t.cat([pred, gt.to(t.int32)], 0).contiguous()
  tri, nrm, mid, mats, ranges, vps, modes, counts = bench_render.render_inputs(pmf, ex, grids)
  bin_, colour, geometry, sizes = raster_calls(tri, nrm, mid, mats.cuda(), ranges, vps, modes, (384, 384))
  res = {"batch": a.batch, "image": [384, 384], "triangles": counts, **sizes, "format": "[median, min, max] ms"}
  res["bin_ms"] = event_ms(bin_, a.iters, a.warmup)
  res["bin_colour_raster_ms"] = event_ms(colour, a.iters, a.warmup)
  res["bin_geometry_raster_ms"] = event_ms(geometry, a.iters, a.warmup)
  res["geometry_raster_again_ms"] = event_ms(geometry, a.iters, a.warmup)   # the same measurement twice: the spread
  for gt_kind in () if a.only_raster else ("grid", "mesh"):
    def metric():
      ER.reprojection_metrics_for_batch(pmf, ex, "semantic", gt=gt_kind)
      t.cuda.synchronize()
    wall = bench_render.timed(metric, a.iters, a.warmup)
    res[f"reprojection_{gt_kind}_ms"] = {"median": round(wall[0], 3), "min": round(wall[1], 3)}
  res["reprojection_image"] = list(ex.input_image.shape[-2:])
  res["iters"], res["warmup"] = a.iters, a.warmup
  print(json.dumps(res), flush=True)


if __name__ == "__main__":
  main()
