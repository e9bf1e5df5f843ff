#!/usr/bin/env python
"""Streaming evaluation (crn_eval_labels, CoreNet.multi_offset_labels): the kernel against the one it generalises, one x2
evaluation batch against the pmf path, and whether x4 runs.

  python tools/bench_eval_labels.py [--rounds 10] [--out profiles/r10_eval_labels_bench.txt]     # JSON lines

(a) kernel: crn_argmax_confusion and crn_eval_labels at m = 1, K = C, no scene class, on the same logits and labels,
    B = 4, 128^3, C = 2 and C = 14.  Two label distributions: uniform over the classes, and 97 % void with the
    prediction agreeing with the label on 90 % of the voxels (what an evaluation batch looks like: a few bins take
    nearly all the adds).  The two kernels alternate; a round times one window of each between device events, a window
    being as many back-to-back launches as fill 0.3 s (counted once, after warm-up); the spread of a kernel is
    (max - min) / median of its rounds.  Bytes: (C + 2) * 4 per voxel (C scores, one label read, one label written)
    against the 8 TB/s HBM peak of the MI355X.  Then the new kernel alone on one pass of an x2 grid (m = 2, n = 3, 256^3
    ground truth and labels) with the same scores: what the strided label accesses cost.
(b) one x2 evaluation batch, B = 4, h7 (2 logits, fg_bg) and m9 (14 logits, semantic): SuperResolutionInference.__call__
    -> extract_labels -> scatter_add confusion matrix (what the project offered before) against predict_labels with
    ground truth; time per batch after warm-up (windows of 0.3 s again) and torch.cuda.max_memory_allocated above what
    was allocated before.
(c) x4 for h7 at B = 1 through predict_labels (64 decoder passes, 512^3 labels)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch as t

HBM_PEAK = 8.0e12
WINDOW_MS = 300.0                 # a timing window lasts at least this long


def window(fn, launches):
  e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(launches):
    fn()
  e1.record()
  t.cuda.synchronize()
  return e0.elapsed_time(e1) / launches


def launches_for(fn):
  """How many back-to-back calls of fn fill a window (fn is warm)."""
  return max(1, math.ceil(WINDOW_MS / window(fn, 5)))


def stats(ts, launches):
  med = float(np.median(ts))
  return {"ms_median": med, "ms_min": min(ts), "ms_max": max(ts), "spread": (max(ts) - min(ts)) / med,
          "launches_per_window": launches}


def kernel_comparison(rounds, emit):
  from corenet_amd import voxel_metrics as VM
  from corenet_amd.backend import default_backend
  be = default_backend()
  B, D = 4, 128
  S = D ** 3
  for C in (2, 14):
    g = t.Generator(device="cuda").manual_seed(C)
    for dist in ("uniform", "mostly_void"):
      if dist == "uniform":
        gt = t.randint(0, C, (B, D, D, D), device="cuda", generator=g, dtype=t.int32)
        logits = t.randn((B, C, D, D, D), device="cuda", generator=g)
      else:
        fg = t.rand((B, D, D, D), device="cuda", generator=g) < 0.03
        gt = t.where(fg, t.randint(1, C, (B, D, D, D), device="cuda", generator=g, dtype=t.int32), t.zeros((), dtype=t.int32, device="cuda"))
        logits = t.randn((B, C, D, D, D), device="cuda", generator=g)
        agree = t.rand((B, D, D, D), device="cuda", generator=g) < 0.9
        logits.scatter_add_(1, gt.long()[:, None], 8.0 * agree[:, None].float())
      labels_old = t.empty((B, D, D, D), dtype=t.int32, device="cuda")
      labels_new = t.empty_like(labels_old)
      cm_old = t.zeros((C, C), dtype=t.int64, device="cuda")
      cm_new, bad = t.zeros_like(cm_old), t.zeros(1, dtype=t.int32, device="cuda")
      old = lambda: be.argmax_confusion(logits, gt, B, C, S, labels_old, cm_old)
      new = lambda: be.eval_labels(logits, gt, None, B, C, C, D, D, D, 1, 0, labels_new, cm_new, bad)
      old(); new()
      t.cuda.synchronize()
      same = bool(t.equal(labels_old, labels_new)) and bool(t.equal(cm_old, cm_new)) and int(bad) == 0
      for _ in range(2):
        window(old, 20); window(new, 20)
      n_old, n_new = launches_for(old), launches_for(new)
      t_old, t_new = [], []
      for _ in range(rounds):
        t_old.append(window(old, n_old))
        t_new.append(window(new, n_new))
      so, sn = stats(t_old, n_old), stats(t_new, n_new)
      bytes_moved = B * S * (C + 2) * 4
      emit({"kernel_b4_128^3": {"C": C, "labels": dist, "same_result": same, "bins_hit": int((cm_new > 0).sum()),
                                 "argmax_confusion": so, "eval_labels_m1": sn, "new_over_old": sn["ms_median"] / so["ms_median"],
                                 "bytes": bytes_moved, "eval_labels_share_of_hbm_peak": bytes_moved / (sn["ms_median"] * 1e-3) / HBM_PEAK,
                                 "argmax_confusion_share_of_hbm_peak": bytes_moved / (so["ms_median"] * 1e-3) / HBM_PEAK}})
      del gt, labels_old, labels_new
      if dist == "mostly_void":
        x2_pass(be, logits, C, rounds, emit)
      del logits


def x2_pass(be, logits, C, rounds, emit):
  """Pass n = 3 (ix = 1, iy = 1, iz = 0) of an x2 evaluation of these scores: gt reads and label writes have stride 2."""
  B, D = logits.shape[0], logits.shape[2]
  g = t.Generator(device="cuda").manual_seed(100 + C)
  fine = (B, 2 * D, 2 * D, 2 * D)
  fg = t.rand(fine, device="cuda", generator=g) < 0.03
  gt = t.where(fg, t.randint(1, C, fine, device="cuda", generator=g, dtype=t.int32), t.zeros((), dtype=t.int32, device="cuda"))
  del fg
  labels = t.empty(fine, dtype=t.int32, device="cuda")
  cm, bad = t.zeros((C, C), dtype=t.int64, device="cuda"), t.zeros(1, dtype=t.int32, device="cuda")
  fn = lambda: be.eval_labels(logits, gt, None, B, C, C, D, D, D, 2, 3, labels, cm, bad)
  window(fn, 20); window(fn, 20)
  n = launches_for(fn)
  st = stats([window(fn, n) for _ in range(rounds)], n)
  bytes_moved = B * D ** 3 * (C + 2) * 4
  emit({"kernel_b4_128^3_x2_pass": {"C": C, "labels": "mostly_void", "m": 2, "n": 3, "eval_labels": st, "bytes_needed": bytes_moved,
                                    "bytes_of_touched_lines": B * D ** 3 * (C + 4) * 4,
                                    "needed_share_of_hbm_peak": bytes_moved / (st["ms_median"] * 1e-3) / HBM_PEAK}})


def scatter_add_cm(pred, gt, K):
  index = (gt.to(t.int64) * K + pred.to(t.int64)).reshape(-1)
  return t.zeros(K * K, dtype=t.int64, device=pred.device).scatter_add(0, index, t.ones_like(index)).reshape(K, K)


def model_and_batch(nc, B):
  import bench
  from corenet_amd.model.core_net import CoreNet, CoreNetConfig, DecoderConfig
  model = CoreNet(CoreNetConfig(DecoderConfig((128, 128, 128), nc, 2, 64, 0.75)), device="cuda", decoder_math="bf16x3").eval()
  image, v2s, off, _ = [x.cuda() for x in bench.synthetic_batch(B, 0, nc)]
  return model, image


def evaluation_batch(rounds, emit):
  import types
  from corenet_amd import evaluation_results as ER, super_resolution as SR
  from corenet_amd.geometry import transformations
  B, res = 4, (256, 256, 256)
  for name, nc, task, K in (("h7_fg_bg", 2, "fg_bg", 14), ("m9_semantic", 14, "semantic", 14)):
    model, image = model_and_batch(nc, B)
    sr = SR.super_resolution_from_state(types.SimpleNamespace(model=model))
    camera = camera_of_bench().cuda().expand(B, 4, 4).contiguous()
    v2x = transformations.scale([256.0] * 3).cuda()[None].expand(B, 4, 4).contiguous()
    go = t.full((B, 3), 0.5, device="cuda")
    g = t.Generator(device="cuda").manual_seed(3)
    gt = (t.rand((B,) + res, device="cuda", generator=g) < 0.03).to(t.int32)
    mesh_labels = [[1 + b % (K - 1)] for b in range(B)]
    if task == "semantic":
      gt = gt * t.randint(1, K, (B,) + res, device="cuda", generator=g, dtype=t.int32)
    ex = types.SimpleNamespace(grid=gt, mesh_labels=mesh_labels, scene_id=[str(b) for b in range(B)])
    scene = ER.scene_classes_of(ex).cuda() if task == "fg_bg" else None

    def parent():
      pmf = sr(image, camera, v2x, go, res)
      pred, g2 = ER.extract_labels(pmf, ex, task)
      return scatter_add_cm(pred, g2, K)

    def streaming():
      cm, bad = t.zeros((K, K), dtype=t.int64, device="cuda"), t.zeros(1, dtype=t.int32, device="cuda")
      sr.predict_labels(image, camera, v2x, go, res, gt=gt, num_classes=K, scene_classes=scene, cm=cm, bad=bad)
      return cm
    out = {}
    cms = {}
    for what, fn in (("parent_pmf_path", parent), ("streaming", streaming)):
      with t.no_grad():
        for _ in range(2):
          cms[what] = fn()
        t.cuda.synchronize()
        t.cuda.empty_cache()
        base = t.cuda.memory_allocated()
        t.cuda.reset_peak_memory_stats()
        n = launches_for(fn)
        ts = [window(fn, n) for _ in range(rounds)]
        out[what] = dict(stats(ts, n), peak_bytes_above_resident=t.cuda.max_memory_allocated() - base, resident_bytes=base)
    # two runs of the network differ in the last bits (split-K atomics), so a few near-tied voxels may move
    diff = int((cms["parent_pmf_path"] - cms["streaming"]).abs().sum())
    out["confusion_matrix_l1_difference"] = diff
    out["voxels"] = int(np.prod((B,) + res))
    out["parent_over_streaming_time"] = out["parent_pmf_path"]["ms_median"] / out["streaming"]["ms_median"]
    out["parent_over_streaming_peak"] = out["parent_pmf_path"]["peak_bytes_above_resident"] / max(1, out["streaming"]["peak_bytes_above_resident"])
    emit({"x2_eval_batch_b4_" + name: out})
    del model, sr, gt, ex, cms
    t.cuda.empty_cache()


def camera_of_bench():
  import bench
  image, v2s, off, _ = bench.synthetic_batch(1, 0, 2)
  return v2s[:1] @ t.diag(t.tensor([128.0, 128.0, 128.0, 1.0]))        # v2s = camera @ scale(1 / 128)


def x4(emit):
  import types
  from corenet_amd import super_resolution as SR
  from corenet_amd.geometry import transformations
  model, image = model_and_batch(2, 1)
  sr = SR.super_resolution_from_state(types.SimpleNamespace(model=model))
  camera = camera_of_bench().cuda()
  v2x = transformations.scale([512.0] * 3).cuda()[None]
  go = t.full((1, 3), 0.5, device="cuda")
  res = (512, 512, 512)
  t.cuda.synchronize()
  t.cuda.empty_cache()
  base = t.cuda.memory_allocated()
  t.cuda.reset_peak_memory_stats()
  try:
    with t.no_grad():
      sr.predict_labels(image, camera, v2x, go, res)          # warm-up: plans, packs
      fn = lambda: sr.predict_labels(image, camera, v2x, go, res)
      n = launches_for(fn)
      ms = window(fn, n)
    emit({"x4_h7_b1": {"runs": True, "ms": ms, "launches_per_window": n, "peak_bytes_above_resident": t.cuda.max_memory_allocated() - base,
                       "labels_bytes": 512 ** 3 * 4, "stash_plus_pmf_bytes_of_the_pmf_path": 2 * 64 * 2 * 128 ** 3 * 4}})
  except Exception as e:                                      # recorded, not hidden: the line says it did not run
    emit({"x4_h7_b1": {"runs": False, "error": repr(e)[:300]}})


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=10)
  ap.add_argument("--out", default=None)
  a = ap.parse_args()
  if not t.cuda.is_available():
    raise SystemExit("bench_eval_labels.py needs the GPU")
  lines = ["# tools/bench_eval_labels.py --rounds %d on %s; times in ms per launch or batch, device events" %
           (a.rounds, t.cuda.get_device_name(0))]

  def emit(d):
    lines.append(json.dumps(d))
    print(lines[-1], flush=True)
  kernel_comparison(a.rounds, emit)
  evaluation_batch(a.rounds, emit)
  x4(emit)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
