#!/usr/bin/env python
"""Score-level evaluation (crn_eval_scores, corenet_amd.score_metrics.score_histogram): the kernel against the HBM copy
rate of the bytes it must read, and against the torch formulation of the same table.

  python tools/bench_eval_scores.py [--rounds 7] [--out profiles/r17_eval_scores_bench.txt]     # JSON lines

(a) kernel, from logits, nbins = 20, B = 4, 128^3, C = 2 and C = 14, K = C, two inputs each: `mostly_void` (97 % void,
    the logits agreeing with the label on 90 % of the voxels by a margin of 8: nearly every entry of a row falls on two
    keys, the contended case) and `spread` (standard normal logits, uniform labels: the keys change from voxel to voxel).
    Three things alternate, a round timing one window of each between device events, a window being as many
    back-to-back launches as fill 0.3 s (counted once, after warm-up):
      eval_scores   the kernel; bytes it must read: (C + 1) * 4 per voxel (C logits and the label)
      copy          a device-to-device copy of a buffer of half those bytes (it reads them and writes them: the same
                    traffic); its rate is the HBM copy rate, and bytes / rate the floor for the kernel
      torch         softmax, then per class bucketize + bincount (count, sum of scores, squared error), the alternative
    spread of a series: (max - min) / median of its rounds.
(b) the kernel alone on pass n = 3 of an x2 grid (m = 2, 256^3 labels) with the mostly-void logits: what the strided
    label reads cost."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch as t

WINDOW_MS = 300.0                 # a timing window lasts at least this long
NBINS = 20


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
  return max(1, math.ceil(WINDOW_MS / window(fn, 3)))


def stats(ts, launches):
  med = float(np.median(ts))
  return {"ms_median": med, "ms_min": min(ts), "ms_max": max(ts), "spread": (max(ts) - min(ts)) / med,
          "launches_per_window": launches}


def torch_table(logits, gt, nbins):
  """The same quantities in torch: per class the (bin, y) counts, the sums of the scores and the squared error."""
  p = logits.softmax(1)
  edges = t.arange(1, nbins, device=p.device, dtype=p.dtype) / nbins
  out = []
  for c in range(p.shape[1] + 1):
    pc = (p[:, c] if c < p.shape[1] else 1 - p[:, 0]).reshape(-1)
    y = ((gt == c) if c < p.shape[1] else (gt != 0)).reshape(-1).long()
    key = t.bucketize(pc, edges, right=True) * 2 + y
    out.append((t.bincount(key, minlength=2 * nbins), t.bincount(key, weights=pc.double(), minlength=2 * nbins),
                t.bincount(y, weights=((pc - y) ** 2).double(), minlength=2)))
  return out


def inputs(C, dist, B, D, g):
  shape = (B, D, D, D)
  if dist == "spread":
    return t.randn((B, C, D, D, D), device="cuda", generator=g), t.randint(0, C, shape, device="cuda", generator=g, dtype=t.int32)
  fg = t.rand(shape, device="cuda", generator=g) < 0.03
  gt = t.where(fg, t.randint(1, C, shape, device="cuda", generator=g, dtype=t.int32), t.zeros((), dtype=t.int32, device="cuda"))
  logits = t.randn((B, C, D, D, D), device="cuda", generator=g)
  agree = t.rand(shape, device="cuda", generator=g) < 0.9
  logits.scatter_add_(1, gt.long()[:, None], 8.0 * agree[:, None].float())
  return logits, gt


def kernel_comparison(rounds, emit, with_torch=True):
  from corenet_amd import score_metrics as SM
  from corenet_amd.backend import default_backend
  be = default_backend()
  B, D = 4, 128
  S = D ** 3
  for C in (2, 14):
    g = t.Generator(device="cuda").manual_seed(C)
    medians = {}
    for dist in ("mostly_void", "spread"):
      logits, gt = inputs(C, dist, B, D, g)
      h = SM.empty_histogram(C, NBINS, "cuda")
      bytes_read = B * S * (C + 1) * 4
      src = t.empty(bytes_read // 2, dtype=t.uint8, device="cuda").random_(generator=g)
      dst = t.empty_like(src)
      kern = lambda: be.eval_scores(logits, True, gt, None, B, C, C, D, D, D, 1, 0, NBINS, h.table, h.sq, h.bad)
      copy = lambda: dst.copy_(src)
      alt = lambda: torch_table(logits, gt, NBINS)
      kern()
      t.cuda.synchronize()
      ok = int(h.table[..., 0].sum()) == (C + 1) * B * S and int(h.bad) == 0
      keys_hit = int((h.table[..., 0] > 0).sum())
      top2_share = float(h.table[..., 0].reshape(C + 1, -1).topk(2, dim=1).values.sum() / h.table[..., 0].sum())
      # the torch formulation agrees up to the bits of its softmax: compare the totals per row
      ref = torch_table(logits, gt, NBINS)
      rows_agree = all(int(ref[c][0].sum()) == int(h.table[c, :, :, 0].sum()) for c in range(C + 1))
      del ref
      for _ in range(2):
        window(kern, 20); window(copy, 20)
        if with_torch:
          window(alt, 1)
      n_k, n_c, n_a = launches_for(kern), launches_for(copy), launches_for(alt) if with_torch else 0
      t_k, t_c, t_a = [], [], []
      for _ in range(rounds):
        t_k.append(window(kern, n_k))
        t_c.append(window(copy, n_c))
        t_a.append(window(alt, n_a) if with_torch else float("nan"))
      sk, sc, sa = stats(t_k, n_k), stats(t_c, n_c), stats(t_a, n_a)
      copy_rate = bytes_read / (sc["ms_median"] * 1e-3)                       # the copy reads half and writes half
      medians[dist] = sk["ms_median"]
      emit({"kernel_b4_128^3": {"C": C, "nbins": NBINS, "input": dist, "counts_complete": ok, "row_totals_agree_with_torch": rows_agree,
                                 "keys_hit": keys_hit, "share_of_entries_on_the_top_two_keys_of_a_row": top2_share,
                                 "eval_scores": sk, "copy": sc, "torch": sa, "bytes_read": bytes_read, "hbm_copy_rate_bytes_per_s": copy_rate,
                                 "kernel_over_copy_floor": sk["ms_median"] / sc["ms_median"],
                                 "torch_over_kernel": sa["ms_median"] / sk["ms_median"]}})
      del src, dst, gt
      if dist == "mostly_void":
        x2_pass(be, SM, logits, C, rounds, emit)
      del logits
    emit({"contended_over_spread_b4_128^3": {"C": C, "ratio": medians["mostly_void"] / medians["spread"]}})


def x2_pass(be, SM, logits, C, rounds, emit):
  """Pass n = 3 (ix = 1, iy = 1, iz = 0) of an x2 evaluation of these logits: the label reads have stride 2."""
  B, D = logits.shape[0], logits.shape[2]
  g = t.Generator(device="cuda").manual_seed(100 + C)
  fine = (B, 2 * D, 2 * D, 2 * D)
  fg = t.rand(fine, device="cuda", generator=g) < 0.03
  gt = t.where(fg, t.randint(1, C, fine, device="cuda", generator=g, dtype=t.int32), t.zeros((), dtype=t.int32, device="cuda"))
  del fg
  h = SM.empty_histogram(C, NBINS, "cuda")
  fn = lambda: be.eval_scores(logits, True, gt, None, B, C, C, D, D, D, 2, 3, NBINS, h.table, h.sq, h.bad)
  window(fn, 20); window(fn, 20)
  n = launches_for(fn)
  st = stats([window(fn, n) for _ in range(rounds)], n)
  emit({"kernel_b4_128^3_x2_pass": {"C": C, "input": "mostly_void", "m": 2, "n": 3, "labels": "256^3", "eval_scores": st,
                                    "bytes_needed": B * D ** 3 * (C + 1) * 4, "bytes_of_touched_lines": B * D ** 3 * (C + 2) * 4}})


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=7)
  ap.add_argument("--out", default=None)
  ap.add_argument("--skip-torch", action="store_true", help="leave the torch formulation out (it takes seconds per call)")
  a = ap.parse_args()
  if not t.cuda.is_available():
    raise SystemExit("bench_eval_scores.py needs the GPU")
  lines = ["# tools/bench_eval_scores.py --rounds %d on %s; times in ms per launch, device events" %
           (a.rounds, t.cuda.get_device_name(0))]

  def emit(d):
    lines.append(json.dumps(d))
    print(lines[-1], flush=True)
  kernel_comparison(a.rounds, emit, with_torch=not a.skip_torch)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
