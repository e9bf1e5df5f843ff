"""Shared by test_eval_cpu.py and test_eval_gpu.py: a numpy restatement of crn_eval_labels' contract
(include/corenet_hip.h) written from the contract alone, the inputs both test files run, and the known answers of the
reference's voxel_metrics_test.py (data: two label grids, their matrix, the counts and the metric values)."""
import itertools

import numpy as np

SHAPES = [(1, 1, 1), (3, 5, 7), (4, 4, 65),       # a single voxel; odd sizes; a ragged W beyond one wave
          (3, 5, 8), (2, 3, 260)]                 # W a multiple of 4: the kernel takes four voxels per lane; 65 lanes per row
MULTIPLIERS = [1, 2, 3]
CLASSES = [1, 2, 5, 14, 17, 32]                   # every template bucket (2, 4, 8, 16, 32) and its edge
BATCHES = [1, 3]
SENTINEL = -77                                    # what untouched label voxels hold


def bins_of(C):
  return [C, 7, 64]


def eval_labels_ref(scores, gt, scene_class, K, m, n, labels, cm, bad):
  """scores f32 [B, C, D, H, W], gt int32 [B, mD, mH, mW] or None, scene_class int32 [B] or None; writes labels (or
  None) and adds to cm int64 [K, K] / bad int32 [1] in place."""
  B, C = scores.shape[:2]
  ix, iy, iz = n % m, (n // m) % m, n // (m * m)
  best = scores[:, 0].copy()
  pred = np.zeros(best.shape, dtype=np.int64)
  with np.errstate(invalid="ignore"):
    for c in range(1, C):
      take = scores[:, c] > best                  # strict: the first maximum stays; False for any NaN
      best = np.where(take, scores[:, c], best)
      pred[take] = c
  sc = np.ones(B, dtype=np.int64) if scene_class is None else scene_class.astype(np.int64)
  pred = pred * sc[:, None, None, None]
  if labels is not None:
    labels[:, iz::m, iy::m, ix::m] = pred.astype(np.int32)
  if gt is not None:
    g = gt[:, iz::m, iy::m, ix::m].astype(np.int64) * sc[:, None, None, None]
    ok = (g >= 0) & (g < K) & (pred >= 0) & (pred < K)
    cm += np.bincount((g[ok] * K + pred[ok]).ravel(), minlength=K * K).reshape(K, K)
    bad[0] += np.int32((~ok).sum())


def make_case(shape, m, C, K, B, scene, seed):
  """(scores, gt, scene_class): scores are multiples of 1/8 in [-1, 1] (17 values: exact ties are frequent, and any two
  unequal scores differ by at least 0.125), with a NaN at class 0 of the first voxel and at the last class of the last;
  gt and the scene classes are drawn so that labels and products land inside, at and beyond K."""
  D, H, W = shape
  r = np.random.RandomState(seed)
  scores = (r.randint(-8, 9, size=(B, C, D, H, W)) / 8.0).astype(np.float32)
  flat = scores.reshape(B, C, -1)
  flat[0, 0, 0] = np.nan
  flat[B - 1, C - 1, -1] = np.nan
  fine = (B, m * D, m * H, m * W)
  if scene:
    scene_class = r.randint(0, max(2, K // 2 + 2), size=B).astype(np.int32)
    scene_class[0] = K if C > 1 else 1            # pred 1 of scene 0 lands exactly at K: rejected
    gt = r.randint(0, 3, size=fine).astype(np.int32)
  else:
    scene_class = None
    gt = r.randint(-1, K + 2, size=fine).astype(np.int32)       # -1, K and K + 1 are rejected
  return scores, gt, scene_class


def kernel_cases(shape, m):
  """Every (C, K, B, scene) combination for a shape and a multiplier, with a seed of its own."""
  for i, (C, B, scene) in enumerate(itertools.product(CLASSES, BATCHES, (False, True))):
    for j, K in enumerate(bins_of(C)):
      yield C, K, B, scene, 1000 * i + 10 * j + m


# ---- the reference's voxel_metrics_test.py, as data ----
KNOWN_GT = np.array([[[3, 2, 2, 4], [4, 3, 2, 2], [3, 1, 3, 0]],
                     [[3, 0, 1, 3], [2, 3, 1, 1], [2, 3, 0, 4]]], dtype=np.int32)
KNOWN_PRED = np.array([[[0, 2, 3, 1], [1, 1, 1, 3], [4, 0, 2, 3]],
                       [[1, 0, 1, 4], [2, 4, 4, 0], [4, 2, 4, 2]]], dtype=np.int32)
KNOWN_CM = np.array([[1, 0, 0, 1, 1], [2, 1, 0, 0, 1], [0, 1, 2, 2, 1], [1, 2, 2, 0, 3], [0, 2, 1, 0, 0]])
KNOWN_TFPN = dict(tp=[1, 1, 2, 0, 0], tn=[18, 15, 15, 13, 15], fp=[3, 5, 3, 3, 6], fn=[2, 3, 4, 8, 3])
# voxel_metrics_test.py:75-80 states these for the counts above (rtol 1e-7).  Its zeros stand at the classes with tp == 0,
# where voxel_metrics.py:118-120 (nan_tp_div) gives NaN by definition: test_known_metrics checks the literals where
# tp != 0 and NaN where tp == 0.
KNOWN_METRICS = dict(iou=[0.16666667, 0.11111111, 0.22222222, 0., 0.], precision=[0.25, 0.16666667, 0.4, 0., 0.],
                     recall=[0.33333333, 0.25, 0.33333333, 0., 0.])
