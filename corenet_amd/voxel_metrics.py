"""Eval epilogue: fused argmax + confusion matrix on the GPU
(evaluation_results.py:40-51, voxel_metrics.py:33-58,123-138), and the reference's voxel metrics: true / false
positives / negatives, IoU, precision and recall from a confusion matrix (voxel_metrics.py:24-138).

label_confusion is the streaming form of the epilogue (crn_eval_labels): one native pass of an x m
inference at a time, a K x K matrix over the dataset's classes (fg_bg: K != C), CUDA(HIP) tensors on the kernel and
CPU tensors on the library's host twin, with identical results."""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Tuple

import torch as t

from corenet_amd.backend import default_backend


def argmax_confusion(logits: t.Tensor, gt: t.Tensor, num_classes: int, cm: t.Tensor = None):
  """Returns (pred_labels int32[B,...], confusion_matrix int64[K,K]); cm[gt, pred]."""
  B, C = logits.shape[:2]
  S = logits[0, 0].numel()
  assert C == num_classes
  labels = t.empty((B,) + tuple(logits.shape[2:]), dtype=t.int32, device=logits.device)
  if cm is None:
    cm = t.zeros(num_classes, num_classes, dtype=t.int64, device=logits.device)
  default_backend().argmax_confusion(logits.contiguous(), gt.to(t.int32).contiguous(), B, C, S, labels, cm)
  return labels, cm


def mean_iou(cm: t.Tensor, void_class: int = 0) -> float:
  """voxel_metrics.py:123-138 + evaluation_results.py:262-266 (NaN for absent classes,
  mean over non-void classes skipping NaNs like pandas)."""
  cm = cm.to(t.float64).cpu()
  tp = cm.diag(); fp = cm.sum(0) - tp; fn = cm.sum(1) - tp
  vals = [float(tp[i] / (tp[i] + fp[i] + fn[i])) for i in range(cm.shape[0])
          if i != void_class and tp[i] != 0]
  return sum(vals) / len(vals) if vals else math.nan


@dataclasses.dataclass
class TfpnValues:
  """True / false positives / negatives (voxel_metrics.py:24-30); one value per class, or scalars."""
  tp: t.Tensor
  tn: t.Tensor
  fp: t.Tensor
  fn: t.Tensor


@dataclasses.dataclass
class VoxelMetrics:
  """float64, the shape of the TfpnValues they come from (voxel_metrics.py:110-115)."""
  iou: t.Tensor
  precision: t.Tensor
  recall: t.Tensor


def _assert_label_pair(predicted: t.Tensor, gt: t.Tensor):
  """What the reference asserts of two label tensors: 32- or 64-bit integers, one shape."""
  for name, x in (("predicted", predicted), ("gt", gt)):
    assert x.dtype in (t.int32, t.int64), f"{name}: integer labels (int32 or int64) expected, got {x.dtype}"
  assert predicted.shape == gt.shape, f"predicted {tuple(predicted.shape)} and gt {tuple(gt.shape)} differ in shape"


def confusion_matrix(predicted: t.Tensor, gt: t.Tensor, num_classes: int) -> t.Tensor:
  """int64 [num_classes, num_classes], (gt, predicted), from two label tensors of one shape (voxel_metrics.py:33-58).
  A compatibility function off the hot path (the hot path is label_confusion): one torch bincount."""
  _assert_label_pair(predicted, gt)
  K = int(num_classes)
  pairs = t.stack([gt.flatten().long(), predicted.flatten().long()])          # [2, N]: row 0 the label, row 1 the prediction
  if pairs.shape[1] == 0:
    return t.zeros((K, K), dtype=t.int64, device=gt.device)
  lo, hi = int(pairs.min()), int(pairs.max())
  if lo < 0 or hi >= K:
    raise ValueError(f"confusion_matrix: labels span [{lo}, {hi}], outside [0, {K})")
  return t.bincount(pairs[0] * K + pairs[1], minlength=K * K).view(K, K)


def compute_tfpn(matrix: t.Tensor) -> TfpnValues:
  """Per-class counts from a confusion matrix [K, K], axis 0 the ground truth, axis 1 the prediction
  (voxel_metrics.py:61-97): a class's hits are its diagonal entry, the rest of its column was predicted as it wrongly
  (fp), the rest of its row was labelled it and missed (fn), and everything else is a true negative."""
  assert matrix.dim() == 2 and matrix.shape[0] == matrix.shape[1], f"square matrix expected, got {tuple(matrix.shape)}"
  hits = matrix.diagonal()
  wrongly_predicted = matrix.sum(dim=0) - hits
  missed = matrix.sum(dim=1) - hits
  return TfpnValues(tp=hits, tn=matrix.sum() - (hits + wrongly_predicted + missed), fp=wrongly_predicted, fn=missed)


def compute_tfpn_fg(matrix: t.Tensor) -> TfpnValues:
  """Class-agnostic foreground / background counts (scalars): class 0 against all others (voxel_metrics.py:100-107)."""
  void_row, object_rows = matrix[0], matrix[1:]
  return TfpnValues(tp=object_rows[:, 1:].sum(), tn=void_row[0], fp=void_row[1:].sum(), fn=object_rows[:, 0].sum())


def nan_tp_div(tp: t.Tensor, y: t.Tensor) -> t.Tensor:
  """tp / y, NaN where tp == 0 (voxel_metrics.py:118-120)."""
  return t.where(tp == 0, t.full_like(tp, math.nan), tp / y)


def compute_voxel_metrics(tfpn: TfpnValues) -> VoxelMetrics:
  """IoU, precision and recall in float64; NaN for a class without a true positive (voxel_metrics.py:123-138)."""
  tp, fp, fn = (v.to(t.float64) for v in (tfpn.tp, tfpn.fp, tfpn.fn))
  return VoxelMetrics(iou=nan_tp_div(tp, tp + fp + fn), precision=nan_tp_div(tp, tp + fp), recall=nan_tp_div(tp, tp + fn))


def check_eval_labels_args(score_shape, dev: t.device, gt: Optional[t.Tensor], num_classes: Optional[int],
                           scene_classes: Optional[t.Tensor], m: int, labels: Optional[t.Tensor], cm: Optional[t.Tensor],
                           bad: Optional[t.Tensor]) -> int:
  """Every shape, dtype and device rule of crn_eval_labels' tensors other than the scores themselves, for scores of
  shape score_shape [B, C, D, H, W] on dev; ValueError otherwise.  Returns K (num_classes, default C).  gt, cm and bad
  go together: cm and bad without gt are checked too, gt without them is the caller's to settle."""
  if len(score_shape) != 5:
    raise ValueError(f"label_confusion: scores must be [B, C, D, H, W], got {tuple(score_shape)}")
  if dev.type not in ("cuda", "cpu"):
    raise ValueError(f"label_confusion: unsupported device {dev}")
  B, C, D, H, W = (int(v) for v in score_shape)
  K = C if num_classes is None else int(num_classes)
  if min(B, D, H, W) < 1 or not 1 <= C <= 32 or not 1 <= K <= 64 or m < 1:
    raise ValueError(f"label_confusion: scores {tuple(score_shape)}, num_classes {K}, m {m}: need 1 <= C <= 32, "
                     "1 <= num_classes <= 64, m >= 1 and no empty axis")
  if 4 * B * max(C, m ** 3) * D * H * W >= 2 ** 63:
    raise ValueError(f"label_confusion: scores {tuple(score_shape)} at m {m}: the grids do not fit 64-bit offsets")
  fine = (B, m * D, m * H, m * W)
  for x, what, shape, dtype in ((gt, "gt", fine, t.int32), (cm, "cm", (K, K), t.int64), (bad, "bad", (1,), t.int32),
                                (scene_classes, "scene_classes", (B,), t.int32), (labels, "labels", fine, t.int32)):
    if x is not None and (x.dtype != dtype or tuple(x.shape) != shape or x.device != dev or not x.is_contiguous()):
      raise ValueError(f"label_confusion: {what} must be contiguous {dtype} {shape} on {dev}, got {tuple(x.shape)} "
                       f"{x.dtype} on {x.device}")
  return K


def label_confusion(scores: t.Tensor, gt: Optional[t.Tensor] = None, num_classes: Optional[int] = None,
                    scene_classes: Optional[t.Tensor] = None, m: int = 1, offset_index: int = 0,
                    labels: Optional[t.Tensor] = None, cm: Optional[t.Tensor] = None,
                    bad: Optional[t.Tensor] = None) -> Tuple[t.Tensor, Optional[t.Tensor], Optional[t.Tensor]]:
  """One native pass of an x m evaluation (crn_eval_labels): returns (labels, cm, bad).

  scores f32 [B, C, D, H, W]: logits or a pmf of pass offset_index = (iz * m + iy) * m + ix.  labels int32
  [B, mD, mH, mW] (allocated, uninitialised outside this pass's sub-lattice, when None) receives argmax * scene class at
  (z*m+iz, y*m+iy, x*m+ix).  With gt int32 [B, mD, mH, mW]: cm int64 [K, K] (gt, predicted) and bad int32 [1] are
  accumulated (zeros when None), K = num_classes (default C); a voxel whose scaled label or prediction is outside [0, K)
  goes to bad[0] and is not counted.  scene_classes int32 [B] (fg_bg: the label of the scene's mesh) multiplies both.
  All tensors on the scores' device; nothing is read back."""
  if scores.dtype != t.float32:
    raise ValueError(f"label_confusion: scores must be float32, got {scores.dtype}")
  dev = scores.device
  m, n = int(m), int(offset_index)
  K = check_eval_labels_args(scores.shape, dev, gt, num_classes, scene_classes, m, labels, cm, bad)
  if not 0 <= n < m ** 3:
    raise ValueError(f"label_confusion: offset_index {n} outside [0, {m}^3)")
  B, C, D, H, W = scores.shape
  if gt is not None:
    if cm is None:
      cm = t.zeros((K, K), dtype=t.int64, device=dev)
    if bad is None:
      bad = t.zeros((1,), dtype=t.int32, device=dev)
  if labels is None:
    labels = t.empty((B, m * D, m * H, m * W), dtype=t.int32, device=dev)
  scores = scores.contiguous()
  if dev.type == "cuda":
    default_backend().eval_labels(scores, gt, scene_classes, B, C, K, D, H, W, m, n, labels, cm, bad)
  else:
    from corenet_amd import _lib
    p = _lib.ptr
    _lib.lib().crn_eval_labels_cpu(p(scores), p(gt), p(scene_classes), B, C, K, D, H, W, m, n, p(labels), p(cm), p(bad),
                                   t.get_num_threads())
  return labels, cm, bad
