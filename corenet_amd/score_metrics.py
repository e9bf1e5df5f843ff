"""Score-level evaluation: the probabilities of a prediction evaluated as probabilities.

score_histogram bins the scores of one native pass of an x m inference, per class and against the ground truth, into a
small integer table (`crn_eval_scores`): CUDA(HIP) tensors run the kernel of csrc/eval_scores.hip, CPU tensors the
library's host twin (csrc/eval_scores_cpu.cpp).  Both give the same tensors exactly; a CUDA tensor never goes to the host
twin.  Everything else here -- the reliability diagram, expected / maximum calibration error, the Brier score, the
IoU / precision / recall curve over the threshold with its best threshold, average precision -- follows from that table
in float64 torch, on whatever device the table is on.

Rows of a table: row r < K is class r (fg_bg: channel c scores class c * scene class), row K is the class-agnostic
foreground, scored with 1 - p_0 against gt != 0.  A score p in [0, 1] is q = rint(p * 2^24) in q24 units and falls into
bin min(nbins - 1, (q * nbins) >> 24)."""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import NamedTuple, Optional, Tuple

import torch as t

from corenet_amd import voxel_metrics
from corenet_amd.backend import default_backend

Q_ONE = 1 << 24
MAX_NBINS = 256
MAX_ENTRIES = 2048


@dataclasses.dataclass
class ScoreHistogram:
  """table int64 [K+1, nbins, 2, 2]: (row, bin, y, {count, sum of q}); sq int64 [K+1, 2]: (row, y) sums of the squared
  error in units of 2^-24; bad int64 [1]: voxels counted nowhere else; nbins."""
  table: t.Tensor
  sq: t.Tensor
  bad: t.Tensor
  nbins: int


class Reliability(NamedTuple):
  """Per row and bin, float64 [K+1, nbins]: the number of voxels, their mean score and the fraction of them that are
  positive (NaN for both in an empty bin)."""
  count: t.Tensor
  confidence: t.Tensor
  frequency: t.Tensor


class ThresholdCounts(NamedTuple):
  """int64 [K+1, nbins+1] at the thresholds j / nbins, j = 0..nbins."""
  tp: t.Tensor
  fp: t.Tensor
  fn: t.Tensor


def score_tiles() -> Tuple[int, int, int]:
  """(voxels of a sample one workgroup of the kernel takes, the limit of (K+1) * nbins, the limit of nbins)."""
  from corenet_amd import _lib
  out = (C.c_int32 * 3)()
  _lib.lib().crn_eval_scores_tiles(C.addressof(out))
  return int(out[0]), int(out[1]), int(out[2])


def _check(scores: t.Tensor, what: str):
  if not isinstance(scores, t.Tensor) or scores.dtype != t.float32:
    raise ValueError(f"{what}: scores must be float32, got {getattr(scores, 'dtype', type(scores))}")
  if scores.device.type not in ("cuda", "cpu"):
    raise ValueError(f"{what}: unsupported device {scores.device}")


def check_score_args(score_shape, dev: t.device, gt: t.Tensor, num_classes: Optional[int], scene_classes: Optional[t.Tensor],
                     m: int, nbins: int, out: Optional[ScoreHistogram]) -> int:
  """Every shape, dtype and device rule of crn_eval_scores' tensors other than the scores themselves, for scores of shape
  score_shape [B, C, D, H, W] on dev; ValueError otherwise.  Returns K (num_classes, default C)."""
  try:
    K = voxel_metrics.check_eval_labels_args(score_shape, dev, gt, num_classes, scene_classes, m, None, None, None)
  except ValueError as e:
    raise ValueError(str(e).replace("label_confusion:", "score_histogram:", 1)) from None
  if gt is None:
    raise ValueError("score_histogram: gt is required")
  nbins = int(nbins)
  if not 1 <= nbins <= MAX_NBINS or (K + 1) * nbins > MAX_ENTRIES:
    raise ValueError(f"score_histogram: nbins {nbins} with {K} classes: need 1 <= nbins <= {MAX_NBINS} and "
                     f"(num_classes + 1) * nbins <= {MAX_ENTRIES}")
  if out is not None:
    if int(out.nbins) != nbins:
      raise ValueError(f"score_histogram: out has {out.nbins} bins, nbins is {nbins}")
    for x, what, shape in ((out.table, "out.table", (K + 1, nbins, 2, 2)), (out.sq, "out.sq", (K + 1, 2)),
                           (out.bad, "out.bad", (1,))):
      if x.dtype != t.int64 or tuple(x.shape) != shape or x.device != dev or not x.is_contiguous():
        raise ValueError(f"score_histogram: {what} must be contiguous {t.int64} {shape} on {dev}, got {tuple(x.shape)} "
                         f"{x.dtype} on {x.device}")
  return K


def empty_histogram(num_classes: int, nbins: int, device) -> ScoreHistogram:
  K, nbins = int(num_classes), int(nbins)
  return ScoreHistogram(t.zeros((K + 1, nbins, 2, 2), dtype=t.int64, device=device),
                        t.zeros((K + 1, 2), dtype=t.int64, device=device), t.zeros((1,), dtype=t.int64, device=device), nbins)


def score_histogram(scores: t.Tensor, gt: t.Tensor, num_classes: Optional[int] = None,
                    scene_classes: Optional[t.Tensor] = None, nbins: int = 20, from_logits: bool = False, m: int = 1,
                    offset_index: int = 0, out: Optional[ScoreHistogram] = None) -> ScoreHistogram:
  """One native pass of an x m evaluation, binned by score (crn_eval_scores).

  scores f32 [B, C, D, H, W]: the pmf of pass offset_index = (iz * m + iy) * m + ix, or with from_logits its logits,
  which go through the shared softmax (softmax_scores) first.  gt int32 [B, mD, mH, mW]; coarse voxel (z, y, x) is
  scored against fine voxel (z*m+iz, y*m+iy, x*m+ix).  K = num_classes (default C); scene_classes int32 [B] (fg_bg: the
  label of the scene's mesh) scales the label and the row of a channel.  A voxel whose scene class is below 1, whose
  scaled label is outside [0, K), whose last channel's row is outside [0, K) or which has a score that is NaN or outside
  [0, 1] adds one to bad and is counted nowhere else.  Accumulates into `out` when given (zeros otherwise) and returns
  it.  Integer sums: the same bits on every run, on the GPU and on the host.  All tensors on the scores' device;
  nothing is read back."""
  _check(scores, "score_histogram")
  dev = scores.device
  m, n, nbins = int(m), int(offset_index), int(nbins)
  K = check_score_args(scores.shape, dev, gt, num_classes, scene_classes, m, nbins, out)
  if not 0 <= n < m ** 3:
    raise ValueError(f"score_histogram: offset_index {n} outside [0, {m}^3)")
  B, Cn, D, H, W = scores.shape
  if out is None:
    out = empty_histogram(K, nbins, dev)
  scores = scores.contiguous()
  if dev.type == "cuda":
    default_backend().eval_scores(scores, from_logits, gt, scene_classes, B, Cn, K, D, H, W, m, n, nbins, out.table, out.sq,
                                  out.bad)
  else:
    from corenet_amd import _lib
    p = _lib.ptr
    _lib.lib().crn_eval_scores_cpu(p(scores), int(bool(from_logits)), p(gt), p(scene_classes), B, Cn, K, D, H, W, m, n, nbins,
                                   p(out.table), p(out.sq), p(out.bad), t.get_num_threads())
  return out


def softmax_scores(logits: t.Tensor) -> t.Tensor:
  """The pmf score_histogram(from_logits=True) bins: the shared softmax over axis 1 of logits f32 [B, C, ...] (first
  maximum, exp built from +, * and bit operations, sum in channel order, one division per channel), the same bits on the
  GPU and on the host."""
  _check(logits, "softmax_scores")
  if logits.dim() < 2 or not 1 <= logits.shape[1] <= 32 or logits.numel() == 0:
    raise ValueError(f"softmax_scores: logits must be [B, C, ...] with 1 <= C <= 32 and no empty axis, got "
                     f"{tuple(logits.shape)}")
  logits = logits.contiguous()
  B, Cn = int(logits.shape[0]), int(logits.shape[1])
  S = logits[0, 0].numel()
  out = t.empty_like(logits)
  if logits.device.type == "cuda":
    default_backend().score_softmax(logits, B, Cn, S, out)
  else:
    from corenet_amd import _lib
    _lib.lib().crn_score_softmax_cpu(_lib.ptr(logits), B, Cn, S, _lib.ptr(out), t.get_num_threads())
  return out


# ---- derived quantities: float64 torch on the small tables -----------------------------------------

def _nan_div(a: t.Tensor, b: t.Tensor) -> t.Tensor:
  return t.where(b == 0, t.full_like(a, math.nan), a / t.where(b == 0, t.ones_like(b), b))


def reliability(h: ScoreHistogram) -> Reliability:
  """The reliability diagram: per row and bin the count, the mean score (confidence) and the positive frequency."""
  tab = h.table.to(t.float64)
  count = tab[..., 0].sum(-1)
  return Reliability(count, _nan_div(tab[..., 1].sum(-1) / Q_ONE, count), _nan_div(tab[:, :, 1, 0], count))


def _gaps(h: ScoreHistogram):
  r = reliability(h)
  gap = t.where(r.count == 0, t.zeros_like(r.count), (r.confidence - r.frequency).abs())
  return r.count, gap


def expected_calibration_error(h: ScoreHistogram) -> t.Tensor:
  """f64 [K+1]: sum over the bins of (count / total) * |confidence - frequency|; NaN for a row without voxels."""
  count, gap = _gaps(h)
  return _nan_div((count * gap).sum(1), count.sum(1))


def maximum_calibration_error(h: ScoreHistogram) -> t.Tensor:
  """f64 [K+1]: the largest |confidence - frequency| over the non-empty bins; NaN for a row without voxels."""
  count, gap = _gaps(h)
  return t.where(count.sum(1) == 0, t.full_like(gap[:, 0], math.nan), gap.max(1).values)


def brier_score(h: ScoreHistogram) -> t.Tensor:
  """f64 [K+1]: the mean squared difference between score and label; NaN for a row without voxels."""
  return _nan_div(h.sq.to(t.float64).sum(1) / Q_ONE, h.table[..., 0].sum((1, 2)).to(t.float64))


def threshold_counts(h: ScoreHistogram) -> ThresholdCounts:
  """tp / fp / fn at the thresholds j / nbins, j = 0..nbins: a voxel is predicted positive iff its bin is >= j, which
  by the integer binning is exactly q >= j * 2^24 / nbins (the last bin also holds q = 2^24, so at j = nbins nothing
  is predicted positive)."""
  cnt = h.table[..., 0]                                               # [K+1, nbins, 2]
  zero = t.zeros_like(cnt[:, :1])
  above = t.cat([cnt.flip(1).cumsum(1).flip(1), zero], 1)             # [K+1, nbins+1, 2]: voxels in bins >= j
  pos = cnt[:, :, 1].sum(1, keepdim=True)
  tp = above[..., 1]
  return ThresholdCounts(tp=tp, fp=above[..., 0], fn=pos - tp)


def threshold_curve(h: ScoreHistogram) -> voxel_metrics.VoxelMetrics:
  """IoU, precision and recall f64 [K+1, nbins+1] over the thresholds of threshold_counts; NaN where tp == 0
  (voxel_metrics.nan_tp_div)."""
  c = threshold_counts(h)
  return voxel_metrics.compute_voxel_metrics(voxel_metrics.TfpnValues(tp=c.tp, tn=t.zeros_like(c.tp), fp=c.fp, fn=c.fn))


def best_threshold(h: ScoreHistogram) -> Tuple[t.Tensor, t.Tensor]:
  """(threshold f64 [K+1], its IoU f64 [K+1]): per row the first threshold of maximum IoU; NaN for both in a row
  without positives."""
  iou = threshold_curve(h).iou
  filled = t.where(t.isnan(iou), t.full_like(iou, -1.0), iou)
  best = filled.max(1).values
  first = (filled == best[:, None]).to(t.int64).argmax(1)             # argmax of a 0/1 tensor: its first 1
  none = best < 0
  nan = t.full_like(best, math.nan)
  return t.where(none, nan, first.to(t.float64) / h.nbins), t.where(none, nan, best)


def average_precision(h: ScoreHistogram) -> t.Tensor:
  """f64 [K+1]: the step sum of (R_j - R_{j+1}) * P_j over the thresholds j = nbins-1 .. 0 (descending, R_nbins = 0);
  NaN for a row without positives."""
  c = threshold_counts(h)
  tp, fp = c.tp.to(t.float64), c.fp.to(t.float64)
  pos = (c.tp + c.fn)[:, :1].to(t.float64)
  recall = _nan_div(tp, pos.expand_as(tp))
  precision = t.where(tp == 0, t.zeros_like(tp), tp / t.where(tp + fp == 0, t.ones_like(tp), tp + fp))
  return ((recall[:, :-1] - recall[:, 1:]) * precision[:, :-1]).sum(1)
