"""Image-space evaluation on the renderer's geometry buffers (visualization.render.render_geometry): does a predicted
scene cover the same pixels, at the same depth and with the same labels as the true one, seen from the input camera.

Three small functions over per-image tensors [I, H, W]; they run on the tensors' device with torch ops, except the label
table, which is the overlap kernel's count (voxel_overlap.label_overlaps on [I, 1, H, W] grids).  Integer results are
exact.  The depth sums are float64 and are added in a fixed pairwise order (halves onto halves, elementwise), so the host
and the GPU give the same bits.  evaluation_results.reprojection_metrics_for_batch builds the per-scene rows on these
(DESIGN section 21)."""
from __future__ import annotations

from typing import NamedTuple

import torch as t


class SilhouetteCounts(NamedTuple):
  intersection: t.Tensor     # i64 [I]
  union: t.Tensor            # i64 [I]
  iou: t.Tensor              # f64 [I], NaN where the union is 0


class DepthErrors(NamedTuple):
  """Per image, over the pixels of `valid`: the sums behind the usual depth errors.  mean abs = abs_sum / count,
  RMSE = sqrt(sq_sum / count), abs-rel = abs_rel_sum / count, delta_1 = delta1_count / count."""
  count: t.Tensor            # i64 [I]
  abs_sum: t.Tensor          # f64 [I]: sum |dp - dg|
  sq_sum: t.Tensor           # f64 [I]: sum (dp - dg)^2
  abs_rel_sum: t.Tensor      # f64 [I]: sum |dp - dg| / dg
  delta1_count: t.Tensor     # i64 [I]: pixels with max(dp / dg, dg / dp) < 1.25


def _images(x, name: str, like=None) -> t.Tensor:
  x = t.as_tensor(x)
  if x.dim() != 3 or (like is not None and (tuple(x.shape) != tuple(like.shape) or x.device != like.device)):
    want = "[I, H, W]" if like is None else f"{tuple(like.shape)} on {like.device}"
    raise ValueError(f"image_metrics: {name} must be {want}, got {tuple(x.shape)} on {x.device}")
  return x


def _iou(intersection: t.Tensor, union: t.Tensor) -> t.Tensor:
  nan = t.full((), float("nan"), dtype=t.float64, device=union.device)
  return t.where(union > 0, intersection.to(t.float64) / union.to(t.float64), nan)


def silhouette_counts(pred_mask, gt_mask) -> SilhouetteCounts:
  """Intersection, union and IoU per image of two masks bool [I, H, W] (GeometryBuffers.mask)."""
  p = _images(pred_mask, "pred_mask")
  g = _images(gt_mask, "gt_mask", p)
  if p.dtype != t.bool or g.dtype != t.bool:
    raise ValueError(f"image_metrics: masks must be bool, got {p.dtype} and {g.dtype}")
  inter = (p & g).flatten(1).sum(1)
  union = (p | g).flatten(1).sum(1)
  return SilhouetteCounts(inter, union, _iou(inter, union))


def _pairwise_sum(x: t.Tensor) -> t.Tensor:
  """Sum over dim 1 of f64 [I, N] in an order that does not depend on the device: pad to a power of two with zeros, then
  add the upper half onto the lower until one column is left."""
  n = 1
  while n < x.shape[1]:
    n *= 2
  if n != x.shape[1]:
    x = t.cat([x, x.new_zeros((x.shape[0], n - x.shape[1]))], 1)
  while n > 1:
    n //= 2
    x = x[:, :n] + x[:, n:]
  return x[:, 0]


def depth_errors(pred_depth, gt_depth, valid) -> DepthErrors:
  """The depth-error sums per image of two depth images f32 [I, H, W] (GeometryBuffers.depth) over the pixels of valid
  bool [I, H, W], which the caller builds as covered on both sides (depths there are finite and positive).  Differences
  and sums are float64."""
  dp = _images(pred_depth, "pred_depth")
  dg = _images(gt_depth, "gt_depth", dp)
  v = _images(valid, "valid", dp)
  if v.dtype != t.bool or not dp.is_floating_point() or not dg.is_floating_point():
    raise ValueError(f"image_metrics: depths must be floating and valid bool, got {dp.dtype}, {dg.dtype}, {v.dtype}")
  v = v.flatten(1)
  one = t.ones((), dtype=t.float64, device=dp.device)
  dp = t.where(v, dp.flatten(1).to(t.float64), one)                    # 1 vs 1 outside valid: every term is 0 there
  dg = t.where(v, dg.flatten(1).to(t.float64), one)
  err = (dp - dg).abs()
  ratio = t.maximum(dp / dg, dg / dp)
  return DepthErrors(v.sum(1), _pairwise_sum(err), _pairwise_sum(err * err), _pairwise_sum(err / dg),
                     (v & (ratio < 1.25)).sum(1))


def label_image_overlaps(pred_labels, gt_labels, num_classes: int) -> t.Tensor:
  """The pixel table int64 [I, C, C] of two label images [I, H, W] with labels in [0, C): entry [i, p, g] counts the
  pixels of image i that are p in pred_labels and g in gt_labels (0: background).  A pixel with a label outside [0, C)
  on either side is counted nowhere.  The count is voxel_overlap.label_overlaps on [I, 1, H, W] grids."""
  from corenet_amd import voxel_overlap
  p = _images(pred_labels, "pred_labels")
  g = _images(gt_labels, "gt_labels", p)
  C = int(num_classes)
  if C < 1:
    raise ValueError(f"image_metrics: num_classes must be positive, got {num_classes}")
  I = p.shape[0]
  dev = p.device
  table = t.zeros((I, C, C), dtype=t.int64, device=dev)
  if I == 0:
    return table
  top = t.full((I,), C - 1, dtype=t.int64, device=dev)
  ov = voxel_overlap.label_overlaps(p[:, None], g[:, None], num_a=top, num_b=top)
  table[voxel_overlap._grid_of_rows(ov.offsets, dev), ov.a.to(t.int64), ov.b.to(t.int64)] = ov.count
  return table
