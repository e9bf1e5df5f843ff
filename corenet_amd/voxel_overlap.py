"""Label overlaps of two voxel grids, and what per-object evaluation builds on them: segment sizes, IoU matching of
segments and panoptic quality.

label_overlaps counts, for N pairs of label grids, how many voxels carry label i in one grid and label j in the other.
CUDA(HIP) tensors run the kernel of csrc/voxel_overlap.hip, CPU tensors the library's host twin
(csrc/voxel_overlap_cpu.cpp).  Both give the same tensors exactly; a CUDA tensor never goes to the host twin.

Contract:
  * a, b: [N, D, H, W], N independent pairs of grids of one shape on one device; anything else raises ValueError, and so
    does D*H*W > 2^31 - 1.  N == 0 returns empty results.  W stride 1 (a view with another W stride is copied first),
    N / D / H strides arbitrary, so `labels[:, ::2]` and `labels[..., 1:]` need no copy.
  * Labels are integers: bool grids become a uint8 mask, uint8 and int32 grids are taken as they are, other integer types
    become int32 (values beyond it wrap, as torch's conversion does); floating grids raise ValueError.
  * num_a, num_b: int64 [N], the highest valid label of every grid (e.g. Components.num_components); a negative one
    raises ValueError.  Left None they are the per-grid maximum clamped at 0 -- one extra pass over that grid.
  * A voxel with a < 0, a > num_a[n], b < 0 or b > num_b[n] is counted in bad[n] and nowhere else.
  * The result is the sparse form of the (num_a[n] + 1) x (num_b[n] + 1) tables: every pair with a non-zero count,
    background (label 0) pairs included, sorted by (grid, a, b).  Segment sizes are row and column sums.
  * Integer adds only: identical from run to run and between GPU and host twin; nothing depends on
    crn_set_deterministic.  The kernel is queued on the current stream.  Reading num_a / num_b back sizes the tables (the
    one read of the counting part); compacting them (torch.nonzero) and the CSR offsets read the number of pairs back.

Three paths: a grid whose table has at most lds_entries entries is counted in LDS, a larger one directly in global
memory; a call is split into groups of grids whose tables together stay within max_table_entries, and a single grid
whose own table is larger goes through a sorted fallback in torch (unique with counts over 64-bit keys): the same
result, slow, there so that the function is total.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import torch as t

_MAX_VOXELS = (1 << 31) - 1
_MAX_LABEL = (1 << 31) - 2


class Overlaps(NamedTuple):
  offsets: t.Tensor           # i64 [N + 1] on the host: the pairs of grid n are rows offsets[n] .. offsets[n + 1]
  a: t.Tensor                 # i32 [P]
  b: t.Tensor                 # i32 [P]
  count: t.Tensor             # i64 [P], > 0
  num_a: t.Tensor             # i64 [N]
  num_b: t.Tensor             # i64 [N]
  bad: t.Tensor               # i64 [N]


class Matches(NamedTuple):
  """Segments are indexed CSR over grids with index 0 of every grid its background: segment (n, label) of a is row
  offsets_a[n] + label, as in segment_sizes."""
  offsets_a: t.Tensor         # i64 [N + 1] on the host
  offsets_b: t.Tensor         # i64 [N + 1] on the host
  size_a: t.Tensor            # i64 [Sa] voxels, after min_voxels_a folded small segments into the background
  size_b: t.Tensor            # i64 [Sb]
  valid_a: t.Tensor           # bool [Sa]: label > 0, at least one voxel, not folded -- the segments that count
  valid_b: t.Tensor           # bool [Sb]: label > 0 -- every label of b counts, with or without voxels
  partner_a: t.Tensor         # i32 [Sa]: the label of b the segment is matched to, 0 if none
  iou_a: t.Tensor             # f64 [Sa]: the IoU of that match, 0 if none
  partner_b: t.Tensor         # i32 [Sb]
  iou_b: t.Tensor             # f64 [Sb]
  best_iou_b: t.Tensor        # f64 [Sb]: the best IoU with a valid segment of a of the same class, matched or not
  class_a: Optional[t.Tensor]  # i32 [Sa] as given
  class_b: Optional[t.Tensor]  # i32 [Sb]


class PanopticCounts(NamedTuple):
  tp: t.Tensor                # i64 [N, num_classes]
  fp: t.Tensor                # i64 [N, num_classes]
  fn: t.Tensor                # i64 [N, num_classes]
  sum_iou: t.Tensor           # f64 [N, num_classes]: the IoU of the matched pairs, summed

  @property
  def sq(self) -> t.Tensor:
    return panoptic_scores(self.tp, self.fp, self.fn, self.sum_iou)[1]

  @property
  def rq(self) -> t.Tensor:
    return panoptic_scores(self.tp, self.fp, self.fn, self.sum_iou)[2]

  @property
  def pq(self) -> t.Tensor:
    return panoptic_scores(self.tp, self.fp, self.fn, self.sum_iou)[0]


def panoptic_scores(tp, fp, fn, sum_iou) -> Tuple[t.Tensor, t.Tensor, t.Tensor]:
  """(PQ, SQ, RQ) in float64: SQ = sum_iou / tp, RQ = tp / (tp + fp / 2 + fn / 2), PQ = sum_iou / (tp + fp / 2 + fn / 2),
  which is SQ * RQ wherever tp > 0; each is NaN where its own denominator is 0."""
  tp, fp, fn = (t.as_tensor(x).to(t.float64) for x in (tp, fp, fn))
  sum_iou = t.as_tensor(sum_iou).to(t.float64)
  den = tp + 0.5 * fp + 0.5 * fn
  return sum_iou / den, sum_iou / tp, tp / den


def _lib():
  from corenet_amd import _lib as L
  return L.lib()


def overlap_tiles() -> Tuple[int, int, int]:
  """(chunk, lds_entries, max_table_entries): a workgroup owns `chunk` consecutive voxels of a grid; a table of at most
  lds_entries entries is counted in LDS; a native call holds tables of at most max_table_entries entries together."""
  out = (C.c_int32 * 3)()
  _lib().crn_voxel_overlap_tiles(C.addressof(out))
  return int(out[0]), int(out[1]), int(out[2])


def _prepare(grid: t.Tensor, what: str) -> t.Tensor:
  """The uint8 / int32 tensor with W stride 1 the library takes."""
  if grid.dtype.is_floating_point or grid.dtype.is_complex:
    raise ValueError(f"label_overlaps: {what} must hold integer labels, got {grid.dtype}")
  if grid.dtype == t.bool:
    grid = grid.to(t.uint8)
  elif grid.dtype not in (t.uint8, t.int32):
    grid = grid.to(t.int32)
  if grid.stride(-1) != 1:
    grid = grid.contiguous()
  return grid


def _highest(grid: t.Tensor, num, what: str) -> t.Tensor:
  N = grid.shape[0]
  if num is None:
    return grid.amax(dim=(1, 2, 3)).to(t.int64).clamp_(min=0)               # the extra pass
  num = t.as_tensor(num)
  if num.dtype.is_floating_point or num.dtype == t.bool or tuple(num.shape) != (N,):
    raise ValueError(f"label_overlaps: {what} must be an integer tensor of shape [{N}], got {num.dtype} {tuple(num.shape)}")
  return num.to(device=grid.device, dtype=t.int64).contiguous()


def _sorted_overlaps(a: t.Tensor, b: t.Tensor, na: int, nb: int):
  """One grid through torch: (a, b, count) sorted by (a, b) and the bad count.  64-bit keys; slow."""
  ga, gb = a.reshape(-1).to(t.int64), b.reshape(-1).to(t.int64)
  ok = (ga >= 0) & (ga <= na) & (gb >= 0) & (gb <= nb)
  key, count = t.unique(ga[ok] * (nb + 1) + gb[ok], return_counts=True)
  ia = t.div(key, nb + 1, rounding_mode="floor")
  return ia, key - ia * (nb + 1), count, ga.numel() - ok.sum()


def label_overlaps(a, b, num_a=None, num_b=None, _max_table_entries: Optional[int] = None) -> Overlaps:
  """The overlap table of N pairs of label grids in sparse form (see the module docstring for the contract)."""
  a, b = t.as_tensor(a), t.as_tensor(b)
  if a.dim() != 4 or tuple(a.shape) != tuple(b.shape) or a.device != b.device:
    raise ValueError(f"label_overlaps: a and b must be [N, D, H, W] grids of one shape on one device, got "
                     f"{tuple(a.shape)} on {a.device} and {tuple(b.shape)} on {b.device}")
  N, D, H, W = a.shape
  dev = a.device
  if dev.type not in ("cuda", "cpu"):
    raise ValueError(f"label_overlaps: unsupported device {dev}")
  if N and (D == 0 or H == 0 or W == 0):
    raise ValueError(f"label_overlaps: empty grid extent {tuple(a.shape)}")
  if D * H * W > _MAX_VOXELS:
    raise ValueError(f"label_overlaps: grid of {D}x{H}x{W} too large (at most 2^31 - 1 voxels per grid)")
  a, b = _prepare(a, "a"), _prepare(b, "b")
  if N == 0:
    z64, z32 = t.zeros(0, dtype=t.int64, device=dev), t.zeros(0, dtype=t.int32, device=dev)
    return Overlaps(t.zeros(1, dtype=t.int64), z32, z32.clone(), z64, z64.clone(), z64.clone(), z64.clone())
  num_a, num_b = _highest(a, num_a, "num_a"), _highest(b, num_b, "num_b")
  host = t.stack([num_a, num_b]).cpu()                                       # the read that sizes the tables
  if bool((host < 0).any()) or bool((host > _MAX_LABEL).any()):
    raise ValueError(f"label_overlaps: num_a and num_b must lie in [0, 2^31 - 2], got {host.tolist()}")
  na, nb = host[0].tolist(), host[1].tolist()
  entries = [(x + 1) * (y + 1) for x, y in zip(na, nb)]
  cap = overlap_tiles()[2] if _max_table_entries is None else int(_max_table_entries)
  if cap < 1:
    raise ValueError(f"label_overlaps: _max_table_entries must be positive, got {cap}")
  bad = t.zeros(N, dtype=t.int64, device=dev)
  grids, ias, ibs, counts = [], [], [], []
  n = 0
  while n < N:
    if entries[n] > cap:                                                     # the sorted fallback, one grid
      ia, ib, count, nbad = _sorted_overlaps(a[n], b[n], na[n], nb[n])
      bad[n] = nbad
      g = t.full_like(ia, n)
      n += 1
    else:
      m, total = n, 0
      while m < N and entries[m] <= cap and total + entries[m] <= cap:
        total += entries[m]
        m += 1
      offsets = t.zeros(m - n + 1, dtype=t.int64)
      offsets[1:] = t.cumsum(t.tensor(entries[n:m], dtype=t.int64), 0)
      table = t.empty(total, dtype=t.int64, device=dev)
      if dev.type == "cuda":
        from corenet_amd.backend import default_backend
        default_backend().voxel_overlap(a[n:m], b[n:m], num_a[n:m], num_b[n:m], offsets, table, bad[n:m])
      else:
        from corenet_amd.backend import _DTYPE_CODE
        sa, sb = (C.c_int64 * 4)(*a.stride()), (C.c_int64 * 4)(*b.stride())
        _lib().crn_voxel_overlap_cpu(a[n:m].data_ptr(), sa, _DTYPE_CODE[a.dtype], b[n:m].data_ptr(), sb, _DTYPE_CODE[b.dtype],
                                     m - n, D, H, W, num_a[n:m].data_ptr(), num_b[n:m].data_ptr(), offsets.data_ptr(),
                                     table.data_ptr(), bad[n:m].data_ptr(), t.get_num_threads())
      flat = t.nonzero(table)[:, 0]                                          # ascending: (grid, a, b) order
      count = table[flat]
      off = offsets.to(dev)
      g = t.searchsorted(off, flat, right=True) - 1
      local = flat - off[g]
      width = (num_b[n:m] + 1)[g]
      ia = t.div(local, width, rounding_mode="floor")
      ib = local - ia * width
      g = g + n
      n = m
    grids.append(g), ias.append(ia), ibs.append(ib), counts.append(count)
  g = t.cat(grids)
  offsets = t.zeros(N + 1, dtype=t.int64)
  offsets[1:] = t.cumsum(t.bincount(g, minlength=N).cpu(), 0)
  return Overlaps(offsets, t.cat(ias).to(t.int32), t.cat(ibs).to(t.int32), t.cat(counts), num_a, num_b, bad)


def _grid_of_rows(offsets: t.Tensor, dev) -> t.Tensor:
  """int64 [offsets[-1]] on dev: the grid of every row of a CSR table with host offsets."""
  N = offsets.numel() - 1
  return t.repeat_interleave(t.arange(N, device=dev), (offsets[1:] - offsets[:-1]).to(dev), output_size=int(offsets[N]))


def _segment_offsets(num: t.Tensor) -> t.Tensor:
  off = t.zeros(num.numel() + 1, dtype=t.int64)
  off[1:] = t.cumsum(num.cpu() + 1, 0)
  return off


def segment_sizes(overlaps: Overlaps) -> Tuple[t.Tensor, t.Tensor, t.Tensor, t.Tensor]:
  """(size_a, size_b, offsets_a, offsets_b): the voxels of every segment as the row and column sums of the tables, CSR
  over grids with index 0 the background: segment (n, label) of a is size_a[offsets_a[n] + label].  The offsets are on
  the host (one read of num_a and num_b).  Bad voxels are in no size."""
  dev = overlaps.count.device
  off_a, off_b = _segment_offsets(overlaps.num_a), _segment_offsets(overlaps.num_b)
  g = _grid_of_rows(overlaps.offsets, dev)
  size_a = t.zeros(int(off_a[-1]), dtype=t.int64, device=dev).index_add_(0, off_a.to(dev)[g] + overlaps.a, overlaps.count)
  size_b = t.zeros(int(off_b[-1]), dtype=t.int64, device=dev).index_add_(0, off_b.to(dev)[g] + overlaps.b, overlaps.count)
  return size_a, size_b, off_a, off_b


def _classes(c, S: int, dev, what: str) -> Optional[t.Tensor]:
  if c is None:
    return None
  c = t.as_tensor(c)
  if c.dtype.is_floating_point or tuple(c.shape) != (S,):
    raise ValueError(f"match_segments: {what} must be an integer tensor of shape [{S}] (one class per segment, background "
                     f"rows included), got {c.dtype} {tuple(c.shape)}")
  return c.to(device=dev, dtype=t.int32)


def match_segments(overlaps: Overlaps, class_a=None, class_b=None, iou_threshold: float = 0.5, min_voxels_a: int = 0) -> Matches:
  """Matches the segments (labels > 0) of a to those of b by IoU = c / (|a| + |b| - c), in float64, where c is the
  overlap of the pair and |.| the segment sizes of segment_sizes.  A pair matches iff IoU > iou_threshold, strictly, and,
  when class_a and class_b are given (int32 per segment, CSR as in segment_sizes, e.g. ComponentStats.value behind a
  background row), its classes are equal; they are given both or neither.

  iou_threshold < 0.5 raises ValueError: from 0.5 on a segment has at most one partner, so no assignment has to be
  solved.  Proof: IoU > 1/2 means 2c > |a| + |b| - c, so 3c > |a| + |b| >= |a| + c and c > |a| / 2 -- the partner covers
  more than half of a, and the segments of b are disjoint, so only one of them can; the same holds for b.

  min_voxels_a = n > 0 first folds the segments of a with fewer than n voxels into a's background by re-aggregating the
  sparse rows -- no second pass over the grids; it equals filtering the grid with filter_components(min_voxels=n) when a
  holds connected components.  Runs in torch on the sparse table, which is small."""
  if not iou_threshold >= 0.5:
    raise ValueError(f"match_segments: iou_threshold must be at least 0.5 (below it a match is not unique), got {iou_threshold}")
  if int(min_voxels_a) != min_voxels_a or min_voxels_a < 0:
    raise ValueError(f"match_segments: min_voxels_a must be a non-negative integer, got {min_voxels_a}")
  if (class_a is None) != (class_b is None):
    raise ValueError("match_segments: give class_a and class_b both or neither")
  size_a, size_b, off_a, off_b = segment_sizes(overlaps)
  dev = size_a.device
  Sa, Sb = size_a.numel(), size_b.numel()
  class_a, class_b = _classes(class_a, Sa, dev, "class_a"), _classes(class_b, Sb, dev, "class_b")
  off_a_d, off_b_d = off_a.to(dev), off_b.to(dev)
  bg_a, bg_b = t.zeros(Sa, dtype=t.bool, device=dev), t.zeros(Sb, dtype=t.bool, device=dev)
  bg_a[off_a_d[:-1]] = True
  bg_b[off_b_d[:-1]] = True
  g = _grid_of_rows(overlaps.offsets, dev)
  ia, ib, count = off_a_d[g] + overlaps.a, off_b_d[g] + overlaps.b, overlaps.count
  folded = t.zeros(Sa, dtype=t.bool, device=dev)
  if min_voxels_a > 0:
    folded = (size_a < int(min_voxels_a)) & ~bg_a
    ia = t.where(folded[ia], off_a_d[g], ia)
    key, inverse = t.unique(ia * Sb + ib, return_inverse=True)               # sorted: still (grid, a, b) order
    count = t.zeros(key.numel(), dtype=t.int64, device=dev).index_add_(0, inverse, count)
    ia = t.div(key, Sb, rounding_mode="floor")
    ib = key - ia * Sb
    size_a = t.zeros(Sa, dtype=t.int64, device=dev).index_add_(0, ia, count)
  valid_a, valid_b = ~bg_a & ~folded & (size_a > 0), ~bg_b
  fg = valid_a[ia] & valid_b[ib]
  pa, pb, c = ia[fg], ib[fg], count[fg]
  iou = c.to(t.float64) / (size_a[pa] + size_b[pb] - c).to(t.float64)
  same = class_a[pa] == class_b[pb] if class_a is not None else t.ones_like(fg[fg])
  m = (iou > float(iou_threshold)) & same
  label_a = (pa - off_a_d[t.searchsorted(off_a_d, pa, right=True) - 1]).to(t.int32)
  label_b = (pb - off_b_d[t.searchsorted(off_b_d, pb, right=True) - 1]).to(t.int32)
  partner_a, partner_b = t.zeros(Sa, dtype=t.int32, device=dev), t.zeros(Sb, dtype=t.int32, device=dev)
  iou_a, iou_b = t.zeros(Sa, dtype=t.float64, device=dev), t.zeros(Sb, dtype=t.float64, device=dev)
  partner_a[pa[m]], iou_a[pa[m]] = label_b[m], iou[m]                        # at most one m per segment: no write meets another
  partner_b[pb[m]], iou_b[pb[m]] = label_a[m], iou[m]
  best_iou_b = t.zeros(Sb, dtype=t.float64, device=dev).scatter_reduce_(0, pb[same], iou[same], "amax", include_self=True)
  return Matches(off_a, off_b, size_a, size_b, valid_a, valid_b, partner_a, iou_a, partner_b, iou_b, best_iou_b, class_a, class_b)


def panoptic_quality(matches: Matches, num_classes: int) -> PanopticCounts:
  """Per (grid, class): tp, the matched pairs; fp, the valid segments of a without a partner; fn, the segments of b
  without one (a label of b without voxels is one); sum_iou, the IoU of the matched pairs.  Without classes every segment
  has class 0.  A class outside [0, num_classes) on a segment that counts raises ValueError.  PanopticCounts.pq / .sq /
  .rq (panoptic_scores) give the quotients, NaN where the denominator is 0."""
  num_classes = int(num_classes)
  if num_classes < 1:
    raise ValueError(f"panoptic_quality: num_classes must be positive, got {num_classes}")
  dev = matches.size_a.device
  N = matches.offsets_a.numel() - 1
  ga, gb = _grid_of_rows(matches.offsets_a, dev), _grid_of_rows(matches.offsets_b, dev)
  ca = t.zeros_like(ga) if matches.class_a is None else matches.class_a.to(t.int64)
  cb = t.zeros_like(gb) if matches.class_b is None else matches.class_b.to(t.int64)
  for c, valid, what in ((ca, matches.valid_a, "class_a"), (cb, matches.valid_b, "class_b")):
    if bool((((c < 0) | (c >= num_classes)) & valid).any()):
      raise ValueError(f"panoptic_quality: {what} has a class outside [0, {num_classes})")

  def per_class(group, cls, mask, weight=None):
    out = t.zeros(N * num_classes, dtype=t.int64 if weight is None else t.float64, device=dev)
    idx = (group * num_classes + cls)[mask]
    out.index_add_(0, idx, t.ones_like(idx) if weight is None else weight[mask])
    return out.reshape(N, num_classes)
  hit_b = matches.valid_b & (matches.partner_b > 0)
  return PanopticCounts(per_class(gb, cb, hit_b), per_class(ga, ca, matches.valid_a & (matches.partner_a == 0)),
                        per_class(gb, cb, matches.valid_b & ~hit_b), per_class(gb, cb, hit_b, matches.iou_b))
