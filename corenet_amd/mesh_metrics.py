"""Surface metrics of predicted against ground-truth meshes: Chamfer distance and F-score at distance thresholds, from
area-weighted point samples and brute-force nearest neighbours.  CUDA(HIP) tensors run the kernels of
csrc/point_metrics.hip, CPU tensors the library's host twin (csrc/point_metrics_cpu.cpp); both give the same arrays bit
for bit and a CUDA tensor never goes to the host twin.  The reference project reports voxel IoU only; these are the
surface metrics other single-view reconstruction work is compared on.

Objects are ragged everywhere: N objects share one buffer and are described by int64 offsets [N + 1] (CSR); an object
may be empty.  Offsets may live on any device (they are small; one copy to the host sizes the launch).

Contract (arithmetic in csrc/point_metrics_common.h):
  * sample_surface_points: a triangle's weight is round(area / largest area of its object * 2^24), an integer (the area
    is |cross| in float32; zero, NaN and infinite areas weigh 0 and never receive a sample).  Sample i of S draws u_i in
    [0, 1) and takes the triangle whose interval of the running integer sum contains floor((i + u_i) / S * total): one
    sample per stratum of 1 / S of the surface.  Its position is the square-root warp of two more uniforms,
    r = sqrt(u1), barycentrics (1 - r, r (1 - u2), r u2).  The uniforms are 24-bit mantissas of a counter-based hash of
    (seed, i, 0 / 1 / 2).  A row depends only on (the object's triangles, S, seed): not on the other objects of the
    call, the device or the launch.
  * nearest_distances: d2 = (dx*dx + dy*dy) + dz*dz in float32 without contraction, dx = ax - bx; the winner is the
    minimum of (d2, index), ties to the lowest index; a candidate whose d2 is NaN is never chosen; a query with no
    eligible candidate (an empty object, a NaN query) gets +inf and -1.
  * chamfer_fscore: per object, float64 means of sqrt(d2) (accuracy: pred -> gt, completeness: gt -> pred), of d2
    (chamfer_l2), exact integer counts of d2 <= tau^2 (both sides float32) -> precision, recall and
    fscore = 2 P R / (P + R) (0 when P + R = 0).  Both sets empty: every field NaN; exactly one empty: the distances
    are +inf and precision, recall and fscore 0.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Tuple

import torch as t


class SurfaceSamples(NamedTuple):
  points: t.Tensor         # f32 [N, S, 3]
  tri_index: t.Tensor      # i32 [N, S], local to the object; -1 where the object is not valid
  valid: t.Tensor          # bool [N]: the object has a triangle of positive finite area


class SurfaceMetrics(NamedTuple):
  accuracy: t.Tensor           # f64 [N]   mean distance pred -> gt
  completeness: t.Tensor       # f64 [N]   mean distance gt -> pred
  chamfer_l1: t.Tensor         # f64 [N]   (accuracy + completeness) / 2
  chamfer_l2: t.Tensor         # f64 [N]   the same on squared distances
  precision: t.Tensor          # f64 [N, K] share of pred points within tau_k of gt
  recall: t.Tensor             # f64 [N, K] share of gt points within tau_k of pred
  fscore: t.Tensor             # f64 [N, K]
  precision_count: t.Tensor    # i64 [N, K] pred points within tau_k
  recall_count: t.Tensor       # i64 [N, K]
  num_pred: t.Tensor           # i64 [N]
  num_gt: t.Tensor             # i64 [N]


def _lib():
  from corenet_amd import _lib as L
  return L.lib()


def _host_offsets(offsets, total: int, what: str) -> t.Tensor:
  """Validated host copy (int64 [N + 1]) of CSR offsets over `total` elements."""
  off = t.as_tensor(offsets)
  if off.dim() != 1 or off.numel() < 1 or off.dtype not in (t.int64, t.int32):
    raise ValueError(f"{what}: offsets must be a rank-1 int64 tensor [N + 1], got {tuple(off.shape)} {off.dtype}")
  off = off.detach().to("cpu", t.int64)
  if int(off[0]) != 0 or int(off[-1]) != total or bool((off[1:] < off[:-1]).any()):
    raise ValueError(f"{what}: offsets must start at 0, never decrease and end at {total}")
  return off


def _points(x, what: str) -> t.Tensor:
  x = t.as_tensor(x)
  if x.dim() != 2 or x.shape[1] != 3 or x.dtype != t.float32:
    raise ValueError(f"{what}: expected float32 points [n, 3], got {tuple(x.shape)} {x.dtype}")
  return x.contiguous()


def _device_kind(dev: t.device, what: str) -> bool:
  if dev.type not in ("cuda", "cpu"):
    raise ValueError(f"{what}: unsupported device {dev}")
  return dev.type == "cuda"


def sample_surface_points(triangles, mesh_num_tri=None, num_samples: int = 16384, seed: int = 0,
                          offsets=None) -> SurfaceSamples:
  """num_samples area-stratified points on every object of a triangle soup.

  triangles f32 [T, 3, 3]; the objects are given either by mesh_num_tri (integers [N], consecutive runs of triangles, as
  BatchedExample.mesh_num_tri and marching cubes' num_faces) or by offsets int64 [N + 1].  Returns points [N, S, 3],
  tri_index [N, S] (local to the object) and valid [N] on the triangles' device."""
  tri = t.as_tensor(triangles)
  if tri.dim() != 3 or tuple(tri.shape[1:]) != (3, 3) or tri.dtype != t.float32:
    raise ValueError(f"sample_surface_points: expected float32 triangles [T, 3, 3], got {tuple(tri.shape)} {tri.dtype}")
  if (mesh_num_tri is None) == (offsets is None):
    raise ValueError("sample_surface_points: give exactly one of mesh_num_tri and offsets")
  if int(num_samples) != num_samples or num_samples < 1 or num_samples >= 1 << 31:
    raise ValueError(f"sample_surface_points: num_samples must be an integer in [1, 2^31), got {num_samples}")
  T, S = tri.shape[0], int(num_samples)
  if offsets is None:
    cnt = t.as_tensor(mesh_num_tri)
    if cnt.dim() != 1 or cnt.is_floating_point() or cnt.dtype == t.bool:
      raise ValueError(f"sample_surface_points: mesh_num_tri must be rank-1 integers, got {tuple(cnt.shape)} {cnt.dtype}")
    cnt = cnt.detach().to("cpu", t.int64)
    if bool((cnt < 0).any()):
      raise ValueError("sample_surface_points: negative triangle count")
    offsets = t.cat([t.zeros(1, dtype=t.int64), t.cumsum(cnt, 0)])
  off = _host_offsets(offsets, T, "sample_surface_points")
  N, dev = off.numel() - 1, tri.device
  gpu = _device_kind(dev, "sample_surface_points")
  tri = tri.contiguous()
  points = t.empty((N, S, 3), dtype=t.float32, device=dev)
  tri_index = t.empty((N, S), dtype=t.int32, device=dev)
  valid = t.empty((N,), dtype=t.bool, device=dev)
  if N == 0:
    return SurfaceSamples(points, tri_index, valid)
  if gpu:
    from corenet_amd.backend import default_backend
    default_backend().sample_surface(tri, off.to(dev), S, seed, points, tri_index, valid)
  else:
    _lib().crn_sample_surface_cpu(tri.data_ptr(), off.data_ptr(), N, S, int(seed) & 0xffffffff, points.data_ptr(),
                                  tri_index.data_ptr(), valid.data_ptr(), t.get_num_threads())
  return SurfaceSamples(points, tri_index, valid)


def _nearest(a: t.Tensor, a_off: t.Tensor, b: t.Tensor, b_off: t.Tensor) -> Tuple[t.Tensor, t.Tensor]:
  """nearest_distances on validated inputs; a_off / b_off: host int64."""
  dev, N = a.device, a_off.numel() - 1
  dist2 = t.empty((a.shape[0],), dtype=t.float32, device=dev)
  index = t.empty((a.shape[0],), dtype=t.int32, device=dev)
  if N == 0 or a.shape[0] == 0:
    return dist2, index
  max_na, max_nb = int((a_off[1:] - a_off[:-1]).max()), int((b_off[1:] - b_off[:-1]).max())
  if max_nb >= 1 << 31:
    raise ValueError("nearest_distances: an object has 2^31 or more candidates (indices are int32)")
  if dev.type == "cuda":
    from corenet_amd.backend import default_backend
    default_backend().nearest(a, a_off.to(dev), b, b_off.to(dev), max_na, max_nb, dist2, index)
  else:
    _lib().crn_nearest_cpu(a.data_ptr(), a_off.data_ptr(), b.data_ptr(), b_off.data_ptr(), N, dist2.data_ptr(),
                           index.data_ptr(), t.get_num_threads())
  return dist2, index


def _nearest_args(a, a_offsets, b, b_offsets, what: str):
  a, b = _points(a, what + ": a"), _points(b, what + ": b")
  if a.device != b.device:
    raise ValueError(f"{what}: a is on {a.device}, b on {b.device}")
  _device_kind(a.device, what)
  a_off = _host_offsets(a_offsets, a.shape[0], what + ": a")
  b_off = _host_offsets(b_offsets, b.shape[0], what + ": b")
  if a_off.numel() != b_off.numel():
    raise ValueError(f"{what}: {a_off.numel() - 1} objects of queries, {b_off.numel() - 1} of candidates")
  return a, a_off, b, b_off


def nearest_distances(a, a_offsets, b, b_offsets) -> Tuple[t.Tensor, t.Tensor]:
  """For every query of a f32 [Na, 3] the nearest candidate of the SAME object of b f32 [Nb, 3]: (dist2 f32 [Na], index
  i32 [Na], local to the object).  Brute force and deterministic (see the module docstring for the rules)."""
  return _nearest(*_nearest_args(a, a_offsets, b, b_offsets, "nearest_distances"))


def _segment_sums(off: t.Tensor, dev, *values: t.Tensor):
  """Per-object sums over axis 0 of values laid out by the host offsets `off`: the objects' rows are padded to the
  longest object ([N, L, ...], scattered without accumulation) and summed along L.  No atomics: the same inputs give the
  same bits on every run."""
  N, total = off.numel() - 1, int(off[-1])
  cnt = off[1:] - off[:-1]
  L = int(cnt.max()) if N else 0
  if total and not bool((cnt == L).all()):
    owner = t.repeat_interleave(t.arange(N, device=dev), cnt.to(dev), output_size=total)
    pos = t.arange(total, device=dev) - off.to(dev)[owner]
  out = []
  for v in values:
    if total == 0:
      out.append(t.zeros((N,) + tuple(v.shape[1:]), dtype=v.dtype, device=dev))
    elif bool((cnt == L).all()):
      out.append(v.reshape((N, L) + tuple(v.shape[1:])).sum(1))
    else:
      pad = t.zeros((N, L) + tuple(v.shape[1:]), dtype=v.dtype, device=dev)
      pad[owner, pos] = v
      out.append(pad.sum(1))
  return out


def _one_side(d2: t.Tensor, off: t.Tensor, tau2: t.Tensor):
  """Per object: float64 sums of sqrt(d2) and of d2, int64 counts of d2 <= tau2, number of points."""
  dev = d2.device
  d2d = d2.to(t.float64)
  within = (d2[:, None] <= tau2.to(dev)[None, :]).to(t.int64)              # float32 on both sides
  s1, s2, c = _segment_sums(off, dev, d2d.sqrt(), d2d, within)
  return s1, s2, c, (off[1:] - off[:-1]).to(dev)


def chamfer_fscore(pred, pred_offsets, gt, gt_offsets, thresholds: Sequence[float]) -> SurfaceMetrics:
  """Chamfer distance and F-score of N predicted point sets against N ground-truth point sets, one row per object.

  pred f32 [Np, 3] / gt f32 [Ng, 3] with their offsets [N + 1]; thresholds: K distances tau_k in the points' units.  Two
  nearest-neighbour calls (pred -> gt, gt -> pred); the reductions are small torch ops in float64 without atomics (two
  runs agree bit for bit), the threshold counts exact integers.  All fields are on the points' device."""
  pred, p_off, gt, g_off = _nearest_args(pred, pred_offsets, gt, gt_offsets, "chamfer_fscore")
  tau = t.as_tensor(thresholds, dtype=t.float32).reshape(-1).cpu()
  if bool((~(tau >= 0)).any()):
    raise ValueError(f"chamfer_fscore: thresholds must be >= 0, got {tau.tolist()}")
  tau2 = tau * tau                                                          # float32, on the host for either device
  d2_pg, _ = _nearest(pred, p_off, gt, g_off)
  d2_gp, _ = _nearest(gt, g_off, pred, p_off)
  sp, sp2, cp, np_ = _one_side(d2_pg, p_off, tau2)
  sg, sg2, cg, ng = _one_side(d2_gp, g_off, tau2)
  has_p, has_g = np_ > 0, ng > 0
  nan, inf = float("nan"), float("inf")

  def mean(s, n, has):
    m = s / n.clamp(min=1).to(t.float64)
    m = t.where(has, m, t.full_like(m, inf))                                # no points on this side: +inf ...
    return t.where(has_p | has_g, m, t.full_like(m, nan))                   # ... unless both are empty: NaN

  acc, comp = mean(sp, np_, has_p), mean(sg, ng, has_g)
  acc2, comp2 = mean(sp2, np_, has_p), mean(sg2, ng, has_g)

  def share(c, n):
    r = c.to(t.float64) / n.clamp(min=1).to(t.float64)[:, None]
    return t.where((has_p | has_g)[:, None], r, t.full_like(r, nan))

  P, R = share(cp, np_), share(cg, ng)
  den = P + R
  F = t.where(den > 0, 2 * P * R / t.where(den > 0, den, t.ones_like(den)), t.where(den == 0, t.zeros_like(den), den))
  return SurfaceMetrics(acc, comp, (acc + comp) / 2, (acc2 + comp2) / 2, P, R, F, cp, cg, np_, ng)
