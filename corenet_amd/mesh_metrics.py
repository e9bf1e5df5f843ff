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

Point to triangle (arithmetic pm_tri_record / pm_tri_d2 of csrc/point_metrics_common.h):
  * point_triangle_distances: for every query the triangle of the same object with the smallest (d2, index), d2 the
    squared Euclidean distance from the query to the closed triangle in float32.  A triangle is eligible when the sampler
    would give it samples (positive finite area: pm_area_ok(pm_area)); zero-area, collinear, NaN and infinite triangles
    are never chosen.  One exception: a triangle that passes this rule but whose frame is not finite in float32 (an edge
    length or the height over AB underflows to 0, or cancels to exactly 0 on an extreme sliver) becomes a record of NaNs
    and is never chosen either, although the sampler still draws from it.  A candidate is chosen only when its d2 is below +inf: never a NaN d2, nor one that overflows
    float32.  A query without such a candidate (an empty object, no eligible triangle, a NaN query) gets +inf and -1.
    Ties go to the lowest index.  A triangle becomes a record of 20 floats (an orthonormal frame at its first vertex, the
    edges' unit directions and lengths in that frame); d2 is z^2 plus the squared in-plane distance, which is 0 inside
    and the smallest of the three clamped edge distances elsewhere, by selects alone and without contraction.  The kernel
    and the host twin call the same two header functions and return the same dist2 and index bit for bit.
  * mesh_chamfer_fscore: both soups are sampled (sample_surface_points, same seed); the predicted samples are measured
    against the ground-truth TRIANGLES (accuracy, precision) and the ground-truth samples against the predicted triangles
    (completeness, recall), reduced as chamfer_fscore does.  Normal consistency of a sample is |n_src . n_near|, the
    unit normals (float64, from the float32 vertices) of the sample's own triangle and of the nearest triangle of the
    other mesh; per direction the float64 mean, overall the mean of the two directions.  An object with triangles but
    none eligible counts as empty; both sides empty: NaN, exactly one: distances +inf, F-score and normal consistency 0.
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


class MeshSurfaceMetrics(NamedTuple):
  """SurfaceMetrics (same fields, same meanings) measured from samples to triangles, plus normal consistency."""
  accuracy: t.Tensor
  completeness: t.Tensor
  chamfer_l1: t.Tensor
  chamfer_l2: t.Tensor
  precision: t.Tensor
  recall: t.Tensor
  fscore: t.Tensor
  precision_count: t.Tensor
  recall_count: t.Tensor
  num_pred: t.Tensor
  num_gt: t.Tensor
  normal_consistency: t.Tensor         # f64 [N]   mean of the two directions
  normal_consistency_pred: t.Tensor    # f64 [N]   mean |n . n| over the pred samples against the gt triangles
  normal_consistency_gt: t.Tensor      # f64 [N]   mean |n . n| over the gt samples against the pred triangles


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


def _thresholds(thresholds, what: str) -> t.Tensor:
  """tau^2 in float32 on the host (for either device)."""
  tau = t.as_tensor(thresholds, dtype=t.float32).reshape(-1).cpu()
  if bool((~(tau >= 0)).any()):
    raise ValueError(f"{what}: thresholds must be >= 0, got {tau.tolist()}")
  return tau * tau


def _metrics_of(d2_pg: t.Tensor, p_off: t.Tensor, d2_gp: t.Tensor, g_off: t.Tensor, tau2: t.Tensor) -> SurfaceMetrics:
  """The reductions of chamfer_fscore from the squared distances of both directions."""
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


def chamfer_fscore(pred, pred_offsets, gt, gt_offsets, thresholds: Sequence[float]) -> SurfaceMetrics:
  """Chamfer distance and F-score of N predicted point sets against N ground-truth point sets, one row per object.

  pred f32 [Np, 3] / gt f32 [Ng, 3] with their offsets [N + 1]; thresholds: K distances tau_k in the points' units.  Two
  nearest-neighbour calls (pred -> gt, gt -> pred); the reductions are small torch ops in float64 without atomics (two
  runs agree bit for bit), the threshold counts exact integers.  All fields are on the points' device."""
  pred, p_off, gt, g_off = _nearest_args(pred, pred_offsets, gt, gt_offsets, "chamfer_fscore")
  tau2 = _thresholds(thresholds, "chamfer_fscore")
  d2_pg, _ = _nearest(pred, p_off, gt, g_off)
  d2_gp, _ = _nearest(gt, g_off, pred, p_off)
  return _metrics_of(d2_pg, p_off, d2_gp, g_off, tau2)


def _triangles(x, what: str) -> t.Tensor:
  x = t.as_tensor(x)
  if x.dim() != 3 or tuple(x.shape[1:]) != (3, 3) or x.dtype != t.float32:
    raise ValueError(f"{what}: expected float32 triangles [T, 3, 3], got {tuple(x.shape)} {x.dtype}")
  return x.contiguous()


def point_triangle_tiles() -> Tuple[int, int]:
  """(queries a workgroup of the point-to-triangle kernel holds, triangle records of one LDS tile), as the library was
  built (crn_point_triangle_tile): the sizes at which the kernel takes another path."""
  return int(_lib().crn_point_triangle_tile(0)), int(_lib().crn_point_triangle_tile(1))


def point_triangle_splits(num_objects: int, max_np: int, max_nt: int) -> int:
  """The number of shares the kernel cuts the triangles of an object into for a launch of num_objects objects whose
  largest object has max_np queries and max_nt triangles (more than 1: the split launch with the atomicMin merge)."""
  return int(_lib().crn_point_triangle_splits(int(num_objects), int(max_np), int(max_nt)))


def _point_triangle(p: t.Tensor, p_off: t.Tensor, tri: t.Tensor, t_off: t.Tensor) -> Tuple[t.Tensor, t.Tensor]:
  """point_triangle_distances on validated inputs; p_off / t_off: host int64."""
  dev, N = p.device, p_off.numel() - 1
  dist2 = t.empty((p.shape[0],), dtype=t.float32, device=dev)
  index = t.empty((p.shape[0],), dtype=t.int32, device=dev)
  if N == 0 or p.shape[0] == 0:
    return dist2, index
  max_np, max_nt = int((p_off[1:] - p_off[:-1]).max()), int((t_off[1:] - t_off[:-1]).max())
  if max_nt >= 1 << 31:
    raise ValueError("point_triangle_distances: an object has 2^31 or more triangles (indices are int32)")
  if dev.type == "cuda":
    from corenet_amd.backend import default_backend
    default_backend().point_triangle(p, p_off.to(dev), tri, t_off.to(dev), max_np, max_nt, dist2, index)
  else:
    _lib().crn_point_triangle_cpu(p.data_ptr(), p_off.data_ptr(), tri.data_ptr(), t_off.data_ptr(), N, dist2.data_ptr(),
                                  index.data_ptr(), t.get_num_threads())
  return dist2, index


def _point_triangle_args(points, p_offsets, triangles, t_offsets, what: str):
  p, tri = _points(points, what + ": points"), _triangles(triangles, what + ": triangles")
  if p.device != tri.device:
    raise ValueError(f"{what}: the points are on {p.device}, the triangles on {tri.device}")
  _device_kind(p.device, what)
  p_off = _host_offsets(p_offsets, p.shape[0], what + ": points")
  t_off = _host_offsets(t_offsets, tri.shape[0], what + ": triangles")
  if p_off.numel() != t_off.numel():
    raise ValueError(f"{what}: {p_off.numel() - 1} objects of queries, {t_off.numel() - 1} of triangles")
  return p, p_off, tri, t_off


def point_triangle_distances(points, p_offsets, triangles, t_offsets) -> Tuple[t.Tensor, t.Tensor]:
  """For every query of points f32 [Np, 3] the nearest eligible triangle of the SAME object of triangles f32 [T, 3, 3]:
  (dist2 f32 [Np], index i32 [Np], local to the object).  Brute force and deterministic (see the module docstring)."""
  return _point_triangle(*_point_triangle_args(points, p_offsets, triangles, t_offsets, "point_triangle_distances"))


def _unit_normals(tri: t.Tensor) -> t.Tensor:
  """f64 [T, 3]: the unit normals of float32 triangles, elementwise in float64 (no fused kernel: the same on any device)."""
  v = tri.to(t.float64)
  a, b = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
  n = t.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
               a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
  return n / (n * n).sum(1, keepdim=True).sqrt()


def _normal_agreement(src_tri: t.Tensor, src_off: t.Tensor, src_index: t.Tensor, s_off: t.Tensor, near_tri: t.Tensor,
                      near_off: t.Tensor, near_index: t.Tensor) -> t.Tensor:
  """f64 [P]: |n_src . n_near| per sample; 0 where the sample found no triangle.  src_index / near_index are local to
  the object, s_off the samples' offsets (host)."""
  dev, N, P = src_index.device, s_off.numel() - 1, src_index.shape[0]
  if P == 0:
    return t.zeros(0, dtype=t.float64, device=dev)
  # the owner of every sample, built on the samples' device from the small offset tensors: nothing of size P crosses
  owner = t.repeat_interleave(t.arange(N, device=dev), (s_off[1:] - s_off[:-1]).to(dev), output_size=P)
  found = near_index >= 0
  i_src = src_index.to(t.int64) + src_off.to(dev)[owner]
  i_near = t.where(found, near_index.to(t.int64) + near_off.to(dev)[owner], t.zeros_like(i_src))
  if near_tri.shape[0] == 0:
    return t.zeros(P, dtype=t.float64, device=dev)
  dot = (_unit_normals(src_tri[i_src]) * _unit_normals(near_tri[i_near])).sum(1).abs()
  return t.where(found, dot, t.zeros_like(dot))


def mesh_chamfer_fscore(pred_triangles, pred_offsets, gt_triangles, gt_offsets, thresholds: Sequence[float],
                        num_samples: int = 16384, seed: int = 0) -> MeshSurfaceMetrics:
  """Chamfer distance, F-score and normal consistency of N predicted against N ground-truth triangle soups, one row per
  object, measured from area-weighted samples of one mesh to the TRIANGLES of the other: no sampling floor, and the same
  surface in another tessellation scores 0 up to float32 rounding.

  pred_triangles f32 [Tp, 3, 3] / gt_triangles f32 [Tg, 3, 3] with their offsets [N + 1]; thresholds: K distances.  Two
  sampling calls (num_samples per object, the same seed), two point-to-triangle calls, the reductions of chamfer_fscore;
  two runs agree bit for bit.  All fields are on the triangles' device."""
  what = "mesh_chamfer_fscore"
  pred, gt = _triangles(pred_triangles, what + ": pred"), _triangles(gt_triangles, what + ": gt")
  if pred.device != gt.device:
    raise ValueError(f"{what}: pred is on {pred.device}, gt on {gt.device}")
  dev = pred.device
  _device_kind(dev, what)
  pt_off = _host_offsets(pred_offsets, pred.shape[0], what + ": pred")
  gt_off = _host_offsets(gt_offsets, gt.shape[0], what + ": gt")
  if pt_off.numel() != gt_off.numel():
    raise ValueError(f"{what}: {pt_off.numel() - 1} predicted objects, {gt_off.numel() - 1} of ground truth")
  tau2 = _thresholds(thresholds, what)
  S = int(num_samples)

  def side(tri, off):
    """samples of the valid objects, packed: (points [P, 3], tri_index [P], offsets [N + 1] on the host)"""
    s = sample_surface_points(tri, num_samples=num_samples, seed=seed, offsets=off)
    valid = s.valid.cpu()
    s_off = t.cat([t.zeros(1, dtype=t.int64), t.cumsum(valid.to(t.int64) * S, 0)])
    if bool(valid.all()):
      return s.points.reshape(-1, 3), s.tri_index.reshape(-1), s_off
    keep = valid.nonzero()[:, 0].to(dev)
    return s.points[keep].reshape(-1, 3), s.tri_index[keep].reshape(-1), s_off

  p_pts, p_src, p_off = side(pred, pt_off)
  g_pts, g_src, g_off = side(gt, gt_off)
  d2_pg, i_pg = _point_triangle(p_pts, p_off, gt, gt_off)
  d2_gp, i_gp = _point_triangle(g_pts, g_off, pred, pt_off)
  m = _metrics_of(d2_pg, p_off, d2_gp, g_off, tau2)
  nc_p, = _segment_sums(p_off, dev, _normal_agreement(pred, pt_off, p_src, p_off, gt, gt_off, i_pg))
  nc_g, = _segment_sums(g_off, dev, _normal_agreement(gt, gt_off, g_src, g_off, pred, pt_off, i_gp))
  nc_p = nc_p / m.num_pred.clamp(min=1).to(t.float64)                         # no samples on this side: 0 ...
  nc_g = nc_g / m.num_gt.clamp(min=1).to(t.float64)
  both_empty = (m.num_pred == 0) & (m.num_gt == 0)                            # ... unless both are empty: NaN
  nan = t.full_like(nc_p, float("nan"))
  nc_p, nc_g = t.where(both_empty, nan, nc_p), t.where(both_empty, nan, nc_g)
  return MeshSurfaceMetrics(*m, (nc_p + nc_g) / 2, nc_p, nc_g)
