"""Exact Euclidean distance transform of voxel grids: distances to a set of voxels, signed distance fields, Euclidean
dilation / erosion, and a Chamfer / F-score measure at voxel resolution that needs no mesh and no seed.

One call transforms N grids: CUDA(HIP) tensors run the kernels of csrc/voxel_distance.hip, CPU tensors the library's host
twin (csrc/voxel_distance_cpu.cpp).  Both give the same tensors exactly; a CUDA tensor never goes to the host twin.

Contract:
  * grid: [N, D, H, W], N independent grids; W stride 1 (a view with another W stride is copied first), N / D / H strides
    arbitrary, so `labels[:, k]` views need no copy.  Rank other than 4 raises ValueError, so does an empty extent --
    except that N == 0 returns empty results --, D*H*W > 2^31 - 1 and (D-1)^2 + (H-1)^2 + (W-1)^2 >= 2^31 - 1 (the
    squared distances are int32).
  * Foreground: a voxel is foreground iff its value is > 0 (NaN is not).  The library takes uint8 and int32 grids: bool
    and floating grids are converted to a uint8 mask (v > 0), other integer types to int32.
  * target: "foreground" (value > 0), "background" (every other voxel) or "surface" (the foreground voxels with at least
    one of their 6 neighbours not foreground or outside the grid).
  * d2: int32 [N, D, H, W], min over the target voxels u of |v - u|^2 in voxel units, exact.  index: int32, the per-grid
    linear index d*H*W + h*W + w of the target voxel that attains it, defined by the separable recurrence (nearest target
    of the row, ties to the lower w; then the best row along h, then along d, ties to the lower one), so it is identical
    between GPU and host twin.  A grid without a target voxel gives d2 = NO_TARGET (2^31 - 1) and index = -1 everywhere.
  * Nothing depends on crn_set_deterministic; everything is queued on the current stream.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional, Sequence, Tuple

import torch as t

from corenet_amd.voxel_components import _prepare

NO_TARGET = (1 << 31) - 1
_MODES = {"foreground": 0, "background": 1, "surface": 2}


class SquaredDistance(NamedTuple):
  d2: t.Tensor                # i32 [N, D, H, W]
  index: Optional[t.Tensor]   # i32 [N, D, H, W] (None unless asked for)


def _lib():
  from corenet_amd import _lib as L
  return L.lib()


def distance_tiles() -> Tuple[int, int, int]:
  """(R, capacity, pack_bits) of the line passes: a lane keeps R outputs in registers; lines of up to `capacity`
  elements are staged in LDS, longer ones are read from global memory; with the index a pass packs value and row into
  one word where (bound + 1) << ceil(log2(line length)) <= 2^pack_bits, bound being the largest value it can produce
  (the sum of (extent - 1)^2 over w, h and, for the d pass, d)."""
  out = (C.c_int32 * 3)()
  _lib().crn_voxel_distance_tiles(C.addressof(out))
  return int(out[0]), int(out[1]), int(out[2])


def _check_shape(grid: t.Tensor, what: str):
  if grid.dim() != 4:
    raise ValueError(f"{what} expects a rank-4 grid [N, D, H, W], got shape {tuple(grid.shape)}")
  N, D, H, W = grid.shape
  if D == 0 or H == 0 or W == 0:
    if N:
      raise ValueError(f"{what}: empty grid extent {tuple(grid.shape)}")
    return
  if D * H * W > NO_TARGET:
    raise ValueError(f"{what}: grid of {D}x{H}x{W} too large (at most 2^31 - 1 voxels per grid)")
  if (D - 1) ** 2 + (H - 1) ** 2 + (W - 1) ** 2 >= NO_TARGET:
    raise ValueError(f"{what}: the squared diagonal of a {D}x{H}x{W} grid does not fit int32")


def squared_distance_to(grid, target: str = "foreground", return_index: bool = False) -> SquaredDistance:
  """The exact squared distance of every voxel to the nearest `target` voxel of its grid, and with return_index the
  linear index of that voxel (see the module docstring).  Nothing synchronises."""
  grid = t.as_tensor(grid)
  if target not in _MODES:
    raise ValueError(f"squared_distance_to: target must be one of {sorted(_MODES)}, got {target!r}")
  _check_shape(grid, "squared_distance_to")
  N, D, H, W = grid.shape
  dev = grid.device
  if dev.type not in ("cuda", "cpu"):
    raise ValueError(f"squared_distance_to: unsupported device {dev}")
  d2 = t.empty((N, D, H, W), dtype=t.int32, device=dev)
  index = t.empty((N, D, H, W), dtype=t.int32, device=dev) if return_index else None
  if N == 0:
    return SquaredDistance(d2, index)
  grid = _prepare(grid)
  if grid.is_cuda:
    from corenet_amd.backend import default_backend
    default_backend().voxel_distance(grid, _MODES[target], d2, index)
  else:
    from corenet_amd.backend import _DTYPE_CODE
    st = (C.c_int64 * 4)(*grid.stride())
    _lib().crn_voxel_distance_cpu(grid.data_ptr(), st, _DTYPE_CODE[grid.dtype], N, D, H, W, _MODES[target], d2.data_ptr(),
                                  None if index is None else index.data_ptr(), t.get_num_threads())
  return SquaredDistance(d2, index)


def _sqrt(d2: t.Tensor) -> t.Tensor:
  d = d2.to(t.float64).sqrt().to(t.float32)     # float64 sqrt is correctly rounded on either device: the same bits
  return t.where(d2 == NO_TARGET, t.full_like(d, float("inf")), d)


def distance_to(grid, target: str = "foreground") -> t.Tensor:
  """float32 [N, D, H, W]: the Euclidean distance (voxel units) to the nearest `target` voxel; +inf in a grid without one."""
  return _sqrt(squared_distance_to(grid, target).d2)


def signed_distance(occupancy) -> t.Tensor:
  """float32 distance_to(occupancy, "foreground") - distance_to(occupancy, "background"): positive outside (the distance
  to the nearest occupied voxel), negative inside (minus the distance to the nearest free voxel); its magnitude is at
  least 1 everywhere, the surface lies between the voxels of either sign.  Outside the grid is neither: a grid that is
  all outside (no occupied voxel) gives +inf everywhere, a grid that is all inside gives -inf everywhere."""
  return distance_to(occupancy, "foreground") - distance_to(occupancy, "background")


def _radius2(radius: float, what: str) -> int:
  r = float(radius)
  if not (r >= 0) or math.isinf(r):
    raise ValueError(f"{what}: radius must be finite and >= 0, got {radius}")
  return min(int(math.floor(r * r)), NO_TARGET - 1)


def dilate(mask, radius: float) -> t.Tensor:
  """bool: the voxels within `radius` (Euclidean, voxel units) of a foreground voxel -- scipy's binary_dilation with the
  ball x^2 + y^2 + z^2 <= radius^2."""
  return squared_distance_to(mask, "foreground").d2 <= _radius2(radius, "dilate")


def erode(mask, radius: float) -> t.Tensor:
  """bool: the voxels farther than `radius` from every voxel that is not foreground.  Outside the grid is neither
  foreground nor background, so a grid border does not erode: scipy's binary_erosion(border_value=1) with the ball."""
  return squared_distance_to(mask, "background").d2 > _radius2(radius, "erode")


def surface_voxels(mask) -> t.Tensor:
  """bool: the foreground voxels with at least one of their 6 neighbours not foreground or outside the grid."""
  return squared_distance_to(mask, "surface").d2 == 0


def voxel_surface_metrics(pred, gt, thresholds: Sequence[float], voxel_size=1.0):
  """Chamfer distance and F-score between the voxel surfaces of N pairs of grids -> mesh_metrics.SurfaceMetrics, with
  the fields and conventions of chamfer_fscore: the "points" of a side are its surface voxels (in raster order), the
  distance of a point is the exact distance to the nearest surface voxel of the other side, times voxel_size (a scalar
  or [N]; thresholds are in the same unit).  A pair without a surface on either side gives NaN, with a surface on one
  side only Chamfer +inf and F-score 0.  Two library calls, no marching cubes, no sampling, no seed; the gathers of the
  surface voxels (nonzero) and the read of their per-grid counts synchronise."""
  from corenet_amd import mesh_metrics
  pred, gt = t.as_tensor(pred), t.as_tensor(gt)
  if pred.dim() != 4 or tuple(pred.shape) != tuple(gt.shape) or pred.device != gt.device:
    raise ValueError(f"voxel_surface_metrics: pred and gt must be [N, D, H, W] grids of one shape on one device, got "
                     f"{tuple(pred.shape)} on {pred.device} and {tuple(gt.shape)} on {gt.device}")
  tau2 = mesh_metrics._thresholds(thresholds, "voxel_surface_metrics")
  N, dev = pred.shape[0], pred.device
  vs = t.as_tensor(voxel_size, dtype=t.float32).to(dev)
  if vs.dim() > 1 or (vs.dim() == 1 and vs.numel() != N):
    raise ValueError(f"voxel_surface_metrics: voxel_size must be a scalar or [N], got {tuple(vs.shape)}")
  vs2 = (vs * vs).expand(N) if vs.dim() == 0 else vs * vs
  to_p = squared_distance_to(pred, "surface").d2.reshape(N, -1)
  to_g = squared_distance_to(gt, "surface").d2.reshape(N, -1)

  def side(own, other):
    on = own == 0                                                           # this side's surface voxels
    cnt = on.sum(1)
    grid_of, voxel = on.nonzero(as_tuple=True)                              # raster order, grid by grid
    d2 = other[grid_of, voxel]
    d2f = t.where(d2 == NO_TARGET, t.full((), float("inf"), device=dev), d2.to(t.float32) * vs2[grid_of])
    return d2f, cnt
  d2_pg, np_ = side(to_p, to_g)
  d2_gp, ng = side(to_g, to_p)
  cnt = t.stack([np_, ng]).cpu()
  zero = t.zeros(1, dtype=t.int64)
  p_off, g_off = t.cat([zero, t.cumsum(cnt[0], 0)]), t.cat([zero, t.cumsum(cnt[1], 0)])
  return mesh_metrics._metrics_of(d2_pg, p_off, d2_gp, g_off, tau2)
