"""Voxel visibility from the camera: which voxels of a grid an eye can see, which occupied voxel hides the others, and
the IoU of a reconstruction split into its seen and its hidden part.

One call handles N grids: CUDA(HIP) tensors run the kernels of csrc/voxel_visibility.hip, CPU tensors the library's host
twin (csrc/voxel_visibility_cpu.cpp).  Both give the same tensors exactly; a CUDA tensor never goes to the host twin.

Contract, exact and in integers:
  * grid: [N, D, H, W], N independent grids, with the strides and dtypes of voxel_distance.squared_distance_to: W
    stride 1 (a view with another W stride is copied first), N / D / H strides arbitrary; a voxel is occupied iff its
    value is > 0 (NaN is not).  Rank other than 4 raises ValueError, so does an empty extent -- except that N == 0 returns
    empty results --, an extent above MAX_EXTENT (2048) and D*H*W > 2^31 - 1 (`first` is int32).
  * Space is measured in 1 / EYE_SUBDIVISIONS (256) of a voxel.  Voxel (x, y, z) = index [z, y, x] is the cube
    [256x, 256x + 256] x [256y, 256y + 256] x [256z, 256z + 256], its centre c = (256x + 128, 256y + 128, 256z + 128).
  * eye: [N, 3] or [3] (broadcast over the grids), (x, y, z) in float voxel coordinates; it is quantised on the host to
    int32 round(eye * 256) in float64, half to even.  ValueError: another shape, a non-finite value, a coordinate beyond
    +-MAX_EYE / 256 = 2048 voxels.  A CUDA `eye` costs one synchronisation (its copy to the host); nothing else synchronises.
  * The traversed set of a voxel v: every voxel u != v of the grid whose open interior meets the open segment from c(v)
    to the eye.  Centres sit at 128 mod 256, so every tie is settled by this definition: a segment through an edge or a
    corner enters the voxel diagonally across it and not the voxels it merely touches.
  * occluded: bool [N, D, H, W], true iff a traversed voxel is occupied.  first: int32, the per-grid linear index
    z*H*W + y*W + x of the occupied traversed voxel nearest the eye, -1 where there is none.  v's own content does not
    matter: free voxels have a visibility too.
  * Nothing depends on crn_set_deterministic; everything is queued on the current stream.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import torch as t

from corenet_amd.voxel_components import _prepare

EYE_SUBDIVISIONS = 256
MAX_EXTENT = 2048
MAX_EYE = 1 << 19                 # sub-units: 2048 voxels
FLAT = 1                          # flags bit 0: the GPU reads the fine occupancy bits only (no coarse map)
_COUNT_STEPS = 2                  # host twin: `first` receives every voxel's trip count (tools/bench_visibility.py)
_MAX_VOXELS = (1 << 31) - 1


class Occlusion(NamedTuple):
  occluded: t.Tensor          # bool [N, D, H, W]
  first: Optional[t.Tensor]   # i32 [N, D, H, W] (None unless asked for)


class VisibilityIoU(NamedTuple):
  intersection: t.Tensor      # i64 [N, 2]: column 0 the voxels the occluder does not hide, column 1 the rest
  union: t.Tensor             # i64 [N, 2]
  region_voxels: t.Tensor     # i64 [N, 2]
  iou: t.Tensor               # f64 [N, 2], NaN where the union is 0


def _lib():
  from corenet_amd import _lib as L
  return L.lib()


def visibility_tiles() -> Tuple[int, int, int]:
  """(brick, coarse_capacity_bytes, workgroup_words): the coarse map holds one bit per brick^3 voxels and is staged in
  LDS when it takes at most coarse_capacity_bytes per grid (otherwise, or with FLAT, the flat form runs); a workgroup of
  the walk pass owns workgroup_words consecutive 64-voxel words of a grid."""
  out = (C.c_int32 * 3)()
  _lib().crn_voxel_visibility_tiles(C.addressof(out))
  return int(out[0]), int(out[1]), int(out[2])


def _check_shape(grid: t.Tensor, what: str):
  if grid.dim() != 4:
    raise ValueError(f"{what} expects a rank-4 grid [N, D, H, W], got shape {tuple(grid.shape)}")
  N, D, H, W = grid.shape
  if D == 0 or H == 0 or W == 0:
    if N:
      raise ValueError(f"{what}: empty grid extent {tuple(grid.shape)}")
    return
  if max(D, H, W) > MAX_EXTENT:
    raise ValueError(f"{what}: grid of {D}x{H}x{W} too large (every extent at most {MAX_EXTENT})")
  if D * H * W > _MAX_VOXELS:
    raise ValueError(f"{what}: grid of {D}x{H}x{W} too large (at most 2^31 - 1 voxels per grid)")


def quantise_eye(eye, N: int, what: str = "quantise_eye") -> t.Tensor:
  """int32 [N, 3] on the host: round(eye * 256), half to even, after the checks of the module docstring."""
  e = t.as_tensor(eye).detach()
  if e.dim() not in (1, 2) or e.shape[-1] != 3 or (e.dim() == 2 and e.shape[0] != N):
    raise ValueError(f"{what}: eye must be [3] or [{N}, 3], got {tuple(e.shape)}")
  e = e.cpu().to(t.float64)                                   # a CUDA eye: the call's one synchronisation
  if not bool(t.isfinite(e).all()):
    raise ValueError(f"{what}: eye must be finite, got {e.tolist()}")
  q = t.round(e * EYE_SUBDIVISIONS)
  if bool((q.abs() > MAX_EYE).any()):
    raise ValueError(f"{what}: eye beyond {MAX_EYE // EYE_SUBDIVISIONS} voxels from the origin: {e.tolist()}")
  return q.to(t.int32).expand(N, 3).contiguous()


def _run(grid: t.Tensor, eye_q: t.Tensor, flags: int, want_first: bool) -> Occlusion:
  N, D, H, W = grid.shape
  dev = grid.device
  occluded = t.empty((N, D, H, W), dtype=t.bool, device=dev)
  first = t.empty((N, D, H, W), dtype=t.int32, device=dev) if want_first else None
  if N == 0:
    return Occlusion(occluded, first)
  grid = _prepare(grid)
  if grid.is_cuda:
    from corenet_amd.backend import default_backend
    default_backend().voxel_visibility(grid, eye_q, flags, occluded, first)
  else:
    from corenet_amd.backend import _DTYPE_CODE
    st = (C.c_int64 * 4)(*grid.stride())
    _lib().crn_voxel_visibility_cpu(grid.data_ptr(), st, _DTYPE_CODE[grid.dtype], N, D, H, W, eye_q.data_ptr(), flags,
                                    occluded.data_ptr(), None if first is None else first.data_ptr(), t.get_num_threads())
  return Occlusion(occluded, first)


def occlusion(grid, eye, return_first: bool = False, flags: int = 0) -> Occlusion:
  """Whether an occupied voxel of its grid lies between every voxel and the eye, and with return_first which one is
  nearest the eye (see the module docstring).  flags: 0, or FLAT to make the GPU skip its coarse map (same results)."""
  grid = t.as_tensor(grid)
  _check_shape(grid, "occlusion")
  if flags not in (0, FLAT):
    raise ValueError(f"occlusion: flags must be 0 or FLAT, got {flags}")
  if grid.device.type not in ("cuda", "cpu"):
    raise ValueError(f"occlusion: unsupported device {grid.device}")
  return _run(grid, quantise_eye(eye, grid.shape[0], "occlusion"), flags, bool(return_first))


def walk_steps(grid, eye) -> t.Tensor:
  """int32 [N, D, H, W], host grids only: the trip count of every voxel's walk to the grid boundary or the eye, the
  work of occlusion(..., return_first=True).  The host twin counts it."""
  grid = t.as_tensor(grid)
  _check_shape(grid, "walk_steps")
  if grid.device.type != "cpu":
    raise ValueError("walk_steps: the host twin counts; pass a CPU grid")
  return _run(grid, quantise_eye(eye, grid.shape[0], "walk_steps"), _COUNT_STEPS, True).first


def visible(grid, eye) -> t.Tensor:
  """bool [N, D, H, W]: the voxels, free or occupied, that no occupied voxel hides from the eye."""
  return ~occlusion(grid, eye).occluded


def visible_surface(grid, eye) -> t.Tensor:
  """bool [N, D, H, W]: the occupied voxels the eye sees."""
  grid = t.as_tensor(grid)
  return (grid > 0) & ~occlusion(grid, eye).occluded


def eye_in_voxel_space(camera_transform, view_to_voxel) -> t.Tensor:
  """float64 [N, 3] on the host: the centre of projection of camera_transform ([N, 4, 4] or [4, 4], column vectors) in
  voxel coordinates, view_to_voxel @ inverse(camera_transform) @ (0, 0, 1, 0) dehomogenised, in float64.  ValueError if
  that is not finite or beyond the range of `occlusion` -- an orthographic camera has its eye at infinity."""
  cam = t.as_tensor(camera_transform).detach().cpu().to(t.float64)
  v2x = t.as_tensor(view_to_voxel).detach().cpu().to(t.float64)
  if cam.dim() == 2:
    cam = cam[None]
  if v2x.dim() == 2:
    v2x = v2x[None]
  if cam.dim() != 3 or v2x.dim() != 3 or cam.shape[1:] != (4, 4) or v2x.shape[1:] != (4, 4):
    raise ValueError(f"eye_in_voxel_space: expected [N, 4, 4] matrices, got {tuple(cam.shape)} and {tuple(v2x.shape)}")
  N = max(cam.shape[0], v2x.shape[0])
  if cam.shape[0] not in (1, N) or v2x.shape[0] not in (1, N):
    raise ValueError(f"eye_in_voxel_space: batch sizes {cam.shape[0]} and {v2x.shape[0]} do not broadcast")
  try:
    inv = t.linalg.inv(cam)
  except RuntimeError as e:
    raise ValueError(f"eye_in_voxel_space: camera_transform is singular ({e})")
  h = (v2x @ inv)[..., 2].expand(N, 4)                        # the third column: the image of (0, 0, 1, 0)
  with_w = h[:, :3] / h[:, 3:4]
  if not bool(t.isfinite(with_w).all()) or bool((t.round(with_w * EYE_SUBDIVISIONS).abs() > MAX_EYE).any()):
    raise ValueError(f"eye_in_voxel_space: the eye is not a finite point within {MAX_EYE // EYE_SUBDIVISIONS} voxels "
                     f"(homogeneous {h.tolist()}); an orthographic camera has none")
  return with_w.contiguous()


def visibility_iou(pred, gt, eye, occluder=None) -> VisibilityIoU:
  """The IoU of N pairs of grids (occupied iff > 0) split by what `occluder` (default gt) hides from the eye: column 0
  counts the voxels it does not occlude, column 1 the rest; the columns add up to the plain intersection and union.  iou
  is NaN where the union is 0.  A few torch ops on one occlusion call."""
  pred, gt = t.as_tensor(pred), t.as_tensor(gt)
  occ = gt if occluder is None else t.as_tensor(occluder)
  if pred.dim() != 4 or tuple(pred.shape) != tuple(gt.shape) or tuple(occ.shape) != tuple(gt.shape) or \
      pred.device != gt.device or occ.device != gt.device:
    raise ValueError(f"visibility_iou: pred, gt and occluder must be [N, D, H, W] grids of one shape on one device, got "
                     f"{tuple(pred.shape)} on {pred.device}, {tuple(gt.shape)} on {gt.device}, {tuple(occ.shape)} on {occ.device}")
  return _split_iou(pred > 0, gt > 0, occlusion(occ, eye).occluded)


def _split_iou(p: t.Tensor, g: t.Tensor, hidden: t.Tensor) -> VisibilityIoU:
  """VisibilityIoU of the bool grids p, g [N, D, H, W] split by the bool mask hidden [N, D, H, W]."""
  N = p.shape[0]
  p, g, hidden = p.reshape(N, -1), g.reshape(N, -1), hidden.reshape(N, -1)

  def split(x):
    total, back = x.sum(1), (x & hidden).sum(1)
    return t.stack([total - back, back], 1)
  inter, union, region = split(p & g), split(p | g), split(t.ones_like(hidden))
  iou = t.where(union > 0, inter.to(t.float64) / union.to(t.float64), t.full((), float("nan"), dtype=t.float64, device=p.device))
  return VisibilityIoU(inter, union, region, iou)
