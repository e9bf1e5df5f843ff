"""Connected components of voxel grids: instances of a semantic label grid, floater removal for predictions.

One call labels N grids: CUDA(HIP) tensors run the kernels of csrc/voxel_components.hip, CPU tensors the library's host
twin (csrc/voxel_components_cpu.cpp).  Both give the same tensors exactly; a CUDA tensor never goes to the host twin.

Contract:
  * grid: [N, D, H, W], N independent grids; W stride 1 (a view with another W stride is copied first), N / D / H strides
    arbitrary, so `labels[:, k]` views need no copy.  Rank other than 4 raises ValueError, so does an empty extent --
    except that N == 0 returns empty results -- and D*H*W > 2^31 - 1 (labels and parents are 32-bit per grid).
  * Foreground: a voxel is foreground iff its value is > 0 (the rule of fill_voxels; NaN is background).  The library
    takes uint8 and int32 grids: bool and floating grids are converted to a uint8 mask (v > 0), other integer types to
    int32 -- their values must fit int32 (values beyond it wrap, as torch's conversion does).
  * connectivity: 6 (faces), 18 (plus edges) or 26 (plus corners); anything else raises ValueError.
  * by_value=True: two neighbouring foreground voxels belong together only if their values are equal (instances per
    class of a semantic label grid; after the conversion above, so a floating grid has one value).  False: any two
    neighbouring foreground voxels belong together.
  * labels: int32 [N, D, H, W], contiguous, on the grid's device; 0 on background; the components of grid n are numbered
    1 .. K_n in ascending order of their lowest linear index d*H*W + h*W + w -- for binary input exactly
    scipy.ndimage.label's numbering.  num_components: int64 [N].
  * The result is a function of the partition alone: identical from run to run and between GPU and host twin; nothing
    depends on crn_set_deterministic.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import torch as t

_MAX_VOXELS = (1 << 31) - 1


class Components(NamedTuple):
  labels: t.Tensor            # i32 [N, D, H, W]
  num_components: t.Tensor    # i64 [N]


class ComponentStats(NamedTuple):
  offsets: t.Tensor           # i64 [N + 1] on the host: component c of grid n is row offsets[n] + c - 1 (CSR over grids)
  size: t.Tensor              # i64 [K] voxels per component
  bbox: t.Tensor              # i32 [K, 6] (d0, h0, w0, d1, h1, w1), upper bounds exclusive
  first: t.Tensor             # i64 [K] lowest linear index
  value: Optional[t.Tensor]   # i32 [K] the grid's value at `first` (None unless a grid was given)


def _lib():
  from corenet_amd import _lib as L
  return L.lib()


def component_bricks() -> Tuple[int, int, int]:
  """The kernel's brick extents (bd, bh, bw): a workgroup labels one brick in LDS, seams between bricks are united on
  the global parent array."""
  out = (C.c_int32 * 3)()
  _lib().crn_voxel_components_bricks(C.addressof(out))
  return int(out[0]), int(out[1]), int(out[2])


def _check_shape(grid: t.Tensor, what: str):
  if grid.dim() != 4:
    raise ValueError(f"{what} expects a rank-4 grid [N, D, H, W], got shape {tuple(grid.shape)}")
  N, D, H, W = grid.shape
  if N and (D == 0 or H == 0 or W == 0):
    raise ValueError(f"{what}: empty grid extent {tuple(grid.shape)}")
  if D * H * W > _MAX_VOXELS:
    raise ValueError(f"{what}: grid of {D}x{H}x{W} too large (at most 2^31 - 1 voxels per grid)")


def _prepare(grid: t.Tensor) -> t.Tensor:
  """The uint8 / int32 tensor with W stride 1 the library takes."""
  if grid.dtype == t.bool or grid.dtype.is_floating_point:
    grid = (grid > 0).to(t.uint8)
  elif grid.dtype not in (t.uint8, t.int32):
    grid = grid.to(t.int32)
  if grid.stride(-1) != 1:
    grid = grid.contiguous()
  return grid


def _check_connectivity(connectivity):
  if connectivity not in (6, 18, 26):
    raise ValueError(f"connectivity must be 6, 18 or 26, got {connectivity}")


def connected_components(grid, connectivity: int = 6, by_value: bool = True) -> Components:
  """Labels the connected components of N grids (see the module docstring for the contract).  Everything is queued on
  the current stream; nothing synchronises."""
  grid = t.as_tensor(grid)
  _check_shape(grid, "connected_components")
  _check_connectivity(connectivity)
  N, D, H, W = grid.shape
  dev = grid.device
  if dev.type not in ("cuda", "cpu"):
    raise ValueError(f"connected_components: unsupported device {dev}")
  labels = t.empty((N, D, H, W), dtype=t.int32, device=dev)
  num = t.empty((N,), dtype=t.int64, device=dev)
  if N == 0:
    return Components(labels, num)
  grid = _prepare(grid)
  if grid.is_cuda:
    from corenet_amd.backend import default_backend
    default_backend().voxel_components(grid, int(connectivity), bool(by_value), labels, num)
  else:
    from corenet_amd.backend import _DTYPE_CODE
    st = (C.c_int64 * 4)(*grid.stride())
    _lib().crn_voxel_components_cpu(grid.data_ptr(), st, _DTYPE_CODE[grid.dtype], N, D, H, W, int(connectivity),
                                    int(bool(by_value)), labels.data_ptr(), num.data_ptr(), t.get_num_threads())
  return Components(labels, num)


def component_stats(components: Components, grid=None) -> ComponentStats:
  """Size, bounding box and first voxel of every component, and with `grid` (the tensor that was labelled, or any grid
  of the same shape) its value there -- after the conversion of the module docstring, so 1 for bool and floating grids.

  On the GPU the call synchronises exactly once: one device-to-host read of num_components that sizes the outputs."""
  labels, num = components.labels, components.num_components
  if labels.dim() != 4 or labels.dtype != t.int32 or not labels.is_contiguous():
    raise ValueError("component_stats: labels must be a contiguous int32 [N, D, H, W] tensor")
  N, D, H, W = labels.shape
  dev = labels.device
  offsets = t.zeros((N + 1,), dtype=t.int64)
  offsets[1:] = t.cumsum(num.cpu(), 0)                                    # the call's one synchronisation
  K = int(offsets[N])
  size = t.empty((K,), dtype=t.int64, device=dev)
  bbox = t.empty((K, 6), dtype=t.int32, device=dev)
  first = t.empty((K,), dtype=t.int64, device=dev)
  value = None
  if grid is not None:
    grid = t.as_tensor(grid)
    if tuple(grid.shape) != tuple(labels.shape) or grid.device != dev:
      raise ValueError("component_stats: grid must have the labels' shape and device")
    grid = _prepare(grid)
    value = t.empty((K,), dtype=t.int32, device=dev)
  if K == 0 or N == 0:
    return ComponentStats(offsets, size, bbox, first, value)
  if labels.is_cuda:
    from corenet_amd.backend import default_backend
    default_backend().component_stats(labels, grid, offsets.to(dev, non_blocking=False), K, size, bbox, first, value)
  else:
    from corenet_amd.backend import _DTYPE_CODE
    st = None if grid is None else (C.c_int64 * 4)(*grid.stride())
    _lib().crn_component_stats_cpu(labels.data_ptr(), None if grid is None else grid.data_ptr(), st,
                                   0 if grid is None else _DTYPE_CODE[grid.dtype], N, D, H, W, offsets.data_ptr(), K,
                                   size.data_ptr(), bbox.data_ptr(), first.data_ptr(),
                                   None if value is None else value.data_ptr(), t.get_num_threads())
  return ComponentStats(offsets, size, bbox, first, value)


def _rank_in_group(size: t.Tensor, group: t.Tensor) -> t.Tensor:
  """Rank of every component among those of its group by size, largest first, ties to the lower component number."""
  K = size.numel()
  by_size = t.argsort(-size, stable=True)
  order = by_size[t.argsort(group[by_size], stable=True)]                 # groups together, each by (size desc, number)
  g = group[order]
  pos = t.arange(K, device=size.device)
  start = t.ones(K, dtype=t.bool, device=size.device)
  start[1:] = g[1:] != g[:-1]
  group_start = t.cummax(t.where(start, pos, t.zeros_like(pos)), 0).values
  rank = t.empty_like(pos)
  rank[order] = pos - group_start
  return rank


def filter_components(grid, min_voxels: int = 0, keep_largest: Optional[int] = None, connectivity: int = 6,
                      by_value: bool = True) -> t.Tensor:
  """A tensor of grid's dtype and shape with the voxels of removed components set to 0.  A component is removed if its
  size is below min_voxels; with keep_largest = k also unless it is among the k largest of its grid -- of its (grid,
  value) with by_value=True -- where ties go to the lower component number."""
  grid = t.as_tensor(grid)
  _check_shape(grid, "filter_components")
  _check_connectivity(connectivity)
  if keep_largest is not None and (int(keep_largest) != keep_largest or keep_largest < 0):
    raise ValueError(f"filter_components: keep_largest must be a non-negative integer or None, got {keep_largest}")
  if grid.shape[0] == 0:
    return grid.clone()
  comps = connected_components(grid, connectivity, by_value)
  stats = component_stats(comps, grid if by_value and keep_largest is not None else None)
  dev = grid.device
  N = grid.shape[0]
  K = stats.size.numel()
  keep = stats.size >= int(min_voxels)
  if keep_largest is not None and K:
    counts = (stats.offsets[1:] - stats.offsets[:-1]).to(dev)
    group = t.repeat_interleave(t.arange(N, device=dev), counts, output_size=K)
    if by_value:
      group = group * (1 << 32) + (stats.value.to(t.int64) & 0xffffffff)
    keep &= _rank_in_group(stats.size, group) < int(keep_largest)
  table = t.cat([t.zeros(1, dtype=t.bool, device=dev), keep])             # row 0: background
  out = t.empty(grid.shape, dtype=grid.dtype, device=dev)
  zero = t.zeros((), dtype=grid.dtype, device=dev)
  for n in range(N):                                                      # per grid: the int64 index is 8 B per voxel
    lab = comps.labels[n].to(t.int64)
    row = t.where(lab > 0, lab + int(stats.offsets[n]), lab)
    out[n] = t.where(table[row], grid[n], zero)
  return out
