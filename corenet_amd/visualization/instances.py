"""One marching-cubes mesh per connected object of a semantic label grid (corenet_amd.voxel_components + marching_cubes)."""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch as t

from corenet_amd.visualization.marching_cubes import Meshes, marching_cubes
from corenet_amd.voxel_components import component_stats, connected_components

_MASK_CHUNK_BYTES = 1 << 30


class InstanceTable(NamedTuple):
  """One row per instance, in the order of the meshes: by grid, then by component number (raster order of the lowest
  voxel)."""
  grid_index: t.Tensor     # i64 [M], host
  value: t.Tensor          # i32 [M] the instance's class (the label grid's value)
  size: t.Tensor           # i64 [M] voxels
  bbox: t.Tensor           # i32 [M, 6] (d0, h0, w0, d1, h1, w1), upper bounds exclusive


def instance_meshes(label_grid, matrices: Optional[t.Tensor] = None, min_voxels: int = 1, connectivity: int = 6,
                    level: float = 0.5) -> Tuple[Meshes, InstanceTable]:
  """Meshes of the instances of label_grid [N, D, H, W]: the connected components (by value, so two touching objects of
  different classes stay apart) with at least min_voxels voxels.  Every instance is meshed from its full-size float32
  mask, so coordinates stay in the padded index space of the whole grid and instance meshes line up with the class
  meshes of marching_cubes(label_grid == k).  matrices: None, [4, 4] or per grid [N, 4, 4]; expanded per instance.
  Masks are built for chunks of instances of at most 1 GiB."""
  label_grid = t.as_tensor(label_grid)
  comps = connected_components(label_grid, connectivity, by_value=True)
  stats = component_stats(comps, label_grid)
  N, D, H, W = comps.labels.shape
  dev = comps.labels.device
  counts = stats.offsets[1:] - stats.offsets[:-1]
  grid_index = t.repeat_interleave(t.arange(N), counts)
  number = t.arange(int(stats.offsets[-1])) - stats.offsets[:-1][grid_index] + 1
  keep = (stats.size >= int(min_voxels)).cpu()
  grid_index, number = grid_index[keep], number[keep]
  sel = keep.nonzero()[:, 0].to(dev)
  table = InstanceTable(grid_index, stats.value[sel], stats.size[sel], stats.bbox[sel])
  if matrices is not None:
    matrices = t.as_tensor(matrices, dtype=t.float32, device=dev)
    if matrices.shape == (4, 4):
      matrices = matrices.expand(N, 4, 4)
    if tuple(matrices.shape) != (N, 4, 4):
      raise ValueError(f"instance_meshes: matrices must be [N, 4, 4] or [4, 4], got {tuple(matrices.shape)}")
  M = grid_index.numel()
  per_chunk = max(1, _MASK_CHUNK_BYTES // (4 * D * H * W)) if M else 1
  parts = []
  for i in range(0, M, per_chunk):
    gi = grid_index[i:i + per_chunk].to(dev)
    ids = number[i:i + per_chunk].to(dev, t.int32)
    masks = (comps.labels[gi] == ids[:, None, None, None]).to(t.float32)
    parts.append(marching_cubes(masks, level=level, matrices=None if matrices is None else matrices[gi]))
  if not parts:
    f32 = t.empty((0, 3), dtype=t.float32, device=dev)
    i64 = t.empty((0,), dtype=t.int64, device=dev)
    return Meshes(f32, f32.clone(), t.empty((0, 3), dtype=t.int32, device=dev), i64, i64.clone()), table
  return Meshes(*[t.cat([p[f] for p in parts]) for f in range(5)]), table
