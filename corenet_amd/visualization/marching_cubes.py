"""Marching-cubes meshes of predicted voxel grids (reference: MarchingCubesArtifact, visualization/artifacts.py:202-289).

The reference turns every predicted grid into a surface with `skimage.measure.marching_cubes` on the host, one object at
a time.  Here one call meshes N objects: CUDA(HIP) tensors run the kernels of csrc/marching_cubes.hip, CPU tensors the
library's host twin (csrc/marching_cubes_cpu.cpp).  Both give the same arrays bit for bit; a CUDA tensor never goes to
the host twin.

Contract:
  * grid: [N, D, H, W], N independent objects; W stride 1 (a view with another W stride is copied first), N / D / H
    strides arbitrary, so `pmf[:, 1:]` and `pmf[b, 1:]` need no copy.  Other dtypes are cast to float32.  Rank other
    than 4 or an empty extent raises ValueError.
  * Every object is padded by one zero voxel on every side; `level` (default 0.5) must be > 0 so that the padding closes
    every surface.  A corner is inside iff f > level (NaN and f == level are outside; NaN samples read as 0).
  * One vertex per grid edge whose endpoints straddle the level.  With f0 the sample at the endpoint with the lower index
    along the edge's axis and f1 the other, t = (level - f0) / (f1 - f0) and the coordinate along the axis is
    float(i0) + t (float32, no contraction); the other two are the grid positions.  Coordinates are in the padded index
    space with axes (x, y, z) = (w, h, d): grid[n, d, h, w] sits at (w + 1, h + 1, d + 1), as in the reference.
  * Normals: central differences of the padded (filtered) grid at both endpoints (one-sided on its border), interpolated
    with t, negated, normalised (sqrtf and a divide): they point from inside to outside; a zero gradient gives (0, 0, 0).
  * Faces: a 256-case table (tools/gen_mc_tables.py -> csrc/mc_tables.h) that never joins two diagonal inside corners of
    a face, so neighbouring cells agree and every surface is closed; triangles are counter-clockwise seen from outside.
  * Order: vertices by object, then owning grid point in raster order (d, h, w), then edge axis x < y < z; faces by
    object, then cell raster order, then table order.  Face indices are int32, local to their object.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch as t


class Meshes(NamedTuple):
  vertices: t.Tensor       # f32 [V, 3], (x, y, z) = (w, h, d) padded index space (or matrices applied)
  normals: t.Tensor        # f32 [V, 3]
  faces: t.Tensor          # i32 [F, 3], vertex ids local to the object
  num_vertices: t.Tensor   # i64 [N]
  num_faces: t.Tensor      # i64 [N]


def _as_grid(grid) -> t.Tensor:
  grid = t.as_tensor(grid)
  if grid.dim() != 4:
    raise ValueError(f"marching cubes expects a rank-4 grid [N, D, H, W], got shape {tuple(grid.shape)}")
  if any(s == 0 for s in grid.shape):
    raise ValueError(f"marching cubes: empty grid extent {tuple(grid.shape)}")
  if grid.dtype != t.float32:
    grid = grid.to(t.float32)
  if grid.stride(-1) != 1:
    grid = grid.contiguous()
  return grid


def _lib():
  from corenet_amd import _lib as L
  return L.lib()


def box_filter(grid, k: int) -> t.Tensor:
  """k^3 box mean of every object of `grid` [N, D, H, W] with the reference's zero padding [(k-1)//2, k-1-(k-1)//2]
  per axis (artifacts.py:225-229): a fresh contiguous float32 tensor on the grid's device (k == 1: a copy).
  Separable (w, then h, then d), each tap sum in ascending order, the last pass times 1/k^3 -- the same arithmetic on
  the GPU and the host twin."""
  grid = t.as_tensor(grid)
  if grid.dim() != 4:
    raise ValueError(f"box_filter expects a rank-4 grid [N, D, H, W], got shape {tuple(grid.shape)}")
  if int(k) != k or k < 1:
    raise ValueError(f"box_filter: kernel size must be a positive integer, got {k}")
  grid = grid.to(t.float32)
  out = t.empty(grid.shape, dtype=t.float32, device=grid.device)
  if grid.numel() == 0:
    return out
  N, D, H, W = grid.shape
  if grid.is_cuda:
    from corenet_amd.backend import default_backend
    default_backend().box_filter(grid, int(k), out)
  elif grid.device.type == "cpu":
    st = (C.c_int64 * 4)(*grid.stride())
    _lib().crn_box_filter_cpu(grid.data_ptr(), st, out.data_ptr(), N, D, H, W, int(k), t.get_num_threads())
  else:
    raise ValueError(f"box_filter: unsupported device {grid.device}")
  return out


def marching_cubes(grid, level: float = 0.5, filter_kernel: int = 1, matrices: Optional[t.Tensor] = None) -> Meshes:
  """Indexed meshes of the `level` surfaces of N objects, grid [N, D, H, W] (see the module docstring for the contract).

  filter_kernel = k > 1 smooths first: the result equals marching_cubes(box_filter(grid, k), level).  matrices: None or
  f32 [N, 4, 4] (or [4, 4] for all objects): positions are transformed as points with the homogeneous divide, normals as
  vectors (w = 0) without renormalising -- transform_mesh as MarchingCubesArtifact uses it (artifacts.py:234-235).

  On the GPU the call synchronises exactly once: one device-to-host read of the per-object (num_vertices, num_faces)
  that sizes the outputs.  Everything else is queued on the current stream."""
  grid = _as_grid(grid)
  level = float(level)
  if not level > 0:
    raise ValueError(f"marching cubes: level must be > 0 (the zero padding closes the surfaces only then), got {level}")
  if int(filter_kernel) != filter_kernel or filter_kernel < 1:
    raise ValueError(f"marching cubes: filter_kernel must be a positive integer, got {filter_kernel}")
  if filter_kernel > 1:
    grid = box_filter(grid, int(filter_kernel))
  N, D, H, W = grid.shape
  if (D + 1) * (H + 1) * (W + 1) > 1 << 29:
    raise ValueError(f"marching cubes: object of {D}x{H}x{W} too large (at most 2^29 cells per object)")
  dev = grid.device
  if matrices is not None:
    matrices = t.as_tensor(matrices, dtype=t.float32, device=dev)
    if matrices.shape == (4, 4):
      matrices = matrices.expand(N, 4, 4)
    if tuple(matrices.shape) != (N, 4, 4):
      raise ValueError(f"marching cubes: matrices must be [N, 4, 4] or [4, 4], got {tuple(matrices.shape)}")
    matrices = matrices.contiguous()
  if grid.is_cuda:
    from corenet_amd.backend import default_backend
    be = default_backend()
    counts = t.empty((N, 2), dtype=t.int64, device=dev)
    be.marching_cubes_count(grid, level, counts)
    host = counts.cpu()                                                    # the call's one synchronisation
    V, F = int(host[:, 0].sum()), int(host[:, 1].sum())
    vertices = t.empty((V, 3), dtype=t.float32, device=dev)
    normals = t.empty((V, 3), dtype=t.float32, device=dev)
    faces = t.empty((F, 3), dtype=t.int32, device=dev)
    if F:
      be.marching_cubes_emit(grid, level, matrices, vertices, normals, faces)
    return Meshes(vertices, normals, faces, counts[:, 0].clone(), counts[:, 1].clone())
  if dev.type != "cpu":
    raise ValueError(f"marching cubes: unsupported device {dev}")
  lib = _lib()
  st = (C.c_int64 * 4)(*grid.stride())
  counts = t.empty((N, 2), dtype=t.int64)
  nthreads = t.get_num_threads()                                         # host twin: one object per thread
  lib.crn_marching_cubes_cpu(grid.data_ptr(), st, N, D, H, W, level, None, counts.data_ptr(), None, None, None, nthreads)
  V, F = int(counts[:, 0].sum()), int(counts[:, 1].sum())
  vertices = t.empty((V, 3), dtype=t.float32)
  normals = t.empty((V, 3), dtype=t.float32)
  faces = t.empty((F, 3), dtype=t.int32)
  if F:
    lib.crn_marching_cubes_cpu(grid.data_ptr(), st, N, D, H, W, level, None if matrices is None else matrices.data_ptr(),
                               counts.data_ptr(), vertices.data_ptr(), normals.data_ptr(), faces.data_ptr(), nthreads)
  return Meshes(vertices, normals, faces, counts[:, 0].clone(), counts[:, 1].clone())


def _triangle_soup(m: Meshes, dummy_v: t.Tensor, dummy_n: t.Tensor) -> Tuple[t.Tensor, t.Tensor, t.Tensor]:
  """Meshes -> the reference's (triangles [T, 3, 3], normals [T, 3, 3], mesh_num_tri int32 [N]); an object without
  faces gets one dummy triangle (artifacts.py:271-275)."""
  dev = m.vertices.device
  nv, nf = m.num_vertices, m.num_faces
  vbase = t.cumsum(nv, 0) - nv
  obj = t.repeat_interleave(t.arange(len(nf), device=dev), nf)
  idx = m.faces.to(t.int64) + vbase[obj][:, None]
  tri, nrm = m.vertices[idx], m.normals[idx]
  empty = nf == 0
  if bool(empty.any()):
    cnt = t.where(empty, t.ones_like(nf), nf)
    start = t.cumsum(cnt, 0) - cnt                                        # first triangle of every object in the output
    T = int(cnt.sum())
    if dummy_v.dim() == 3:                                                # one dummy triangle per object
      owner = t.repeat_interleave(t.arange(len(cnt), device=dev), cnt, output_size=T)
      tri_out, nrm_out = dummy_v.to(dev)[owner], dummy_n.to(dev)[owner]
    else:
      tri_out = dummy_v.to(dev).expand(T, 3, 3).clone()
      nrm_out = dummy_n.to(dev).expand(T, 3, 3).clone()
    pos = start[obj] + (t.arange(len(obj), device=dev) - (t.cumsum(nf, 0) - nf)[obj])
    tri_out[pos], nrm_out[pos] = tri, nrm
    return tri_out, nrm_out, cnt.to(t.int32)
  return tri, nrm, nf.to(t.int32)


def to_marching_cubes(voxel_grid) -> Tuple[t.Tensor, t.Tensor, t.Tensor]:
  """MarchingCubesArtifact.to_marching_cubes (artifacts.py:249-289): voxel_grid f32 [N, D, H, W] ->
  triangles f32 [T, 3, 3], normals f32 [T, 3, 3] (per-triangle corner copies, (x, y, z) = (w, h, d), padded index
  space), mesh_num_tri int32 [N]; an object with no value > 0.5 contributes one triangle of ones (count 1)."""
  m = marching_cubes(voxel_grid, level=0.5)
  ones = t.ones((3, 3), dtype=t.float32)
  return _triangle_soup(m, ones, ones)


def marching_cubes_artifact_mesh(grid, voxel_to_world, filter_kernel: int = 1) -> Tuple[t.Tensor, t.Tensor, t.Tensor]:
  """What MarchingCubesArtifact.__init__ (artifacts.py:202-238) hands to its mesh artifact: grid [C, D, H, W] (class 0
  first), optionally box-filtered, meshed per class for grid[1:], then transformed by voxel_to_world f32 [4, 4]
  (vertices as points, normals as vectors).  Returns (vertices [T, 3, 3], normals [T, 3, 3], mesh_num_tri int32 [C-1]);
  the dummy triangle of an empty class is transformed like the reference transforms it."""
  grid = _as_grid(grid)
  m4 = t.as_tensor(voxel_to_world, dtype=t.float32)
  if tuple(m4.shape) != (4, 4):
    raise ValueError(f"voxel_to_world must be [4, 4], got {tuple(m4.shape)}")
  if filter_kernel > 1:
    grid = box_filter(grid, int(filter_kernel))
  grid = grid[1:]
  m = marching_cubes(grid, level=0.5, matrices=m4.to(grid.device))
  mh = m4.to("cpu", t.float64)
  h = mh @ t.ones(4, dtype=t.float64)
  dummy_v = (h[:3] / h[3]).to(t.float32).expand(3, 3)
  dummy_n = (mh[:3, :3] @ t.ones(3, dtype=t.float64)).to(t.float32).expand(3, 3)
  return _triangle_soup(m, dummy_v, dummy_n)


def write_ply(path: str, vertices, faces, normals=None) -> None:
  """Binary little-endian PLY: float x y z (+ nx ny nz), faces as `list uchar int vertex_indices`."""
  v = np.ascontiguousarray(t.as_tensor(vertices).detach().cpu().numpy(), dtype="<f4").reshape(-1, 3)
  f = np.ascontiguousarray(t.as_tensor(faces).detach().cpu().numpy(), dtype="<i4").reshape(-1, 3)
  cols = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
  if normals is not None:
    n = np.ascontiguousarray(t.as_tensor(normals).detach().cpu().numpy(), dtype="<f4").reshape(-1, 3)
    if n.shape != v.shape:
      raise ValueError("write_ply: normals must have the vertices' shape")
    cols += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
  vrec = np.empty(len(v), dtype=cols)
  vrec["x"], vrec["y"], vrec["z"] = v[:, 0], v[:, 1], v[:, 2]
  if normals is not None:
    vrec["nx"], vrec["ny"], vrec["nz"] = n[:, 0], n[:, 1], n[:, 2]
  frec = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
  frec["n"], frec["i"] = 3, f
  head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(v)]
  head += ["property float %s" % c for c, _ in cols]
  head += ["element face %d" % len(f), "property list uchar int vertex_indices", "end_header"]
  with open(path, "wb") as fh:
    fh.write(("\n".join(head) + "\n").encode("ascii"))
    fh.write(vrec.tobytes())
    fh.write(frec.tobytes())
