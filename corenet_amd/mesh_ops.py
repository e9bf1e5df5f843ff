"""Mesh clean-up: vertex / face incidence tables, Taubin smoothing, area-weighted normals and vertex clustering of
batches of indexed meshes, as `visualization.Meshes` holds them.

CUDA(HIP) tensors run the kernels of csrc/mesh_ops.hip, CPU tensors the library's host twin (csrc/mesh_ops_cpu.cpp).  Both
give the same tensors bit for bit; a CUDA tensor never goes to the host twin.  Everything is queued on the current stream
and nothing depends on crn_set_deterministic.

Contract (the C interface in include/corenet_hip.h states the same):
  * Input: vertices f32 [V, 3], faces i32 [F, 3] with vertex ids local to their object, num_vertices / num_faces i64 [N]
    (tensors on any device, or sequences).  V < 2^31 and 3 F < 2^31.  N == 0, objects without vertices or faces and
    vertices used by no face give empty results.  "Global" ids have the object's first vertex (face) added.
  * All float arithmetic is float32, IEEE + - * / sqrtf in the order written, never contracted.

mesh_topology(faces, num_vertices, num_faces) -> MeshTopology
  * vertex_offsets, face_offsets: i64 [N + 1] on the host (vertex_offsets_dev / face_offsets_dev: the same on the device).
  * vf_offsets i64 [V + 1], vf_corners i32 [3 F]: per vertex the corners that name it, 3 * global_face + corner, ascending;
    one entry per corner, so a face that names a vertex twice is listed twice.
  * vv_offsets i64 [V + 1], vv_neighbours i32 [E]: per vertex the distinct global ids of the other vertices it shares a
    face with, ascending, itself excluded.
  * irregular bool [V].  Face (i, j, k) has the directed edges i -> j, j -> k, k -> i.  An undirected edge {a, b} is regular
    iff a -> b occurs in exactly one face and b -> a in exactly one; a self edge a -> a (a degenerate face) is never
    regular.  A vertex is irregular iff one of its edges is not regular: boundary, non-manifold, inconsistent winding.
  * A face id < 0 or >= its object's num_vertices raises ValueError, so do counts that do not add up to F (and V).
  * On the GPU the call synchronises once: E, the number of bad ids and -- when they arrive as device tensors -- the
    counts are read back together.  Device counts leave V unknown before that read: pass total_vertices (every caller
    that holds the vertices does); without it the counts are read first, a second synchronisation.
  * Lists of up to mesh_ops_tiles().sort_lane keys are sorted by one lane, longer ones by a workgroup, rank by counting
    through LDS tiles of sort_tile keys; the candidate list behind vv has two keys per corner.
is_closed(topology) -> bool [N]: no irregular vertex; an object without faces is closed.

taubin_smooth(vertices, topology, iterations=10, lam=0.5, mu=-0.53, fixed=None) -> f32 [V, 3]
  * One iteration is a step with factor lam, then one with factor mu; mu=None: the lam step alone (Laplacian smoothing).
  * A step with factor f gives a vertex with k >= 1 neighbours that is not in fixed (bool [V]), per component,
    s = ((n0 + n1) + n2) + ... over its neighbours in vv order, m = s / float(k), v' = v + f * (m - v).  Every other vertex
    is copied.  Steps ping-pong between two buffers; iterations=0 returns a copy.  Non-finite values spread by the rule
    and nothing else.

vertex_normals(vertices, faces, topology) -> f32 [V, 3]: per vertex, 0 + the cross products (b - a) x (c - a) of the faces
  of its vf_corners, in order (a, b, c the face's corners 0, 1, 2; x = (u.y * w.z) - (u.z * w.y), cyclically), divided
  by sqrtf((x * x + y * y) + z * z).  A zero length gives (0, 0, 0), as marching_cubes does.  faces must be the topology's.
face_normals(vertices, faces, num_vertices, num_faces=None) -> f32 [F, 3]: the cross products, un-normalised.  num_faces
  may only be left out for a single object.  A face with a bad id gets (0, 0, 0); mesh_topology is what raises on them.

cluster_decimate(vertices, faces, num_vertices, num_faces, cell_size) -> Decimated(meshes, vertex_map, cluster_size)
  * Vertex clustering on a lattice of pitch cell_size (a float > 0, converted to float32 once).  Per axis x = v / cell,
    c = floorf(x), u = (int64)((x - c) * 2^20).  A cluster is (object, c_x, c_y, c_z): two objects never share one.
  * New vertices are ordered by the lowest old vertex id of their cluster, so objects stay contiguous and in order.
    Position per axis: float32((double(c) + (double(sum u) / double(count)) * 2^-20) * double(cell)), sum u exact in int64.
  * Faces: ids mapped to new local ids, faces with two equal ids dropped, order kept.  Faces that become equal to one
    another are all kept: nothing looks for duplicates.
  * meshes.normals is vertex_normals of the result; vertex_map i32 [V] is old -> new global id; cluster_size i32 [V'].
  * Cell indices in [cell_min, cell_max] of mesh_ops_tiles(); a non-finite vertex or a cell outside raises ValueError, so
    does a bad face id.  max_objects objects per launch: larger batches are split.  cluster_max_vertices per launch.
  * One synchronisation (the new per-object counts and the bad count, together) besides the one of mesh_topology.

mesh_volume_area(vertices, faces, num_vertices, num_faces) -> (f64 [N], f64 [N]): signed volume by the divergence theorem
  and area, in torch float64 on the mesh's device."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch as t


class MeshOpsTiles(NamedTuple):
  threads: int                 # items (vertices, faces, corners) per workgroup
  sort_lane: int               # the longest list one lane sorts alone
  sort_tile: int               # keys of a longer list that pass through LDS at a time
  cell_min: int
  cell_max: int
  max_objects: int             # per clustering launch
  cluster_max_vertices: int    # per clustering launch


class MeshTopology(NamedTuple):
  vertex_offsets: t.Tensor     # i64 [N + 1], host
  face_offsets: t.Tensor       # i64 [N + 1], host
  vf_offsets: t.Tensor         # i64 [V + 1]
  vf_corners: t.Tensor         # i32 [3 F]
  vv_offsets: t.Tensor         # i64 [V + 1]
  vv_neighbours: t.Tensor      # i32 [E]
  irregular: t.Tensor          # bool [V]
  vertex_offsets_dev: t.Tensor # the offsets on the tables' device
  face_offsets_dev: t.Tensor


class Decimated(NamedTuple):
  meshes: "Meshes"
  vertex_map: t.Tensor         # i32 [V] old -> new global id
  cluster_size: t.Tensor       # i32 [V']


def _lib():
  from corenet_amd import _lib as L
  return L.lib()


def _backend():
  from corenet_amd.backend import default_backend
  return default_backend()


def mesh_ops_tiles() -> MeshOpsTiles:
  out = (C.c_int32 * 7)()
  _lib().crn_mesh_tiles(C.addressof(out))
  return MeshOpsTiles(*(int(x) for x in out))


def _device_ok(x: t.Tensor, what: str):
  if x.device.type not in ("cuda", "cpu"):
    raise ValueError(f"{what}: unsupported device {x.device}")


def _faces(faces, what: str) -> t.Tensor:
  faces = t.as_tensor(faces)
  if faces.dim() != 2 or faces.shape[1] != 3:
    raise ValueError(f"{what}: faces must be [F, 3], got {tuple(faces.shape)}")
  if faces.dtype.is_floating_point or faces.dtype.is_complex or faces.dtype == t.bool:
    raise ValueError(f"{what}: faces must be integers, got {faces.dtype}")
  _device_ok(faces, what)
  if 3 * faces.shape[0] >= 1 << 31:
    raise ValueError(f"{what}: {faces.shape[0]} faces, 3 F must stay below 2^31")
  return faces.to(t.int32).contiguous()


def _vertices(vertices, what: str) -> t.Tensor:
  vertices = t.as_tensor(vertices)
  if vertices.dim() != 2 or vertices.shape[1] != 3:
    raise ValueError(f"{what}: vertices must be [V, 3], got {tuple(vertices.shape)}")
  _device_ok(vertices, what)
  if vertices.shape[0] >= 1 << 31:
    raise ValueError(f"{what}: {vertices.shape[0]} vertices, V must stay below 2^31")
  return vertices.to(t.float32).contiguous()


def _counts(c, what: str) -> t.Tensor:
  c = t.as_tensor(c)
  if c.dim() != 1 or c.dtype.is_floating_point or c.dtype.is_complex:
    raise ValueError(f"{what}: counts must be an integer vector [N], got {c.dtype} {tuple(c.shape)}")
  return c.to(t.int64)


def _exclusive(c: t.Tensor) -> t.Tensor:
  """[N] -> the offsets [N + 1] on c's device."""
  out = t.zeros(c.numel() + 1, dtype=t.int64, device=c.device)
  t.cumsum(c, 0, out=out[1:])
  return out


def _host_offsets(nv: t.Tensor, nf: t.Tensor, V: Optional[int], F: int, what: str) -> Tuple[t.Tensor, t.Tensor]:
  if nv.numel() != nf.numel():
    raise ValueError(f"{what}: num_vertices has {nv.numel()} objects and num_faces {nf.numel()}")
  if bool((nv < 0).any()) or bool((nf < 0).any()):
    raise ValueError(f"{what}: negative counts")
  voff, foff = _exclusive(nv), _exclusive(nf)
  if int(foff[-1]) != F:
    raise ValueError(f"{what}: num_faces adds up to {int(foff[-1])}, faces has {F} rows")
  if V is not None and int(voff[-1]) != V:
    raise ValueError(f"{what}: num_vertices adds up to {int(voff[-1])}, expected {V} vertices")
  if int(voff[-1]) >= 1 << 31:
    raise ValueError(f"{what}: {int(voff[-1])} vertices, V must stay below 2^31")
  return voff, foff


def mesh_topology(faces, num_vertices, num_faces, total_vertices: Optional[int] = None) -> MeshTopology:
  """The incidence tables of a batch of indexed meshes (see the module docstring for the contract)."""
  what = "mesh_topology"
  faces = _faces(faces, what)
  nv, nf = _counts(num_vertices, what), _counts(num_faces, what)
  F, dev = faces.shape[0], faces.device
  if total_vertices is not None:
    total_vertices = int(total_vertices)
    if not 0 <= total_vertices < 1 << 31:
      raise ValueError(f"{what}: total_vertices must lie in [0, 2^31), got {total_vertices}")
  if not faces.is_cuda:
    voff, foff = _host_offsets(nv.cpu(), nf.cpu(), total_vertices, F, what)
    V, N = int(voff[-1]), nv.numel()
    vf_offsets = t.empty(V + 1, dtype=t.int64)
    vf_corners = t.empty(3 * F, dtype=t.int32)
    vv_offsets = t.empty(V + 1, dtype=t.int64)
    irregular = t.empty(V, dtype=t.uint8)
    counts = t.empty(2, dtype=t.int64)
    args = (faces.data_ptr(), F, voff.data_ptr(), foff.data_ptr(), N, V, vf_offsets.data_ptr(), vf_corners.data_ptr(), vv_offsets.data_ptr())
    _lib().crn_mesh_topology_cpu(*args, None, irregular.data_ptr(), counts.data_ptr())
    if int(counts[1]):
      raise ValueError(f"{what}: {int(counts[1])} face ids outside their object's vertices")
    vv = t.empty(int(counts[0]), dtype=t.int32)
    _lib().crn_mesh_topology_cpu(*args, vv.data_ptr(), irregular.data_ptr(), counts.data_ptr())
    return MeshTopology(voff, foff, vf_offsets, vf_corners, vv_offsets, vv, irregular.view(t.bool), voff, foff)
  on_device = nv.is_cuda or nf.is_cuda
  if on_device and total_vertices is None:
    nv, nf = nv.cpu(), nf.cpu()                                             # V sizes the tables: the extra read-back
    on_device = False
  if on_device:
    if nv.numel() != nf.numel():
      raise ValueError(f"{what}: num_vertices has {nv.numel()} objects and num_faces {nf.numel()}")
    nv, nf = nv.to(dev), nf.to(dev)
    V = total_vertices
    voff = voff_dev = _exclusive(nv)
    foff = foff_dev = _exclusive(nf)
  else:
    voff, foff = _host_offsets(nv.cpu(), nf.cpu(), total_vertices, F, what)
    V = int(voff[-1])
    voff_dev, foff_dev = voff.to(dev), foff.to(dev)
  be = _backend()
  i32 = dict(dtype=t.int32, device=dev)
  bad = t.empty(1, dtype=t.int64, device=dev)
  deg = t.empty(V, **i32)
  be.mesh_corner_count(faces, voff_dev, foff_dev, V, deg, bad)
  vf_offsets = t.zeros(V + 1, dtype=t.int64, device=dev)
  t.cumsum(deg, 0, out=vf_offsets[1:])
  vf_tmp, vf_corners = t.empty(3 * F, **i32), t.empty(3 * F, **i32)
  cand_tmp, cand = t.empty(6 * F, **i32), t.empty(6 * F, **i32)
  vvdeg = t.empty(V, **i32)
  irregular = t.empty(V, dtype=t.uint8, device=dev)
  be.mesh_corner_lists(faces, voff_dev, foff_dev, V, vf_offsets, deg, vf_tmp, vf_corners, cand_tmp, cand, vvdeg, irregular)
  del vf_tmp, cand_tmp
  vv_offsets = t.zeros(V + 1, dtype=t.int64, device=dev)
  t.cumsum(vvdeg, 0, out=vv_offsets[1:])
  parts = [vv_offsets[-1:], bad] + ([voff_dev, foff_dev] if on_device else [])
  host = t.cat(parts).cpu()                                                 # the call's one synchronisation
  E, nbad = int(host[0]), int(host[1])
  if on_device:
    N = nv.numel()
    voff, foff = host[2:3 + N].clone(), host[3 + N:].clone()
    if bool((voff[1:] < voff[:-1]).any()) or bool((foff[1:] < foff[:-1]).any()):
      raise ValueError(f"{what}: negative counts")
    if int(voff[-1]) != V or int(foff[-1]) != F:
      raise ValueError(f"{what}: the counts add up to {int(voff[-1])} vertices and {int(foff[-1])} faces, expected {V} and {F}")
  if nbad:
    raise ValueError(f"{what}: {nbad} face ids outside their object's vertices")
  vv = t.empty(E, **i32)
  be.mesh_neighbours(cand, vf_offsets, vv_offsets, V, vv)
  return MeshTopology(voff, foff, vf_offsets, vf_corners, vv_offsets, vv, irregular.view(t.bool), voff_dev, foff_dev)


def is_closed(topology: MeshTopology) -> t.Tensor:
  """bool [N] on the tables' device: the object has no irregular vertex (an object without faces is closed)."""
  irr = topology.irregular
  cs = t.zeros(irr.numel() + 1, dtype=t.int64, device=irr.device)
  t.cumsum(irr.to(t.int64), 0, out=cs[1:])
  off = topology.vertex_offsets_dev
  return (cs[off[1:]] - cs[off[:-1]]) == 0


def _same_place(x: t.Tensor, topology: MeshTopology, what: str):
  if x.device != topology.vf_offsets.device:
    raise ValueError(f"{what}: tensors on {x.device}, the topology on {topology.vf_offsets.device}")


def taubin_smooth(vertices, topology: MeshTopology, iterations: int = 10, lam: float = 0.5, mu: Optional[float] = -0.53,
                  fixed=None) -> t.Tensor:
  """Taubin (lam, then mu) or, with mu=None, Laplacian smoothing over the topology's neighbour lists (module docstring)."""
  what = "taubin_smooth"
  v = _vertices(vertices, what)
  _same_place(v, topology, what)
  V = v.shape[0]
  if V != topology.vv_offsets.numel() - 1:
    raise ValueError(f"{what}: {V} vertices, the topology has {topology.vv_offsets.numel() - 1}")
  if int(iterations) != iterations or iterations < 0:
    raise ValueError(f"{what}: iterations must be a non-negative integer, got {iterations}")
  if fixed is not None:
    fixed = t.as_tensor(fixed)
    if fixed.dtype != t.bool or tuple(fixed.shape) != (V,):
      raise ValueError(f"{what}: fixed must be bool [{V}], got {fixed.dtype} {tuple(fixed.shape)}")
    _same_place(fixed, topology, what)
    fixed = fixed.contiguous().view(t.uint8)
  a = v.clone() if v.data_ptr() == t.as_tensor(vertices).data_ptr() else v
  if V == 0 or iterations == 0:
    return a
  b = t.empty_like(a)
  factors = [float(lam)] if mu is None else [float(lam), float(mu)]
  be = _backend() if v.is_cuda else None
  for _ in range(int(iterations)):
    for f in factors:
      if be is not None:
        be.mesh_smooth_step(a, b, topology.vv_offsets, topology.vv_neighbours, fixed, f)
      else:
        _lib().crn_mesh_smooth_step_cpu(a.data_ptr(), b.data_ptr(), topology.vv_offsets.data_ptr(), topology.vv_neighbours.data_ptr(),
                                        None if fixed is None else fixed.data_ptr(), f, V)
      a, b = b, a
  return a


def vertex_normals(vertices, faces, topology: MeshTopology) -> t.Tensor:
  """Area-weighted unit normals from the faces (module docstring); faces must be the ones the topology was built from."""
  what = "vertex_normals"
  v, faces = _vertices(vertices, what), _faces(faces, what)
  _same_place(v, topology, what)
  _same_place(faces, topology, what)
  V, F = v.shape[0], faces.shape[0]
  if V != topology.vf_offsets.numel() - 1 or 3 * F != topology.vf_corners.numel():
    raise ValueError(f"{what}: {V} vertices and {F} faces do not match the topology")
  out = t.empty_like(v)
  if V == 0:
    return out
  N = topology.vertex_offsets.numel() - 1
  if v.is_cuda:
    _backend().mesh_vertex_normals(v, faces, topology.vertex_offsets_dev, topology.vf_offsets, topology.vf_corners, out)
  else:
    _lib().crn_mesh_vertex_normals_cpu(v.data_ptr(), faces.data_ptr(), F, topology.vertex_offsets.data_ptr(), N, V,
                                       topology.vf_offsets.data_ptr(), topology.vf_corners.data_ptr(), out.data_ptr())
  return out


def _device_offsets(nv: t.Tensor, nf: t.Tensor, dev, what: str) -> Tuple[t.Tensor, t.Tensor]:
  if nv.numel() != nf.numel():
    raise ValueError(f"{what}: num_vertices has {nv.numel()} objects and num_faces {nf.numel()}")
  return _exclusive(nv.to(dev)), _exclusive(nf.to(dev))


def face_normals(vertices, faces, num_vertices, num_faces=None) -> t.Tensor:
  """f32 [F, 3]: (b - a) x (c - a) of every face, un-normalised (module docstring)."""
  what = "face_normals"
  v, faces = _vertices(vertices, what), _faces(faces, what)
  if v.device != faces.device:
    raise ValueError(f"{what}: vertices on {v.device}, faces on {faces.device}")
  nv = _counts(num_vertices, what)
  if num_faces is None:
    if nv.numel() != 1:
      raise ValueError(f"{what}: num_faces may only be left out for a single object, got {nv.numel()}")
    num_faces = [faces.shape[0]]
  voff, foff = _device_offsets(nv, _counts(num_faces, what), v.device, what)
  out = t.empty((faces.shape[0], 3), dtype=t.float32, device=v.device)
  if faces.shape[0] == 0:
    return out
  if v.is_cuda:
    _backend().mesh_face_normals(v, faces, voff, foff, out)
  else:
    _lib().crn_mesh_face_normals_cpu(v.data_ptr(), faces.data_ptr(), faces.shape[0], voff.data_ptr(), foff.data_ptr(), nv.numel(),
                                     v.shape[0], out.data_ptr())
  return out


def _decimate_chunk(v: t.Tensor, faces: t.Tensor, nv: t.Tensor, nf: t.Tensor, cell: float, what: str):
  """One launch: (new_vertices, new_faces, new_nv host, new_nf host, vertex_map, cluster_size)."""
  V, F, N, dev = v.shape[0], faces.shape[0], nv.numel(), v.device
  tiles = mesh_ops_tiles()
  if V > tiles.cluster_max_vertices:
    raise ValueError(f"{what}: {V} vertices in one launch, at most {tiles.cluster_max_vertices}")
  i32 = dict(dtype=t.int32, device=dev)
  vertex_map = t.empty(V, **i32)
  if not v.is_cuda:
    voff, foff = _host_offsets(nv.cpu(), nf.cpu(), V, F, what)
    counts = t.empty(2 * N + 1, dtype=t.int64)
    args = (v.data_ptr(), V, faces.data_ptr(), F, voff.data_ptr(), foff.data_ptr(), N, cell, vertex_map.data_ptr(), counts.data_ptr())
    _lib().crn_mesh_cluster_cpu(*args, None, None, None)
    if int(counts[-1]):
      raise ValueError(f"{what}: {int(counts[-1])} vertices that are not finite or lie outside the cells "
                       f"[{tiles.cell_min}, {tiles.cell_max}], or face ids outside their object")
    new_nv, new_nf = counts[:N].clone(), counts[N:2 * N].clone()
    new_v = t.empty((int(new_nv.sum()), 3), dtype=t.float32)
    size = t.empty(new_v.shape[0], dtype=t.int32)
    new_f = t.empty((int(new_nf.sum()), 3), dtype=t.int32)
    _lib().crn_mesh_cluster_cpu(*args, new_v.data_ptr(), size.data_ptr(), new_f.data_ptr())
    return new_v, new_f, new_nv, new_nf, vertex_map, size
  be = _backend()
  voff, foff = _device_offsets(nv, nf, dev, what)
  log2 = max(1, (2 * V - 1).bit_length()) if V else 1
  keys = t.empty(1 << log2, dtype=t.int64, device=dev)
  leader = t.empty(1 << log2, **i32)
  slot_of, vflag, fkeep = t.empty(V, **i32), t.empty(V, **i32), t.empty(F, **i32)
  bad = t.empty(1, dtype=t.int64, device=dev)
  be.mesh_cluster_build(v, faces, voff, foff, cell, keys, leader, log2, slot_of, vflag, fkeep, bad)
  del keys
  vcs0 = t.zeros(V + 1, dtype=t.int64, device=dev)
  t.cumsum(vflag, 0, out=vcs0[1:])
  fcs0 = t.zeros(F + 1, dtype=t.int64, device=dev)
  t.cumsum(fkeep, 0, out=fcs0[1:])
  new_voff = vcs0[voff.clamp(0, V)]                                         # counts that do not add up are told below
  new_foff = fcs0[foff.clamp(0, F)]
  host = t.cat([new_voff[1:] - new_voff[:-1], new_foff[1:] - new_foff[:-1], bad, voff, foff]).cpu()    # the call's one synchronisation
  hv, hf = host[2 * N + 1:3 * N + 2], host[3 * N + 2:]
  if bool((hv[1:] < hv[:-1]).any()) or bool((hf[1:] < hf[:-1]).any()):
    raise ValueError(f"{what}: negative counts")
  if int(hv[-1]) != V or int(hf[-1]) != F:
    raise ValueError(f"{what}: the counts add up to {int(hv[-1])} vertices and {int(hf[-1])} faces, expected {V} and {F}")
  if int(host[2 * N]):
    raise ValueError(f"{what}: {int(host[2 * N])} vertices that are not finite or lie outside the cells "
                     f"[{tiles.cell_min}, {tiles.cell_max}], or face ids outside their object")
  new_nv, new_nf = host[:N].clone(), host[N:2 * N].clone()
  new_V, new_F = int(new_nv.sum()), int(new_nf.sum())
  new_v = t.empty((new_V, 3), dtype=t.float32, device=dev)
  new_f = t.empty((new_F, 3), **i32)
  size = t.empty(new_V, **i32)
  sums = t.empty((new_V, 3), dtype=t.int64, device=dev)
  be.mesh_cluster_emit(v, faces, voff, foff, cell, leader, slot_of, vflag, vcs0[1:], fkeep, fcs0[1:], new_voff, vertex_map, sums, size,
                       new_v, new_f)
  return new_v, new_f, new_nv, new_nf, vertex_map, size


def cluster_decimate(vertices, faces, num_vertices, num_faces, cell_size: float) -> Decimated:
  """Vertex clustering on a lattice of pitch cell_size (see the module docstring for the contract)."""
  from corenet_amd.visualization.marching_cubes import Meshes
  what = "cluster_decimate"
  v, faces = _vertices(vertices, what), _faces(faces, what)
  if v.device != faces.device:
    raise ValueError(f"{what}: vertices on {v.device}, faces on {faces.device}")
  cell = float(np.float32(cell_size))
  if not (cell > 0 and np.isfinite(cell)):
    raise ValueError(f"{what}: cell_size must be a finite float > 0, got {cell_size}")
  nv, nf = _counts(num_vertices, what), _counts(num_faces, what)
  N, dev = nv.numel(), v.device
  cap = mesh_ops_tiles().max_objects
  if N <= cap:
    new_v, new_f, new_nv, new_nf, vmap, size = _decimate_chunk(v, faces, nv, nf, cell, what)
  else:                                                                      # the chunks need the counts on the host
    nv, nf = nv.cpu(), nf.cpu()
    voff, foff = _host_offsets(nv, nf, v.shape[0], faces.shape[0], what)
    parts, base = [], 0
    for n0 in range(0, N, cap):
      n1 = min(n0 + cap, N)
      p = _decimate_chunk(v[int(voff[n0]):int(voff[n1])], faces[int(foff[n0]):int(foff[n1])], nv[n0:n1], nf[n0:n1], cell, what)
      parts.append(p[:4] + (p[4] + base, p[5]))
      base += p[0].shape[0]
    new_v, new_f, new_nv, new_nf, vmap, size = (t.cat([p[i] for p in parts]) for i in range(6))
  topo = mesh_topology(new_f, new_nv, new_nf)
  normals = vertex_normals(new_v, new_f, topo)
  return Decimated(Meshes(new_v, normals, new_f, new_nv.to(dev), new_nf.to(dev)), vmap, size)


def mesh_volume_area(vertices, faces, num_vertices, num_faces) -> Tuple[t.Tensor, t.Tensor]:
  """(signed volume f64 [N], area f64 [N]) of every object: sum of a . (b x c) / 6 and of |(b - a) x (c - a)| / 2 over its
  faces, in torch float64 on the mesh's device.  The volume is positive for a closed mesh whose faces are
  counter-clockwise seen from outside."""
  what = "mesh_volume_area"
  v, faces = _vertices(vertices, what), _faces(faces, what)
  dev = v.device
  nv, nf = _counts(num_vertices, what).to(dev), _counts(num_faces, what).to(dev)
  N = nv.numel()
  obj = t.repeat_interleave(t.arange(N, device=dev), nf, output_size=faces.shape[0])
  idx = faces.to(t.int64) + (_exclusive(nv)[:-1])[obj][:, None]
  p = v.to(t.float64)[idx]                                                   # [F, 3, 3]
  a, b, c = p[:, 0], p[:, 1], p[:, 2]
  vol = t.zeros(N, dtype=t.float64, device=dev).index_add_(0, obj, (a * t.linalg.cross(b, c)).sum(-1) / 6.0)
  area = t.zeros(N, dtype=t.float64, device=dev).index_add_(0, obj, t.linalg.cross(b - a, c - a).norm(dim=-1) / 2.0)
  return vol, area
