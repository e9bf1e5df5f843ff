"""Clean-up of meshes before they are written or drawn: optional vertex clustering, Taubin smoothing and normals
recomputed from the faces (corenet_amd.mesh_ops)."""
from __future__ import annotations

from typing import Optional

from corenet_amd.visualization.marching_cubes import Meshes


def refine_meshes(meshes: Meshes, cell_size: Optional[float] = None, smooth_iterations: int = 10, lam: float = 0.5,
                  mu: Optional[float] = -0.53) -> Meshes:
  """Meshes -> Meshes on the same device: clustered on a lattice of pitch cell_size (None: not decimated), smoothed with
  smooth_iterations Taubin iterations (0: not smoothed; mu=None: Laplacian), normals recomputed from the faces -- the
  normals marching_cubes returns come from the grid's gradient and no longer fit a vertex that has moved.  The result
  goes straight into write_ply, render_batch and the triangle soups."""
  from corenet_amd import mesh_ops
  if cell_size is not None:
    meshes = mesh_ops.cluster_decimate(meshes.vertices, meshes.faces, meshes.num_vertices, meshes.num_faces, cell_size).meshes
  topo = mesh_ops.mesh_topology(meshes.faces, meshes.num_vertices, meshes.num_faces, total_vertices=meshes.vertices.shape[0])
  vertices = mesh_ops.taubin_smooth(meshes.vertices, topo, smooth_iterations, lam, mu)
  normals = mesh_ops.vertex_normals(vertices, meshes.faces, topo)
  return Meshes(vertices, normals, meshes.faces, meshes.num_vertices, meshes.num_faces)
