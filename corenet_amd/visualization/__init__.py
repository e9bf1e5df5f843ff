"""Visualisation of predicted and ground-truth scenes: GPU marching cubes (csrc/marching_cubes.hip), the batched
triangle / voxel-grid renderer (csrc/render.hip) and their host twins."""
from corenet_amd.visualization.marching_cubes import (Meshes, box_filter, marching_cubes, marching_cubes_artifact_mesh,
                                                      to_marching_cubes, write_ply)
from corenet_amd.visualization.instances import InstanceTable, instance_meshes
from corenet_amd.visualization.refine import refine_meshes
from corenet_amd.visualization.render import (GeometryBuffers, VoxelFaces, gather_triangle_attribute,
                                              interpolate_vertex_attribute, load_textures, make_materials, render_batch,
                                              render_geometry, render_scene, render_scenes, render_voxel_grid, voxel_faces,
                                              voxel_materials)

__all__ = ["Meshes", "box_filter", "marching_cubes", "marching_cubes_artifact_mesh", "to_marching_cubes", "write_ply",
           "InstanceTable", "instance_meshes", "refine_meshes", "VoxelFaces", "load_textures", "make_materials", "render_batch", "render_scene", "render_scenes",
           "render_voxel_grid", "voxel_faces", "voxel_materials", "GeometryBuffers", "render_geometry",
           "gather_triangle_attribute", "interpolate_vertex_attribute"]
