"""Surfaces of predicted voxel grids: GPU marching cubes (csrc/marching_cubes.hip) and its host twin."""
from corenet_amd.visualization.marching_cubes import (Meshes, box_filter, marching_cubes, marching_cubes_artifact_mesh,
                                                      to_marching_cubes, write_ply)

__all__ = ["Meshes", "box_filter", "marching_cubes", "marching_cubes_artifact_mesh", "to_marching_cubes", "write_ply"]
