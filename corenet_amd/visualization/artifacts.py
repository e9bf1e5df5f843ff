"""Visualisation artifacts (reference: visualization/artifacts.py): meshes, label grids, marching-cubes surfaces and
images drawn from a common set of cameras.  Rendering goes through corenet_amd.visualization.render (GPU kernels for
CUDA tensors, the host twin for CPU tensors).  evaluation_results.visualize_output batches all of one eval batch's
panels into one render call instead of rendering artifact by artifact; both produce the same pictures."""
from __future__ import annotations

import sys
from typing import Iterable, List, Optional, Tuple, Union

import numpy as np
import PIL.Image
import torch as t

from corenet_amd.geometry import transformations
from corenet_amd.visualization import camera_util, colors, render
from corenet_amd.visualization.marching_cubes import marching_cubes_artifact_mesh


def points_box(points: t.Tensor, matrix) -> t.Tensor:
  """Bounds f32 [2, 3] of points f32 [P, 3] transformed as points by matrix [4, 4] with the homogeneous divide.
  Every product and sum is its own float32 elementwise operation, in the order ((m0 x + m1 y) + m2 z) + m3, so the
  bounds are the same on every device."""
  m = render._host(matrix).tolist()
  x, y, z = points[:, 0], points[:, 1], points[:, 2]
  h = [((x * m[r][0] + y * m[r][1]) + z * m[r][2]) + m[r][3] for r in range(4)]
  q = t.stack([h[0] / h[3], h[1] / h[3], h[2] / h[3]], 1)
  return t.stack([q.min(0)[0], q.max(0)[0]], 0)


class VisualizationArtifact:
  """Something drawn in the common (view-space) frame of a scene."""

  def get_3d_box(self, transform) -> Optional[t.Tensor]:
    """Bounds f32 [2, 3] of the artifact under `transform` [4, 4], or None for a 2D artifact."""
    raise NotImplementedError()

  def render(self, camera_matrix, output_shape: Tuple[int, int]) -> t.Tensor:
    """uint8 [height, width, 3] seen through camera_matrix [4, 4]."""
    raise NotImplementedError()


class MultiMeshArtifact(VisualizationArtifact):
  """Several meshes in one triangle soup: vertices f32 [T, 3, 3], mesh_num_tri int32 [num_meshes], optional
  per-vertex normals, mesh_colors f32 [num_meshes, 3] (default DEFAULT_COLOR_PALETTE[1:])."""

  def __init__(self, vertices, mesh_num_tri, normals=None, mesh_colors=None):
    vertices = t.as_tensor(vertices, dtype=t.float32)
    assert vertices.dim() == 3 and vertices.shape[1:] == (3, 3)
    mesh_num_tri = t.as_tensor(mesh_num_tri).to(t.int64).cpu()
    assert mesh_num_tri.dim() == 1 and int(mesh_num_tri.sum()) == vertices.shape[0]
    if mesh_colors is None:
      mesh_colors = colors.DEFAULT_COLOR_PALETTE[1:mesh_num_tri.shape[0] + 1]
    mesh_colors = render._host(mesh_colors)
    assert mesh_colors.shape == (mesh_num_tri.shape[0], 3)
    if normals is not None:
      normals = t.as_tensor(normals, dtype=t.float32).to(vertices.device)
      assert normals.shape == vertices.shape
    self.vertices, self.normals, self.mesh_num_tri, self.mesh_colors = vertices, normals, mesh_num_tri, mesh_colors

  def get_3d_box(self, transform) -> Optional[t.Tensor]:
    return points_box(self.vertices.reshape(-1, 3), transform).cpu()

  def render(self, camera_matrix, output_shape: Tuple[int, int]) -> t.Tensor:
    mids = t.repeat_interleave(t.arange(len(self.mesh_num_tri), dtype=t.int32), self.mesh_num_tri)
    return render.render_scene(self.vertices, camera_matrix, output_shape, normals=self.normals, material_ids=mids,
                               diffuse_coefficients=self.mesh_colors, cull_back_facing=False)


class VoxelGridArtifact(VisualizationArtifact):
  """A label grid int32 [D, H, W] placed by voxel_to_world_transform [4, 4]; palette f32 [max_label, 3] (default
  DEFAULT_COLOR_PALETTE[1:]); label 0 is void.  frame_label > 0 draws a frame of that label along the grid's edges."""

  def __init__(self, voxel_grid, voxel_to_world_transform, palette=None, frame_label: int = -1):
    voxel_grid = t.as_tensor(voxel_grid).to(t.int32)
    assert voxel_grid.dim() == 3
    v2w = render._host(voxel_to_world_transform)
    assert v2w.shape == (4, 4)
    max_label = max(int(voxel_grid.max()), frame_label)
    if palette is None:
      palette = colors.DEFAULT_COLOR_PALETTE[1:max_label + 1]
    palette = render._host(palette)
    assert palette.shape == (max_label, 3)
    self.palette = t.cat([-t.ones(1, 3), palette], 0)
    if frame_label > 0:
      voxel_grid = VoxelGridArtifact.draw_frame(voxel_grid.clone(), frame_label)
    self.voxel_grid = voxel_grid
    self.voxel_to_world_transform = v2w

  def get_3d_box(self, transform) -> Optional[t.Tensor]:
    m = transformations.chain([render._host(transform), self.voxel_to_world_transform])
    f = render.voxel_faces(self.voxel_grid[None], self.palette, self.voxel_to_world_transform, box_matrices=m)
    return f.boxes[0].cpu()

  def render(self, camera_matrix, output_shape: Tuple[int, int]) -> t.Tensor:
    return render.render_voxel_grid(self.voxel_grid, camera_matrix, output_shape,
                                    voxel_to_view_matrix=self.voxel_to_world_transform,
                                    diffuse_coefficients=self.palette)

  @classmethod
  def draw_frame(cls, grid: t.Tensor, label: int) -> t.Tensor:
    """Sets the 12 edges of grid [D, H, W] to `label`, in place; returns grid."""
    for a in (0, -1):
      for b in (0, -1):
        grid[:, a, b] = label
        grid[a, :, b] = label
        grid[a, b, :] = label
    return grid


class MarchingCubesArtifact(VisualizationArtifact):
  """The level-0.5 surfaces of grid f32 [C, D, H, W] (class 0 skipped), optionally box-filtered, placed by
  voxel_to_world [4, 4]; palette f32 [C, 3] (palette[1:] colours the meshes)."""

  def __init__(self, grid, voxel_to_world, palette=None, filter_kernel: int = 1):
    vertices, normals, mesh_num_tri = marching_cubes_artifact_mesh(grid, render._host(voxel_to_world), filter_kernel)
    if palette is not None:
      palette = render._host(palette)[1:]
    self.mesh_artifact = MultiMeshArtifact(vertices, mesh_num_tri, normals=normals, mesh_colors=palette)

  def get_3d_box(self, transform) -> Optional[t.Tensor]:
    return self.mesh_artifact.get_3d_box(transform)

  def render(self, camera_matrix, output_shape: Tuple[int, int]) -> t.Tensor:
    return self.mesh_artifact.render(camera_matrix, output_shape)


class ImageArtifact(VisualizationArtifact):
  """An image uint8 [3, height, width], drawn the same from every camera."""

  def __init__(self, image):
    image = t.as_tensor(image)
    assert image.dim() == 3 and image.shape[0] == 3
    self.image = image.to(t.uint8)

  def get_3d_box(self, transform) -> Optional[t.Tensor]:
    return None

  def render(self, camera_matrix, output_shape: Tuple[int, int]) -> t.Tensor:
    return resize_image(self.image, output_shape).to(self.image.device)


def resize_image(image: t.Tensor, output_shape: Tuple[int, int]) -> t.Tensor:
  """ImageArtifact.render: uint8 [3, h, w] -> uint8 [H, W, 3] on the host, scaled with PIL's bilinear filter to fit
  and keep its aspect ratio, then zero-padded around.  As in the reference the right padding is computed from
  output_shape[0] (the same for the square default)."""
  _, sh, sw = image.shape
  scale = min(output_shape[0] / sh, output_shape[1] / sw)
  th, tw = min(round(sh * scale), output_shape[0]), min(round(sw * scale), output_shape[1])
  pil = PIL.Image.fromarray(image.detach().cpu().permute(1, 2, 0).numpy())
  out = t.from_numpy(np.array(pil.resize((tw, th), PIL.Image.BILINEAR)))
  top, left = (output_shape[0] - th) // 2, (output_shape[1] - tw) // 2
  out = t.constant_pad_nd(out, [0, 0, left, output_shape[0] - left - tw, top, output_shape[0] - top - th])
  return out.contiguous()


def extra_views_for_box(ltf: t.Tensor, rbb: t.Tensor, aspect_ratio: float, view_to_world) -> List[t.Tensor]:
  """The four tetrahedron cameras around the box [ltf, rbb] (world space), as compute_extra_views builds them (host
  float32): an empty box (ltf > rbb anywhere) becomes the unit cube."""
  ltf, rbb = render._host(ltf), render._host(rbb)
  if bool((ltf > rbb).any()):
    ltf, rbb = t.zeros(3), t.ones(3)
  center = (ltf + rbb) / 2
  diagonal = (rbb - ltf).max()
  proj = camera_util.perspective_projection(aspect_ratio, znear=0.01, zfar=10)
  v2w = render._host(view_to_world)
  return [transformations.chain([proj, transformations.translate([0, 0, 0.3]), cam,
                                 transformations.scale(t.stack([1 / diagonal] * 3)), transformations.translate(-center),
                                 v2w])
          for cam in camera_util.cameras_on_tetrahedron_vertices()]


def compute_extra_views(artifacts: Iterable[VisualizationArtifact], aspect_ratio: float,
                        world_to_view) -> List[t.Tensor]:
  """Four extra cameras f32 [4, 4] (host) framing the union of the artifacts' 3D boxes."""
  view_to_world = t.inverse(render._host(world_to_view))
  ltf = t.tensor([sys.float_info.max] * 3, dtype=t.float32)       # +-inf in float32, as in the reference
  rbb = t.tensor([-sys.float_info.max] * 3, dtype=t.float32)
  for a in artifacts:
    box = a.get_3d_box(view_to_world)
    if box is None:
      continue
    ltf, rbb = t.min(ltf, box[0].cpu()), t.max(rbb, box[1].cpu())
  return extra_views_for_box(ltf, rbb, aspect_ratio, view_to_world)


ArtifactOrGroup = Union[VisualizationArtifact, Iterable[VisualizationArtifact]]


def visualize_artifacts(artifacts: Iterable[ArtifactOrGroup], default_camera, world_to_view,
                        image_size: Tuple[int, int] = (384, 384)) -> List[t.Tensor]:
  """Five rows uint8 [H, W * num_artifacts, 3], one per camera (default_camera, then the four extra views of each
  group); artifacts of a group share the extra views."""
  rows = [[] for _ in range(5)]
  for group in artifacts:
    if isinstance(group, VisualizationArtifact):
      group = [group]
    group = list(group)
    cams = [render._host(default_camera)] + compute_extra_views(group, image_size[1] / image_size[0], world_to_view)
    for i, cam in enumerate(cams):
      for a in group:
        rows[i].append(a.render(cam, image_size))
  dev = next((r.device for r in rows[0] if r.device.type != "cpu"), t.device("cpu"))
  return [t.cat([x.to(dev) for x in r], 1) for r in rows]
