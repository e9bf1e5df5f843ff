"""Camera matrices of the visualisations (reference: visualization/camera_util.py).  Host float32 math: every camera
is built on the host, whatever device the geometry is on, so the GPU and the host paths use the same matrices."""
import math

import numpy as np
import torch as t

from corenet_amd.geometry import transformations


def cameras_on_tetrahedron_vertices() -> t.Tensor:
  """View matrices f32[4, 4, 4] of cameras on the vertices of a tetrahedron, looking at the origin (left-handed, y up);
  the first three are above the origin, the last one below."""
  eyes = np.array([(math.sqrt(8.0 / 9), 1.0 / 3, 0), (-math.sqrt(2.0 / 9), 1.0 / 3, math.sqrt(2.0 / 3)),
                   (-math.sqrt(2.0 / 9), 1.0 / 3, -math.sqrt(2.0 / 3)), (0, -1, 0)], dtype=np.float32)
  ups = t.tensor([[0, 1, 0]] * 3 + [[1, -1, 0]], dtype=t.float32)
  return t.stack([transformations.look_at_lh(e, np.zeros(3, np.float32), u) for e, u in zip(eyes, ups)], 0)


def frontal_camera(offset: float) -> t.Tensor:
  """View matrix f32[4, 4] of a camera at (0, 0, offset) looking at the origin."""
  return transformations.look_at_lh((0, 0, offset), (0, 0, 0), (0, 11, 0))


def perspective_projection(aspect_ratio=1.0, znear=0.0001, zfar=10, fovy_degress=60) -> t.Tensor:
  """Perspective projection f32[4, 4] with y flipped, so that world-up lands at image row 0."""
  p = transformations.perspective_lh(float(fovy_degress) * math.pi / 180, aspect_ratio, znear, zfar)
  return t.matmul(transformations.scale((1, -1, 1)), p)


def get_ortho_matrix() -> t.Tensor:
  """Orthographic projection f32[4, 4] of the unit cube around the origin."""
  return transformations.ortho_lh(-0.5, 0.5, 0.5, -0.5, -0.5, 0.5)


def get_default_camera_for_mesh(vertex_positions) -> t.Tensor:
  """View-projection f32[4, 4] looking at the mesh f32[..., 3, 3] from above (the second tetrahedron camera), backed
  off by 0.7 of the box's largest extent."""
  v = t.as_tensor(vertex_positions, dtype=t.float32).detach().cpu()
  assert v.shape[-2:] == (3, 3)
  v = v.reshape(-1, 3)
  lo, hi = v.min(dim=0)[0], v.max(dim=0)[0]
  diagonal = (hi - lo).max()
  center = (lo + hi) / 2
  m = t.matmul(cameras_on_tetrahedron_vertices()[1], transformations.translate(-center))
  m = t.matmul(transformations.translate(t.stack([t.tensor(0.0), t.tensor(0.0), diagonal * 0.7])), m)
  proj = perspective_projection(1, zfar=diagonal * 3, znear=(diagonal + 10) / 1000)
  return t.matmul(proj, m)
