"""Homogeneous transforms used on the hot path's host side (geometry/transformations.py:25-58, 201-262).
Only what the model / voxelizer / super-resolution callers and the benchmark's camera need; plain torch host math."""
import math

import torch as t


def scale(v) -> t.Tensor:
  """Homogeneous scale matrix f32[N+1, N+1] from the scale vector v[N] (transformations.py:25-37)."""
  v = t.as_tensor(v, dtype=t.float32)
  return t.diag(t.cat([v, v.new_ones([1])], dim=0))


def translate(v) -> t.Tensor:
  """Homogeneous translation matrix f32[..., N+1, N+1] from v[..., N] (transformations.py:40-58)."""
  v = t.as_tensor(v, dtype=t.float32)
  n = v.shape[-1]
  result = t.eye(n + 1, dtype=t.float32, device=v.device).expand(v.shape[:-1] + (n + 1, n + 1)).clone()
  result[..., :n, n] = v
  return result


def look_at_rh(eye, center, up) -> t.Tensor:
  """Right-handed world->view matrix f32[4, 4] looking from `eye` at `center` (transformations.py:201-220):
  rows = (side, up', -forward) with the eye moved to the origin."""
  eye, center, up = (t.as_tensor(v, dtype=t.float32) for v in (eye, center, up))
  fwd = center - eye
  fwd = fwd / fwd.norm()
  side = t.linalg.cross(fwd, up)
  side = side / side.norm()
  rot = t.stack([side, t.linalg.cross(side, fwd), -fwd])
  m = t.eye(4, dtype=t.float32)
  m[:3, :3] = rot
  m[:3, 3] = -(rot @ eye)
  return m


def perspective_rh(fov_y: float, aspect: float, z_near: float, z_far: float) -> t.Tensor:
  """Right-handed OpenGL perspective projection f32[4, 4], depth to [-1, 1] (transformations.py:244-262)."""
  th = math.tan(fov_y / 2)
  m = t.zeros(4, 4, dtype=t.float32)
  m[0, 0] = 1.0 / (aspect * th)
  m[1, 1] = 1.0 / th
  m[2, 2] = -(z_far + z_near) / (z_far - z_near)
  m[2, 3] = -(2 * z_far * z_near) / (z_far - z_near)
  m[3, 2] = -1.0
  return m


def look_at_lh(eye, center, up) -> t.Tensor:
  """Left-handed world->view matrix f32[4, 4] looking from `eye` at `center` (transformations.py:180-198):
  rows = (side, up', forward) with forward = normalize(center - eye), side = normalize(up x forward)."""
  eye, center, up = (t.as_tensor(v, dtype=t.float32).cpu() for v in (eye, center, up))
  fwd = center - eye
  fwd = fwd / fwd.norm().clamp_min(1e-12)
  side = t.linalg.cross(up, fwd)
  side = side / side.norm().clamp_min(1e-12)
  rot = t.stack([side, t.linalg.cross(fwd, side), fwd])
  m = t.eye(4, dtype=t.float32)
  m[:3, :3] = rot
  m[:3, 3] = -(rot @ eye)
  return m


def perspective_lh(fov_y: float, aspect: float, z_near: float, z_far: float) -> t.Tensor:
  """Left-handed OpenGL perspective projection f32[4, 4], depth to [-1, 1], w = z_view (transformations.py:223-241)."""
  fov_y, aspect, z_near, z_far = (t.as_tensor(v, dtype=t.float32).cpu() for v in (fov_y, aspect, z_near, z_far))
  th = t.tan(fov_y / 2)
  m = t.zeros(4, 4, dtype=t.float32)
  m[0, 0] = 1.0 / (aspect * th)
  m[1, 1] = 1.0 / th
  m[2, 2] = (z_far + z_near) / (z_far - z_near)
  m[2, 3] = -(2 * z_far * z_near) / (z_far - z_near)
  m[3, 2] = 1.0
  return m


def ortho_lh(left, right, bottom, top, z_near, z_far) -> t.Tensor:
  """Left-handed orthographic projection f32[4, 4] of the box to [-1, 1]^3 (transformations.py:265-288)."""
  l, r, b, tp, n, f = (float(v) for v in (left, right, bottom, top, z_near, z_far))
  return t.tensor([[2 / (r - l), 0, 0, -(r + l) / (r - l)],
                   [0, 2 / (tp - b), 0, -(tp + b) / (tp - b)],
                   [0, 0, 2 / (f - n), -(f + n) / (f - n)],
                   [0, 0, 0, 1]], dtype=t.float32)


def chain(transforms) -> t.Tensor:
  """transforms[0] @ transforms[1] @ ... left to right (transformations.py:291-296)."""
  transforms = list(transforms)
  assert transforms
  result = transforms[0]
  for m in transforms[1:]:
    result = t.mm(result, m)
  return result


def transform_points_homogeneous(points, matrix, w: float) -> t.Tensor:
  """points f32[..., P, 3] -> homogeneous f32[..., P, 4] = matrix[..., 4, 4] . (p, w) (transformations.py:106-134)."""
  points = t.as_tensor(points, dtype=t.float32)
  matrix = t.as_tensor(matrix, dtype=t.float32, device=points.device)
  assert points.shape[-1] == 3 and matrix.shape[-2:] == (4, 4) and points.shape[:-2] == matrix.shape[:-2]
  ph = t.cat([points, points.new_full(points.shape[:-1] + (1,), float(w))], -1)
  return t.matmul(ph, matrix.transpose(-1, -2))


def transform_mesh(mesh, matrix, vertices_are_points: bool = True) -> t.Tensor:
  """mesh f32[..., T, 3, 3] through matrix f32[..., 4, 4]: points with the homogeneous divide, or vectors (w = 0)
  (transformations.py:137-166)."""
  mesh = t.as_tensor(mesh, dtype=t.float32)
  shape = mesh.shape
  assert shape[-2:] == (3, 3)
  flat = mesh.reshape(shape[:-3] + (shape[-3] * 3, 3))
  h = transform_points_homogeneous(flat, matrix, 1.0 if vertices_are_points else 0.0)
  out = h[..., :3] / h[..., 3:4] if vertices_are_points else h[..., :3]
  return out.reshape(shape)


def transform_points(points, matrix) -> t.Tensor:
  """points f32[..., P, 3] as points through matrix f32[..., 4, 4], with the homogeneous divide (:169-173)."""
  h = transform_points_homogeneous(points, matrix, 1.0)
  return h[..., :3] / h[..., 3:4]
