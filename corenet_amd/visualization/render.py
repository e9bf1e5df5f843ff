"""Rendering of triangle soups and voxel grids (reference: visualization/scene_renderer.py, voxel_renderer.py and their
GLSL shaders, drawn there through OpenGL on an EGL context).  Here a software renderer draws many images in one call:
CUDA(HIP) tensors run the kernels of csrc/render.hip, CPU tensors the library's host twin (csrc/render_cpu.cpp).  Both
give identical images when no material has a specular term (powf may differ by one level otherwise); a CUDA tensor
never goes to the host twin.

Contract, GL's rules for one draw of triangles without MSAA:
  * clip = VP . (p, 1); window x = (x_ndc + 1) / 2 * W, y = (y_ndc + 1) / 2 * H; image row r, column c samples the
    pixel centre (c + 0.5, r + 0.5), so row 0 is NDC y = -1 (GL's read-back order, not flipped).
    camera_util.perspective_projection flips y, which puts world-up at row 0.
  * Coverage: homogeneous edge functions with a top-left rule on exact zeros, so shared edges leave no holes and no
    pixel twice.  Only the part of a triangle in front of the eye (w > 0) covers pixels; there is no wrap-around.
    A fragment survives iff z_ndc, linear in screen space, is in [-1, 1] (NaN never survives).
  * Depth: GL LESS_EQUAL in submission order, i.e. the nearest fragment wins and on equal depth the later triangle.
  * Attributes (position, normal) are interpolated perspective-correct.
  * Shading, point_light_illumination.frag: N = normalize(normal), L = normalize(light - pos),
    V = -normalize(cam - pos), R = L - 2 dot(N, L) N; colour = ambient + diffuse |dot(N, L)| light_colour +
    ambient_light diffuse + specular light_colour max(dot(R, V), 0)^shininess, clamped to [0, 1], rint(255 c).
    Uncovered pixels get the clear colour.
  * cam = inverse(VP) . (0, 0, -1, 1), dehomogenised, in float32 on the host; the light defaults to it.
  * Diffuse textures (the fragment shader's `diffuse * texture(textures, (s, t, layer))` on a texture array with GL's
    defaults: GL_LINEAR, no mip-maps, GL_REPEAT, unsigned-normalised bytes).  (s, t) is interpolated perspective-correct
    like position.  Per axis of n texels: s' = s - floor(s) (0 if that is not in [0, 1): NaN, infinity); u = s' n - 0.5;
    i0 = floor(u), i1 = i0 + 1 with weight a = u - i0, and -1 wraps to n - 1, n to 0.  A texel channel is byte / 255;
    tau = lerp(lerp(c00, c10, a), lerp(c01, c11, a), b) with lerp(x, y, w) = x + w (y - x), so equal texels come back
    unchanged and an all-255 texture is the untextured image bit for bit.  Texture row 0 is t = 0 (GL's first row, which
    is why load_textures flips images).  Material m is textured iff 0 <= texture_indices[m] < L; its diffuse colour is
    then diffuse * tau in the formula above.  Only the winning fragment of a pixel samples.
"""
from __future__ import annotations

import ctypes as C
import io
from typing import Iterable, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch as t

from corenet_amd.geometry import transformations
from corenet_amd.visualization import camera_util
from corenet_amd.visualization.colors import DEFAULT_COLOR_PALETTE

TILE = 16
_IMAGE_WORDS = 40      # sizeof(crnRenderImage) / 4 (include/corenet_hip.h)


def _lib():
  from corenet_amd import _lib as L
  return L.lib()


def _host(v, dtype=t.float32) -> t.Tensor:
  return t.as_tensor(v, dtype=dtype).detach().cpu()


def camera_position(view_projection) -> t.Tensor:
  """The eye of a view-projection matrix f32[4, 4]: inverse(VP) . (0, 0, -1, 1), dehomogenised (host float32)."""
  c = t.mv(t.inverse(_host(view_projection)), t.tensor([0, 0, -1, 1], dtype=t.float32))
  return c[:3] / c[3]


def _rows(v, n: int, k: int, name: str) -> t.Tensor:
  v = _host(v)
  if v.dim() == 1:
    v = v.expand(n, v.shape[0])
  if tuple(v.shape) != (n, k):
    raise ValueError(f"render: {name} must be [{k}] or [{n}, {k}], got {tuple(v.shape)}")
  return v


def make_materials(diffuse, ambient=0.05, specular=(0.0, 0.0, 0.0), shininess=2048.0) -> t.Tensor:
  """Material table f32[M, 10] (ambient 3, diffuse 3, specular 3, shininess) from diffuse f32[M, 3]; the others are
  [3] / [M, 3] (ambient, specular) and a scalar or [M] (shininess)."""
  d = _host(diffuse).reshape(-1, 3)
  M = d.shape[0]
  a = _host(ambient)
  a = a.expand(M, 3) if a.dim() == 0 else _rows(a, M, 3, "ambient")
  s = _rows(specular, M, 3, "specular")
  sh = _host(shininess).reshape(-1).expand(M) if _host(shininess).numel() == 1 else _host(shininess).reshape(M)
  return t.cat([a, d, s, sh[:, None]], 1).contiguous()


class _Textures(NamedTuple):
  coords: Optional[t.Tensor]   # f32 [T, 3, 2] on the render device, or None (all zero)
  ids: t.Tensor                # int32 [M]
  texels: t.Tensor             # uint8 [L, Ht, Wt, 4], RGBA8

  def abi(self):
    L, Ht, Wt = self.texels.shape[:3]
    return (None if self.coords is None else self.coords.data_ptr(), self.ids.data_ptr(), self.texels.data_ptr(),
            L, Ht, Wt)


def _texture_args(tex_coords, textures, texture_indices, T: int, M: int, dev) -> Optional[_Textures]:
  """Checks render_batch's texture arguments and brings them to the C ABI's layout on dev; None: nothing is textured."""
  if tex_coords is not None:
    tex_coords = t.as_tensor(tex_coords)
    if tex_coords.dtype != t.float32 or tuple(tex_coords.shape) != (T, 3, 2):
      raise ValueError(f"render: tex_coords must be float32 [{T}, 3, 2], got {tex_coords.dtype} "
                       f"{tuple(tex_coords.shape)}")
  if (textures is None) != (texture_indices is None):
    raise ValueError("render: textures and texture_indices come together")
  if textures is None:
    return None
  textures = t.as_tensor(textures)
  if textures.dtype != t.uint8 or textures.dim() != 4 or textures.shape[3] != 3 or 0 in textures.shape:
    raise ValueError(f"render: textures must be a non-empty uint8 [L, Ht, Wt, 3], got {textures.dtype} "
                     f"{tuple(textures.shape)}")
  if max(textures.shape[:3]) > 1 << 14:
    raise ValueError("render: at most 2^14 texture layers, rows and columns")
  ids = t.as_tensor(texture_indices).detach().cpu()
  if ids.dtype not in (t.int8, t.int16, t.int32, t.int64, t.uint8) or tuple(ids.shape) != (M,):
    raise ValueError(f"render: texture_indices must be an integer [{M}], got {ids.dtype} {tuple(ids.shape)}")
  if M and int(ids.max()) >= textures.shape[0]:
    raise ValueError(f"render: texture index {int(ids.max())} with {textures.shape[0]} texture layers")
  if M == 0 or int(ids.max()) < 0:
    return None
  textures = textures.to(dev)
  texels = t.cat([textures, t.full_like(textures[..., :1], 255)], -1).contiguous()      # RGBA8: one load per texel
  return _Textures(None if tex_coords is None else tex_coords.to(dev).contiguous(), ids.to(dev, t.int32).contiguous(),
                   texels)


def _triangles(triangles) -> t.Tensor:
  triangles = t.as_tensor(triangles, dtype=t.float32).contiguous()
  if triangles.dim() != 3 or triangles.shape[1:] != (3, 3):
    raise ValueError(f"render: triangles must be [T, 3, 3], got {tuple(triangles.shape)}")
  return triangles


def _ranges_and_cameras(ranges, view_projections, H: int, W: int, T: int) -> Tuple[t.Tensor, t.Tensor]:
  """The checked triangle ranges int64 [I, 2] and view-projections f32 [I, 4, 4] of a render call, on the host."""
  ranges = _host(ranges, t.int64).reshape(-1, 2)
  I = ranges.shape[0]
  if I < 1 or H < 1 or W < 1:
    raise ValueError("render: need at least one image of positive size")
  if (ranges[:, 0] < 0).any() or (ranges[:, 1] < ranges[:, 0]).any() or (ranges[:, 1] > T).any() or T >= 1 << 31:
    raise ValueError("render: every range must satisfy 0 <= t0 <= t1 <= T < 2^31")
  return ranges, _host(view_projections).reshape(I, 4, 4)


def _image_records(ranges: t.Tensor, vps: t.Tensor, cull_back_facing) -> Tuple[np.ndarray, int, int]:
  """crnRenderImage[I] as float32 words with the fields every raster call reads (vp, cull, t0, t1, inst0) filled in and
  the rest zero, the number of (image, triangle) pairs and the longest range."""
  I = ranges.shape[0]
  cull = _host(cull_back_facing, t.int64).reshape(-1).expand(I)
  lens = ranges[:, 1] - ranges[:, 0]
  inst0 = t.cumsum(lens, 0) - lens
  num_inst = int(lens.sum())
  if num_inst >= 1 << 31:
    raise ValueError("render: at most 2^31 - 1 (image, triangle) pairs per call")
  rec = np.zeros((I, _IMAGE_WORDS), np.float32)
  rec[:, :16] = vps.reshape(I, 16).numpy()
  ints = rec.view(np.int32)
  ints[:, 31] = cull.numpy()
  ints[:, 33] = ranges[:, 0].numpy()
  ints[:, 34] = ranges[:, 1].numpy()
  ints[:, 35] = inst0.numpy()
  return rec, num_inst, int(lens.max())


def _bin(lib, triangles: t.Tensor, images: t.Tensor, I: int, H: int, W: int, max_len: int, num_inst: int):
  """crn_render_bin on the triangles' device -> (images there, records, counts, offsets, the sized tile lists, stream)."""
  from corenet_amd import _lib as L
  dev = triangles.device
  images = images.to(dev)
  ntiles = ((H + TILE - 1) // TILE) * ((W + TILE - 1) // TILE)
  records = t.empty((max(num_inst, 1), 16), dtype=t.float32, device=dev)
  counts = t.empty(I * ntiles, dtype=t.int32, device=dev)
  offsets = t.empty(I * ntiles + 1, dtype=t.int64, device=dev)
  s = L.stream()
  lib.crn_render_bin(triangles.data_ptr(), images.data_ptr(), I, H, W, max_len, num_inst, records.data_ptr(),
                     counts.data_ptr(), offsets.data_ptr(), s)
  total = int(offsets[-1].item())                                       # the call's one synchronisation
  bins = t.empty(max(total, 1), dtype=t.int32, device=dev)
  return images, records, counts, offsets, bins, s


def render_batch(triangles: t.Tensor, material_ids: t.Tensor, materials: t.Tensor, ranges, view_projections,
                 image_size: Tuple[int, int], normals: Optional[t.Tensor] = None, normal_modes=None,
                 light_positions=None, light_colors=(1.0, 1.0, 1.0), ambient_light_colors=(0.2, 0.2, 0.2),
                 clear_colors=(0.0, 0.0, 0.0), cull_back_facing=False, *, tex_coords: Optional[t.Tensor] = None,
                 textures: Optional[t.Tensor] = None, texture_indices=None) -> t.Tensor:
  """Renders I images of image_size = (H, W) in one call -> uint8 [I, H, W, 3] on the triangles' device.

  Image i draws triangles ranges[i] = [t0, t1) of the shared buffers: triangles f32 [T, 3, 3] (world space),
  material_ids int32 [T] into materials f32 [M, 10] (make_materials; an id outside [0, M) shades black) and normals
  f32 [T, 3, 3] (optional).  normal_modes[i]: 1 = interpolate the per-vertex normals, 2 = flat, normals[t, 0], 0 = the
  geometric normal normalize(cross(normalize(v1 - v0), normalize(v2 - v0))); default 1 with normals, 0 without.
  view_projections [I, 4, 4]; light_positions None (each image's camera) or [I, 3]; light_colors,
  ambient_light_colors, clear_colors [3] or [I, 3]; cull_back_facing a bool or [I] (culls when the signed NDC area is
  <= 0).  Diffuse textures (module docstring): textures uint8 [L, Ht, Wt, 3] (row 0 is t = 0) with texture_indices
  int [M], the layer of each material or -1 for none, and tex_coords f32 [T, 3, 2] (None: all (0, 0)); textures and
  texture_indices come together, tex_coords alone has no effect.  Wrong shapes or types and an index >= L raise
  ValueError before anything is launched.  On the GPU the call synchronises once: a read of the number of
  (tile, triangle) pairs."""
  H, W = (int(v) for v in image_size)
  dev = triangles.device
  triangles = _triangles(triangles)
  T = triangles.shape[0]
  material_ids = t.as_tensor(material_ids).to(dev, t.int32).contiguous()
  materials = t.as_tensor(materials, dtype=t.float32).to(dev).contiguous()
  if material_ids.shape != (T,) or materials.dim() != 2 or materials.shape[1] != 10:
    raise ValueError("render: material_ids must be [T] and materials [M, 10]")
  if normals is not None:
    normals = t.as_tensor(normals, dtype=t.float32).to(dev).contiguous()
    if normals.shape != triangles.shape:
      raise ValueError("render: normals must have the triangles' shape")
  tex = _texture_args(tex_coords, textures, texture_indices, T, materials.shape[0], dev)
  ranges, vps = _ranges_and_cameras(ranges, view_projections, H, W, T)
  I = ranges.shape[0]
  if normal_modes is None:
    normal_modes = t.full((I,), 1 if normals is not None else 0, dtype=t.int64)
  normal_modes = _host(normal_modes, t.int64).reshape(-1).expand(I)
  if normals is None and bool((normal_modes != 0).any()):
    raise ValueError("render: normal modes 1 and 2 need normals")
  cams = t.stack([camera_position(vps[i]) for i in range(I)])
  lights = cams if light_positions is None else _rows(light_positions, I, 3, "light_positions")
  rec, num_inst, max_len = _image_records(ranges, vps, cull_back_facing)
  rec[:, 16:19] = lights.numpy()
  rec[:, 19:22] = cams.numpy()
  rec[:, 22:25] = _rows(light_colors, I, 3, "light_colors").numpy()
  rec[:, 25:28] = _rows(ambient_light_colors, I, 3, "ambient_light_colors").numpy()
  rec[:, 28:31] = _rows(clear_colors, I, 3, "clear_colors").numpy()
  rec.view(np.int32)[:, 32] = normal_modes.numpy()
  images = t.from_numpy(rec)
  M = materials.shape[0]
  lib = _lib()
  if dev.type == "cuda":
    images, records, counts, offsets, bins, s = _bin(lib, triangles, images, I, H, W, max_len, num_inst)
    out = t.empty((I, H, W, 3), dtype=t.uint8, device=dev)
    if tex is None:
      lib.crn_render_raster(triangles.data_ptr(), None if normals is None else normals.data_ptr(),
                            material_ids.data_ptr(), materials.data_ptr(), M, images.data_ptr(), I, H, W, max_len,
                            records.data_ptr(), counts.data_ptr(), offsets.data_ptr(), bins.data_ptr(), out.data_ptr(), s)
    else:
      lib.crn_render_raster_tex(triangles.data_ptr(), None if normals is None else normals.data_ptr(),
                                material_ids.data_ptr(), materials.data_ptr(), M, images.data_ptr(), I, H, W, max_len,
                                records.data_ptr(), counts.data_ptr(), offsets.data_ptr(), bins.data_ptr(),
                                out.data_ptr(), *tex.abi(), s)
    return out
  if dev.type != "cpu":
    raise ValueError(f"render: unsupported device {dev}")
  out = t.empty((I, H, W, 3), dtype=t.uint8)
  if tex is None:
    lib.crn_render_cpu(triangles.data_ptr(), None if normals is None else normals.data_ptr(), material_ids.data_ptr(),
                       materials.data_ptr(), M, images.data_ptr(), I, H, W, out.data_ptr(), t.get_num_threads())
  else:
    lib.crn_render_cpu_tex(triangles.data_ptr(), None if normals is None else normals.data_ptr(),
                           material_ids.data_ptr(), materials.data_ptr(), M, images.data_ptr(), I, H, W, out.data_ptr(),
                           *tex.abi(), t.get_num_threads())
  return out


GEOMETRY_OUTPUTS = ("triangle_index", "barycentrics", "depth", "z_ndc")


class GeometryBuffers(NamedTuple):
  """What the raster stage decides per pixel (render_geometry); an output that was not asked for is None."""
  triangle_index: Optional[t.Tensor]   # int32 [I, H, W]: index into the call's triangles, -1 on background
  barycentrics: Optional[t.Tensor]     # f32 [I, H, W, 3]: perspective-correct weights of the winner's vertices, 0 on background
  depth: Optional[t.Tensor]            # f32 [I, H, W]: clip-space w of the fragment, +inf on background
  z_ndc: Optional[t.Tensor]            # f32 [I, H, W]: the depth-test value in [-1, 1], +inf on background

  @property
  def mask(self) -> t.Tensor:
    """bool [I, H, W]: the pixels a triangle covers (the silhouette)."""
    if self.triangle_index is None:
      raise ValueError("render: mask needs the triangle_index output")
    return self.triangle_index >= 0


def render_geometry(triangles: t.Tensor, ranges, view_projections, image_size: Tuple[int, int], cull_back_facing=False,
                    *, outputs: Sequence[str] = GEOMETRY_OUTPUTS) -> GeometryBuffers:
  """The geometry of I images of image_size = (H, W) instead of their colour -> GeometryBuffers on the triangles' device.

  triangles, ranges, view_projections and cull_back_facing are render_batch's, with the same checks.  Every pixel's
  winner is the triangle render_batch shades there (module docstring: coverage, z_ndc in [-1, 1], nearest, the later
  triangle on equal depth).  outputs names the tensors to compute, any non-empty subset of GEOMETRY_OUTPUTS:
    triangle_index  the winner's index into triangles (not relative to the image's range); -1 on background
    barycentrics    b_i = E_i / (E0 + E1 + E2), the weights render_batch interpolates position and texture
                    coordinates with; they sum to 1 up to rounding; 0 on background
    depth           the fragment's clip-space w, sum b_i w_i; for transformations.perspective_lh / perspective_rh
                    projections (camera_util.perspective_projection, the dataset's camera_transform) that is the
                    distance from the eye along the view axis; +inf on background
    z_ndc           the value of the depth test; +inf on background
  The GPU kernel and the host twin agree bit for bit on all four.  On the GPU the call synchronises once, as
  render_batch does."""
  H, W = (int(v) for v in image_size)
  dev = triangles.device
  triangles = _triangles(triangles)
  outputs = tuple(outputs)
  unknown = [o for o in outputs if o not in GEOMETRY_OUTPUTS]
  if unknown or not outputs:
    raise ValueError(f"render: outputs must be a non-empty subset of {GEOMETRY_OUTPUTS}, got {outputs}")
  ranges, vps = _ranges_and_cameras(ranges, view_projections, H, W, triangles.shape[0])
  I = ranges.shape[0]
  rec, num_inst, max_len = _image_records(ranges, vps, cull_back_facing)
  images = t.from_numpy(rec)
  if dev.type not in ("cuda", "cpu"):
    raise ValueError(f"render: unsupported device {dev}")
  shapes = {"triangle_index": ((I, H, W), t.int32), "barycentrics": ((I, H, W, 3), t.float32),
            "depth": ((I, H, W), t.float32), "z_ndc": ((I, H, W), t.float32)}
  out = {o: (t.empty(shapes[o][0], dtype=shapes[o][1], device=dev) if o in outputs else None) for o in GEOMETRY_OUTPUTS}
  ptrs = [None if out[o] is None else out[o].data_ptr() for o in GEOMETRY_OUTPUTS]
  lib = _lib()
  if dev.type == "cuda":
    images, records, counts, offsets, bins, s = _bin(lib, triangles, images, I, H, W, max_len, num_inst)
    lib.crn_render_raster_geometry(triangles.data_ptr(), images.data_ptr(), I, H, W, max_len, records.data_ptr(),
                                   counts.data_ptr(), offsets.data_ptr(), bins.data_ptr(), *ptrs, s)
  else:
    lib.crn_render_cpu_geometry(triangles.data_ptr(), images.data_ptr(), I, H, W, *ptrs, t.get_num_threads())
  return GeometryBuffers(**out)


def _on_pixels(buffers: GeometryBuffers, what: str):
  if buffers.triangle_index is None:
    raise ValueError(f"render: {what} needs the triangle_index output")
  covered = buffers.triangle_index >= 0
  return covered, buffers.triangle_index.clamp(min=0).to(t.int64)


def gather_triangle_attribute(buffers: GeometryBuffers, per_triangle: t.Tensor, fill) -> t.Tensor:
  """per_triangle [T, ...] (one entry per triangle of the render_geometry call) -> [I, H, W, ...]: the entry of every
  pixel's triangle, `fill` on background.  Label images (voxel_faces' material_ids are material_base + label), object
  ids, flat normals."""
  covered, index = _on_pixels(buffers, "gather_triangle_attribute")
  per_triangle = t.as_tensor(per_triangle).to(index.device)
  if per_triangle.dim() < 1 or (per_triangle.shape[0] == 0 and bool(covered.any())):
    raise ValueError(f"render: per_triangle must be [T, ...], got {tuple(per_triangle.shape)}")
  out = t.empty(tuple(index.shape) + tuple(per_triangle.shape[1:]), dtype=per_triangle.dtype, device=index.device)
  out[...] = fill
  out[covered] = per_triangle[index[covered]]
  return out


def interpolate_vertex_attribute(buffers: GeometryBuffers, per_vertex: t.Tensor, fill) -> t.Tensor:
  """per_vertex [T, 3, K] -> [I, H, W, K]: sum_i b_i a_i at every covered pixel (perspective-correct), `fill` on
  background.  View-space positions (per_vertex = triangles), smooth normals, texture coordinates."""
  covered, index = _on_pixels(buffers, "interpolate_vertex_attribute")
  if buffers.barycentrics is None:
    raise ValueError("render: interpolate_vertex_attribute needs the barycentrics output")
  per_vertex = t.as_tensor(per_vertex).to(index.device)
  if per_vertex.dim() != 3 or per_vertex.shape[1] != 3:
    raise ValueError(f"render: per_vertex must be [T, 3, K], got {tuple(per_vertex.shape)}")
  out = t.empty(tuple(index.shape) + (per_vertex.shape[2],), dtype=per_vertex.dtype, device=index.device)
  out[...] = fill
  b = buffers.barycentrics[covered].to(per_vertex.dtype)[:, :, None]
  a = per_vertex[index[covered]]
  out[covered] = (b[:, 0] * a[:, 0] + b[:, 1] * a[:, 1]) + b[:, 2] * a[:, 2]
  return out


class VoxelFaces(NamedTuple):
  triangles: t.Tensor      # f32 [T, 3, 3], view space
  normals: t.Tensor        # f32 [T, 3, 3], the face's flat normal three times
  material_ids: t.Tensor   # int32 [T], material_base + label
  num_triangles: t.Tensor  # int64 [N]
  boxes: Optional[t.Tensor]  # f32 [N, 2, 3] or None


def voxel_faces(labels, palette, matrices, material_base: int = 0, box_matrices=None) -> VoxelFaces:
  """The triangles the voxel renderer draws for N label grids labels [N, D, H, W] (voxel_renderer.geom).

  Voxel (x, y, z) = (w, h, d) is the unit cube [x, x + 1] x [y, y + 1] x [z, z + 1] iff palette[label] (f32 [P, 3])
  exists and has no negative channel; it goes through matrices[n] (f32 [N, 4, 4] or [4, 4], voxel -> view, no
  homogeneous divide).  Faces come in the order +x, -x, +y, -y, +z, -z, each as the quad (center, dy, dx) of the
  shader split into the strip's two triangles (v0, v1, v2), (v2, v1, v3); the flat normal is
  normalize(cross(dx', dy')) after the transform.  Deliberate difference from the reference, which emits all six
  faces of every voxel: only faces whose neighbour is not drawn (or outside the grid) are emitted, in the reference's
  order.  A face between two drawn voxels is hidden behind a nearer face from every eye outside the solid, so the
  images agree while the triangle count drops by about the solid's volume / surface ratio.

  box_matrices (f32 [N, 4, 4], optional): also returns, per grid, the bounds [2, 3] of the centres (x, y, z) + 0.5 of
  the voxels with label != 0 transformed as points (VoxelGridArtifact.get_3d_box; zeros if there are none).
  On the GPU the call synchronises once (the per-grid counts)."""
  labels = t.as_tensor(labels)
  if labels.dim() != 4 or any(s == 0 for s in labels.shape):
    raise ValueError(f"voxel_faces: labels must be a non-empty [N, D, H, W], got {tuple(labels.shape)}")
  dev = labels.device
  labels = labels.to(t.int32).contiguous()
  N, D, H, W = labels.shape
  pal = t.as_tensor(palette, dtype=t.float32).to(dev).reshape(-1, 3).contiguous()
  mats = t.as_tensor(matrices, dtype=t.float32).to(dev)
  mats = (mats.expand(N, 4, 4) if mats.shape == (4, 4) else mats).contiguous()
  if tuple(mats.shape) != (N, 4, 4):
    raise ValueError(f"voxel_faces: matrices must be [N, 4, 4] or [4, 4], got {tuple(mats.shape)}")
  bm = None
  if box_matrices is not None:
    bm = t.as_tensor(box_matrices, dtype=t.float32).to(dev)
    bm = (bm.expand(N, 4, 4) if bm.shape == (4, 4) else bm).contiguous()
  P = pal.shape[0]
  lib = _lib()
  if dev.type == "cuda":
    from corenet_amd import _lib as L
    from corenet_amd.backend import default_backend
    n = lib.crn_voxel_faces_workspace_bytes(N, D, H, W)
    ws = default_backend().workspace("vxf", n, dev)
    counts = t.empty(N, dtype=t.int64, device=dev)
    boxes = t.empty((N, 2, 3), dtype=t.float32, device=dev) if bm is not None else None
    s = L.stream()
    lib.crn_voxel_faces_count(labels.data_ptr(), N, D, H, W, pal.data_ptr(), P, None if bm is None else bm.data_ptr(),
                              None if boxes is None else boxes.data_ptr(), ws.data_ptr(), n, counts.data_ptr(), s)
    T = int(counts.sum().item())                                        # the call's one synchronisation
    tri = t.empty((T, 3, 3), dtype=t.float32, device=dev)
    nrm = t.empty((T, 3, 3), dtype=t.float32, device=dev)
    mid = t.empty(T, dtype=t.int32, device=dev)
    if T:
      lib.crn_voxel_faces_emit(labels.data_ptr(), N, D, H, W, pal.data_ptr(), P, mats.data_ptr(), int(material_base),
                               ws.data_ptr(), n, tri.data_ptr(), nrm.data_ptr(), mid.data_ptr(), s)
    return VoxelFaces(tri, nrm, mid, counts, boxes)
  if dev.type != "cpu":
    raise ValueError(f"voxel_faces: unsupported device {dev}")
  nt = t.get_num_threads()
  counts = t.empty(N, dtype=t.int64)
  boxes = t.empty((N, 2, 3), dtype=t.float32) if bm is not None else None
  lib.crn_voxel_faces_cpu(labels.data_ptr(), N, D, H, W, pal.data_ptr(), P, None if bm is None else bm.data_ptr(),
                          None if boxes is None else boxes.data_ptr(), None, 0, counts.data_ptr(), None, None, None, nt)
  T = int(counts.sum())
  tri = t.empty((T, 3, 3), dtype=t.float32)
  nrm = t.empty((T, 3, 3), dtype=t.float32)
  mid = t.empty(T, dtype=t.int32)
  if T:
    lib.crn_voxel_faces_cpu(labels.data_ptr(), N, D, H, W, pal.data_ptr(), P, None, None, mats.data_ptr(),
                            int(material_base), counts.data_ptr(), tri.data_ptr(), nrm.data_ptr(), mid.data_ptr(), nt)
  return VoxelFaces(tri, nrm, mid, counts, boxes)


def _finish(img: t.Tensor, output_type, return_rgb: bool = True) -> t.Tensor:
  if output_type != t.uint8:
    raise NotImplementedError("render: only uint8 output is supported")
  if not return_rgb:
    img = t.cat([img, t.full(img.shape[:-1] + (1,), 255, dtype=t.uint8, device=img.device)], -1)
  return img


def render_scene(vertex_positions, view_projection_matrix=None, image_size: Tuple[int, int] = (256, 256),
                 normals=None, material_ids=None, diffuse_coefficients=None, specular_coefficient=None,
                 ambient_coefficients=None, cull_back_facing=True, light_position=None, light_color=(1.0, 1.0, 1.0),
                 ambient_light_color=(0.2, 0.2, 0.2), clear_color=(0, 0, 0, 1), output_type=t.uint8,
                 return_rgb=True, *, tex_coords=None, diffuse_textures=None, diffuse_texture_indices=None) -> t.Tensor:
  """Renders triangles f32 [T, 3, 3] (scene_renderer.render_scene) -> uint8 [H, W, 3] on their device.  normals f32 [T, 3, 3] per vertex (normalised) or None (the geometric normal); material_ids int32 [T]
  (default all 0) into diffuse_coefficients [M, 3] (default 0.8), ambient_coefficients [M, 3] (default 0.05) and
  specular_coefficient [M, 4] (rgb + shininess, default (0, 0, 0, 2048)).  view_projection_matrix defaults to
  camera_util.get_default_camera_for_mesh; light_position to the camera.  tex_coords f32 [T, 3, 2] (default all 0),
  diffuse_textures uint8 [L, Ht, Wt, 3] and diffuse_texture_indices int [M] (default all -1) as in the reference: the
  indices are cut to the used materials and the textures to max(index) + 1 layers."""
  v = t.as_tensor(vertex_positions, dtype=t.float32)
  if v.dim() != 3 or v.shape[1:] != (3, 3):
    raise ValueError(f"render_scene: vertex_positions must be [T, 3, 3], got {tuple(v.shape)}")
  dev, T = v.device, v.shape[0]
  if view_projection_matrix is None:
    view_projection_matrix = camera_util.get_default_camera_for_mesh(v)
  vp = _host(view_projection_matrix)
  if material_ids is None:
    material_ids = t.zeros(T, dtype=t.int32)
  material_ids = t.as_tensor(material_ids).to(dev, t.int32)
  used = int(material_ids.max()) + 1 if T else 1

  def coeffs(arr, k, default):
    arr = t.ones(used, k) * t.tensor(default, dtype=t.float32) if arr is None else _host(arr)
    arr = arr[:used]
    if tuple(arr.shape) != (used, k):
      raise ValueError(f"render_scene: material coefficients must be [{used}, {k}], got {tuple(arr.shape)}")
    return arr

  diffuse = coeffs(diffuse_coefficients, 3, 0.8)
  ambient = coeffs(ambient_coefficients, 3, 0.05)
  spec = coeffs(specular_coefficient, 4, (0.0, 0.0, 0.0, 2048.0))
  mats = make_materials(diffuse, ambient, spec[:, :3], spec[:, 3])
  tex_ids = None
  if diffuse_textures is not None:
    tex_ids = t.full((used,), -1, dtype=t.int32) if diffuse_texture_indices is None else t.as_tensor(
        diffuse_texture_indices).detach().cpu()
    if tex_ids.dim() != 1 or tex_ids.shape[0] < used:
      raise ValueError(f"render_scene: diffuse_texture_indices must be [>= {used}], got {tuple(tex_ids.shape)}")
    tex_ids = tex_ids[:used]
    num_tex = max(int(tex_ids.max()) + 1, 1)
    diffuse_textures = t.as_tensor(diffuse_textures)
    if diffuse_textures.dim() != 4 or diffuse_textures.shape[0] < num_tex or diffuse_textures.shape[3] != 3:
      raise ValueError(f"render_scene: diffuse_textures must be [>= {num_tex}, Ht, Wt, 3], got "
                       f"{tuple(diffuse_textures.shape)}")
    diffuse_textures = diffuse_textures[:num_tex]
  elif diffuse_texture_indices is not None and int(t.as_tensor(diffuse_texture_indices)[:used].max()) >= 0:
    raise ValueError("render_scene: diffuse_texture_indices name a texture, but diffuse_textures is None")
  if tex_coords is not None:
    tex_coords = t.as_tensor(tex_coords, dtype=t.float32)
  img = render_batch(v, material_ids, mats.to(dev), [[0, T]], vp[None], image_size, normals=normals,
                     light_positions=None if light_position is None else _host(light_position)[None],
                     light_colors=light_color, ambient_light_colors=ambient_light_color,
                     clear_colors=_host(clear_color)[:3], cull_back_facing=bool(cull_back_facing),
                     tex_coords=tex_coords, textures=diffuse_textures, texture_indices=tex_ids)[0]
  return _finish(img, output_type, return_rgb)


def load_textures(encoded_images: Iterable[bytes], texture_size: Tuple[int, int]) -> Tuple[t.Tensor, t.Tensor]:
  """A texture array from encoded images (scene_renderer.load_textures) -> (uint8 [N, H, W, 3], int32 [num_images]).

  Every distinct non-empty entry of encoded_images (PNG, JPEG, ... bytes) is decoded once, converted to RGB, resized
  bicubically to texture_size = (H, W) and flipped along its rows, so that the image's bottom row is texture row 0
  (t = 0).  The second result maps entry j to its layer; an empty entry maps to -1.  With nothing to decode the array
  is zeros [1, 1, 1, 3]."""
  import PIL.Image
  height, width = (int(v) for v in texture_size)
  layer_of = {}
  layers, indices = [], []
  for enc in encoded_images:
    enc = bytes(enc)
    if not enc:
      indices.append(-1)
      continue
    if enc not in layer_of:
      layer_of[enc] = len(layers)
      with PIL.Image.open(io.BytesIO(enc)) as im:
        rgb = np.asarray(im.convert("RGB").resize((width, height), resample=PIL.Image.BICUBIC))
      layers.append(np.ascontiguousarray(rgb[::-1]))
    indices.append(layer_of[enc])
  array = t.from_numpy(np.stack(layers)) if layers else t.zeros((1, 1, 1, 3), dtype=t.uint8)
  return array, t.tensor(indices, dtype=t.int32)


def render_scenes(scenes, view_projections=None, image_size: Tuple[int, int] = (256, 256),
                  texture_size: Tuple[int, int] = (128, 128), device="cuda", shading_normals=True,
                  **light_and_clear_kwargs) -> t.Tensor:
  """Draws N data.scene.Scene objects, loaded with load_extra_fields=True, with their own materials and textures in
  one render_batch call -> uint8 [N, H, W, 3] on device.

  Every mesh goes through its o2w_transforms row (world space); with shading_normals its normals go through the
  inverse transpose of that row's 3 x 3 part, else the geometric normal is shaded.  All meshes share one material
  table (material_ids offset per mesh; diffuse from diffuse_colors, ambient and specular render_scene's defaults) and
  one texture array, load_textures over every mesh's diffuse_texture_pngs at texture_size.  Scene n is one triangle
  range; view_projections f32 [N, 4, 4] defaults to each scene's camera_transform @ view_transform.
  light_and_clear_kwargs: render_batch's light_positions, light_colors, ambient_light_colors, clear_colors,
  cull_back_facing."""
  extra = set(light_and_clear_kwargs) - {"light_positions", "light_colors", "ambient_light_colors", "clear_colors",
                                         "cull_back_facing"}
  if extra:
    raise TypeError(f"render_scenes: unexpected arguments {sorted(extra)}")
  scenes = list(scenes)
  if not scenes:
    raise ValueError("render_scenes: need at least one scene")
  tris, nrms, uvs, mids, diffuse, pngs, ranges = [], [], [], [], [], [], []
  num_tri = num_mat = 0
  for n, sc in enumerate(scenes):
    K = len(sc.mesh_vertices)
    fields = (sc.texcoords, sc.material_ids, sc.diffuse_colors, sc.diffuse_texture_pngs) + (
        (sc.normals,) if shading_normals else ())
    if any(len(f) != K for f in fields):
      raise ValueError(f"render_scenes: scene {n} lacks its per-mesh extra fields; load it with "
                       "load_from_npz(..., load_extra_fields=True)")
    t0 = num_tri
    for k in range(K):
      v = _host(sc.mesh_vertices[k]).reshape(-1, 3, 3)
      o2w = _host(sc.o2w_transforms[k])
      colors = _host(sc.diffuse_colors[k]).reshape(-1, 3)
      mesh_pngs = [bytes(p) for p in sc.diffuse_texture_pngs[k]]
      uv = _host(sc.texcoords[k])
      ids = _host(sc.material_ids[k], t.int64).reshape(-1)
      if len(mesh_pngs) != colors.shape[0] or tuple(uv.shape) != (v.shape[0], 3, 2) or ids.shape[0] != v.shape[0]:
        raise ValueError(f"render_scenes: scene {n}, mesh {k}: texcoords must be [T, 3, 2], material_ids [T], and "
                         "diffuse_texture_pngs needs one entry per row of diffuse_colors")
      tris.append(transformations.transform_mesh(v, o2w))
      if shading_normals:
        nm = _host(sc.normals[k]).reshape(-1, 3, 3)
        if nm.shape != v.shape:
          raise ValueError(f"render_scenes: scene {n}, mesh {k}: normals must have the vertices' shape")
        nrms.append(t.matmul(nm, t.inverse(o2w[:3, :3])))                 # rows times inverse == inverse transpose
      uvs.append(uv)
      mids.append(ids + num_mat)
      diffuse.append(colors)
      pngs += mesh_pngs
      num_mat += colors.shape[0]
      num_tri += v.shape[0]
    ranges.append([t0, num_tri])
  if view_projections is None:
    view_projections = t.stack([t.matmul(_host(sc.camera_transform), _host(sc.view_transform)) for sc in scenes])
  textures, tex_ids = load_textures(pngs, texture_size)
  dev = t.device(device)
  return render_batch(t.cat(tris).to(dev), t.cat(mids).to(t.int32).to(dev), make_materials(t.cat(diffuse)).to(dev),
                      ranges, view_projections, image_size, normals=t.cat(nrms).to(dev) if shading_normals else None,
                      tex_coords=t.cat(uvs).to(dev), textures=textures.to(dev), texture_indices=tex_ids,
                      **light_and_clear_kwargs)


def voxel_materials(palette) -> t.Tensor:
  """The voxel renderer's materials f32 [P, 10]: ambient 0, diffuse = palette, specular 0, shininess 1."""
  return make_materials(palette, 0.0, (0.0, 0.0, 0.0), 1.0)


def render_voxel_grid(voxel_grid, view_projection_matrix=None, image_size: Tuple[int, int] = (256, 256),
                      voxel_to_view_matrix=None, diffuse_coefficients=None, light_position=None,
                      light_color=(1.0, 1.0, 1.0), ambient_light_color=(0.2, 0.2, 0.2), clear_color=(0, 0, 0),
                      output_type=t.uint8) -> t.Tensor:
  """Renders a label grid int32 [D, H, W] as unit cubes (voxel_renderer.render_voxel_grid) -> uint8 [H, W, 3] on the
  grid's device.  Label l is drawn with diffuse_coefficients[l] (default DEFAULT_COLOR_PALETTE) unless that colour has
  a negative channel; ambient 0, no specular, no culling.  voxel_to_view_matrix defaults to scale(1 / max(shape)), the
  camera to get_default_camera_for_mesh of the grid's box.  Only exposed faces are drawn (see voxel_faces)."""
  g = t.as_tensor(voxel_grid)
  if g.dim() != 3:
    raise ValueError(f"render_voxel_grid: voxel_grid must be [D, H, W], got {tuple(g.shape)}")
  if voxel_to_view_matrix is None:
    d = 1.0 / max(g.shape)
    voxel_to_view_matrix = transformations.scale([d, d, d])
  v2v = _host(voxel_to_view_matrix)
  if view_projection_matrix is None:
    box = t.tensor([[[0.0] * 3, [0.0] * 3, [float(s) for s in g.shape[::-1]]]])
    view_projection_matrix = camera_util.get_default_camera_for_mesh(transformations.transform_mesh(box, v2v))
  if diffuse_coefficients is None:
    diffuse_coefficients = DEFAULT_COLOR_PALETTE
  pal = _host(diffuse_coefficients).reshape(-1, 3)
  f = voxel_faces(g[None], pal, v2v)
  img = render_batch(f.triangles, f.material_ids, voxel_materials(pal).to(g.device), [[0, f.triangles.shape[0]]],
                     _host(view_projection_matrix)[None], image_size, normals=f.normals, normal_modes=[2],
                     light_positions=None if light_position is None else _host(light_position)[None],
                     light_colors=light_color, ambient_light_colors=ambient_light_color,
                     clear_colors=_host(clear_color)[:3], cull_back_facing=False)[0]
  return _finish(img, output_type)
