"""Textured rendering checks shared by test_render_tex_cpu.py (host twin) and test_render_tex_gpu.py (HIP kernel).

A float64 numpy restatement of the texture rule (wrap, texel position, bilinear blend) for scenes in which one planar
quad (two triangles sharing a diagonal, an affine uv map) overfills the image, and the cases built on it.  It shares no
code with the product.  Every case takes `render`, a function with render_batch's signature that takes and returns host
tensors; the GPU tests pass one that runs the kernel and also compares it with the host twin bit for bit.

Shading is made trivial where the reference is used: material ambient 0, no specular, light_colors 0,
ambient_light_colors 1, so a pixel is rint(255 * clamp(diffuse * tau)).

Tolerance: every channel of every pixel within 1 level.  With textures of at most 16 x 16 and |uv| <= 1004 the float32
error of the texel position is below 16 * 1004 * 2^-22 < 4e-3 texels, that of tau (slope <= 1 per texel) below 1 / 255,
so the values before rint differ by less than one level and the rounded ones by at most one.  Bilinear filtering with
repeat wrap is continuous, so there is no other way for a value to move.  No pixel is left out."""
import io
import os

import numpy as np
import PIL.Image
import torch as t

import render_scenes as S

IDENTITY = np.eye(4, dtype=np.float32)


# ---------------------------------------------------------------- the float64 reference
def ref_axis(s, n):
  with np.errstate(invalid="ignore"):
    f = s - np.floor(s)
    f = np.where((f >= 0) & (f < 1), f, 0.0)
  u = f * n - 0.5
  i0 = np.floor(u)
  a = u - i0
  i0 = i0.astype(np.int64)
  i1 = i0 + 1
  return np.where(i0 < 0, n - 1, i0), np.where(i1 >= n, 0, i1), a


def ref_sample(tex, s, tt):
  """tex uint8 [Ht, Wt, 3] (row 0 is t = 0), s, tt float64 [...] -> tau float64 [..., 3]."""
  Ht, Wt = tex.shape[:2]
  c = tex.astype(np.float64) / 255.0
  i0, i1, a = ref_axis(np.asarray(s, np.float64), Wt)
  j0, j1, b = ref_axis(np.asarray(tt, np.float64), Ht)
  a, b = a[..., None], b[..., None]
  return (1 - a) * (1 - b) * c[j0, i0] + a * (1 - b) * c[j0, i1] + (1 - a) * b * c[j1, i0] + a * b * c[j1, i1]


def ref_quad_uv(vp, corners, uvs, H, W):
  """(s, t) float64 [H, W] at every pixel centre of a quad with corners [4, 3] (0-1-2-3 around, a parallelogram) and
  uvs [4, 2]: the eye ray through the pixel centre meets the quad's plane, the hit goes through the affine uv map."""
  vp = np.asarray(vp, np.float64)
  P = np.asarray(corners, np.float64)
  U = np.asarray(uvs, np.float64)
  x = (np.arange(W) + 0.5) / W * 2 - 1
  y = (np.arange(H) + 0.5) / H * 2 - 1
  X, Y = np.meshgrid(x, y)
  e1, e2 = P[1] - P[0], P[3] - P[0]
  nrm = np.cross(e1, e2)
  if np.array_equal(vp, np.eye(4)):
    o = np.stack([X, Y, np.zeros_like(X)], -1)                       # world = NDC: the ray runs along z
    d = np.broadcast_to(np.array([0.0, 0.0, 1.0]), o.shape)
  else:
    inv = np.linalg.inv(vp)

    def unproject(z):
      h = np.stack([X, Y, np.full_like(X, z), np.ones_like(X)], -1) @ inv.T
      return h[..., :3] / h[..., 3:]
    o = unproject(-1.0)
    d = unproject(1.0) - o
  k = ((P[0] - o) @ nrm) / (d @ nrm)
  hit = o + k[..., None] * d - P[0]
  # plane coordinates (alpha, beta): hit = alpha e1 + beta e2
  G = np.array([[e1 @ e1, e1 @ e2], [e1 @ e2, e2 @ e2]])
  ab = np.linalg.solve(G, np.stack([hit @ e1, hit @ e2], -1)[..., None])[..., 0]
  uv = U[0] + ab[..., :1] * (U[1] - U[0]) + ab[..., 1:] * (U[3] - U[0])
  return uv[..., 0], uv[..., 1]


def ref_quad_image(vp, corners, uvs, diffuse, tex, H, W):
  """The image int64 [H, W, 3] of the overfilling quad under the trivial shading; tex None: untextured."""
  d = np.asarray(diffuse, np.float64)
  if tex is None:
    col = np.broadcast_to(d, (H, W, 3))
  else:
    s, tt = ref_quad_uv(vp, corners, uvs, H, W)
    col = d * ref_sample(tex, s, tt)
  return np.rint(255.0 * np.clip(col, 0.0, 1.0)).astype(np.int64)


# ---------------------------------------------------------------- scenes
def quad(corners, uvs):
  """-> triangles f32 [2, 3, 3], tex_coords f32 [2, 3, 2]: (0, 1, 2) and (0, 2, 3), sharing the diagonal 0-2."""
  P, U = np.asarray(corners, np.float32), np.asarray(uvs, np.float32)
  idx = [0, 1, 2, 0, 2, 3]
  return t.from_numpy(P[idx].reshape(2, 3, 3).copy()), t.from_numpy(U[idx].reshape(2, 3, 2).copy())


def rect(x0, x1, y0, y1, z=0.0):
  return np.array([[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]], np.float32)


def rect_uv(s0, s1, t0, t1):
  return np.array([[s0, t0], [s1, t0], [s1, t1], [s0, t1]], np.float32)


def flat_materials(diffuse):
  """f32 [M, 10]: ambient 0, the diffuse colours, no specular."""
  d = t.as_tensor(diffuse, dtype=t.float32).reshape(-1, 3)
  m = t.zeros(d.shape[0], 10)
  m[:, 3:6] = d
  m[:, 9] = 1.0
  return m


FLAT = dict(light_colors=(0.0, 0.0, 0.0), ambient_light_colors=(1.0, 1.0, 1.0))


def random_texture(Ht, Wt, seed):
  return np.random.RandomState(seed).randint(0, 256, (Ht, Wt, 3)).astype(np.uint8)


def checker_texture(Ht, Wt, cell=1):
  j, i = np.meshgrid(np.arange(Ht) // cell, np.arange(Wt) // cell, indexing="ij")
  on = ((i + j) % 2).astype(np.uint8)
  return np.stack([on * 255, (1 - on) * 200 + 30, on * 90 + 10], -1).astype(np.uint8)


def assert_close(img, exp, what):
  d = np.abs(img.numpy().astype(np.int64) - exp)
  assert d.max() <= 1, (what, int(d.max()), int((d > 1).sum()))


TEX_SIZES = ((1, 1), (2, 3), (5, 7), (16, 16))          # (Ht, Wt)
UV_RANGES = {"unit": (0.0, 1.0, 0.0, 1.0), "wrap": (-2.25, 3.5, -2.25, 3.5),
             "plus1000": (1000.25, 1001.25, 1000.25, 1001.25), "minus1000": (-1002.5, -996.75, -1000.25, -999.25)}
DIFFUSE = (0.9, 0.5, 1.0)


# ---------------------------------------------------------------- cases
def case_orthographic(render, tex_size, uv_range, kind):
  """Case 1: identity view-projection, image 37 x 29 (no multiple of the 16-pixel tile), against the reference."""
  H, W = 29, 37
  Ht, Wt = tex_size
  tex = random_texture(Ht, Wt, 10 * Ht + Wt) if kind == "random" else checker_texture(Ht, Wt)
  corners, uvs = rect(-1.3, 1.7, -1.6, 1.2), rect_uv(*UV_RANGES[uv_range])
  tri, uv = quad(corners, uvs)
  img = render(tri, t.zeros(2, dtype=t.int32), flat_materials([DIFFUSE]), [[0, 2]], t.eye(4)[None], (H, W),
               tex_coords=uv, textures=t.from_numpy(tex)[None], texture_indices=t.tensor([0]), **FLAT)[0]
  assert_close(img, ref_quad_image(IDENTITY, corners, uv.numpy()[[0, 0, 0, 1], [0, 1, 2, 2]], DIFFUSE, tex, H, W),
               (tex_size, uv_range, kind))


def perspective_vp():
  from corenet_amd.visualization import camera_util as C
  return C.perspective_projection(1.0, znear=0.1, zfar=10)          # eye at the origin, looking along +z, fovy 60


def receding_quad():
  """A quad in the plane z = 1.6 + 1.2 x: it meets the image's side edges at z = 0.945 and 5.21, so clip w varies 5.5x."""
  c = np.array([[x, y, 1.6 + 1.2 * x] for x, y in ((-0.8, -3.5), (3.4, -3.5), (3.4, 3.5), (-0.8, 3.5))], np.float32)
  return c, rect_uv(0.0, 3.0, -1.0, 2.5)


def case_perspective(render):
  """Case 2: the receding quad with a 16 x 16 checker.  uv interpolated affinely in screen space would be off by whole
  texels here (checked below on the reference itself), so only perspective-correct interpolation passes."""
  H, W = 29, 37
  tex = checker_texture(16, 16, cell=2)
  corners, uvs = receding_quad()
  vp = perspective_vp()
  clip_w = (np.c_[corners, np.ones(4)] @ vp.numpy().astype(np.float64).T)[:, 3]
  assert clip_w.min() > 0
  s, tt = ref_quad_uv(vp.numpy(), corners, uvs, H, W)
  depth = 1.6 + 1.2 * s / 3.0 * 4.2 + 1.2 * -0.8                    # z = w of the hit, from s (s is affine in x)
  assert depth.max() / depth.min() >= 4
  affine_s = s[:, :1] + (s[:, -1:] - s[:, :1]) * np.linspace(0, 1, W)[None]
  assert np.abs(affine_s - s).max() * 16 > 4                        # a screen-space lerp is off by more than 4 texels
  tri, uv = quad(corners, uvs)
  img = render(tri, t.zeros(2, dtype=t.int32), flat_materials([DIFFUSE]), [[0, 2]], vp[None], (H, W), tex_coords=uv,
               textures=t.from_numpy(tex)[None], texture_indices=t.tensor([0]), **FLAT)[0]
  exp = ref_quad_image(vp.numpy(), corners, uvs, DIFFUSE, tex, H, W)
  assert_close(img, exp, "perspective")
  wrong = np.rint(255 * np.clip(np.array(DIFFUSE) * ref_sample(tex, affine_s, tt), 0, 1))
  assert (np.abs(wrong - exp) > 1).mean() > 0.2                     # the check tells the two apart


def case_row_orientation(render):
  """Case 3: texture row 0 (t = 0) lands where NDC y = -1 is, image row 0."""
  tex = np.zeros((2, 1, 3), np.uint8)
  tex[0, 0] = (255, 0, 0)
  tex[1, 0] = (0, 255, 0)
  tri, uv = quad(rect(-2, 2, -2, 2), rect_uv(-0.5, 1.5, -0.5, 1.5))    # (s, t) = (NDC + 1) / 2
  img = render(tri, t.zeros(2, dtype=t.int32), flat_materials([(1.0, 1.0, 1.0)]), [[0, 2]], t.eye(4)[None], (2, 5),
               tex_coords=uv, textures=t.from_numpy(tex)[None], texture_indices=t.tensor([0]), **FLAT)[0].numpy()
  # rows sample t = 0.25 and 0.75: the centres of texture rows 0 and 1
  assert (img[0] == (255, 0, 0)).all() and (img[1] == (0, 255, 0)).all(), img


def case_layers_and_materials(render):
  """Case 4: L = 3, four materials with texture_indices [-1, 2, 0, 2] in four strips of one image."""
  H, W = 24, 40
  texs = np.stack([random_texture(4, 6, 1), np.full((4, 6, 3), 7, np.uint8), checker_texture(4, 6)])
  ids = [-1, 2, 0, 2]
  diffuse = [(0.3, 0.6, 0.9), (1.0, 0.8, 0.6), (0.7, 0.7, 0.7), (0.2, 1.0, 0.5)]
  edges = [-1.5, -0.45, 0.02, 0.51, 1.5]
  tris, uvs, exp = [], [], np.zeros((H, W, 3), np.int64)
  x = (np.arange(W) + 0.5) / W * 2 - 1
  for k in range(4):
    corners, cuv = rect(edges[k], edges[k + 1], -1.2, 1.4), rect_uv(0.1 * k, 1.3 + k, -0.7, 0.9)
    a, b = quad(corners, cuv)
    tris.append(a)
    uvs.append(b)
    one = ref_quad_image(IDENTITY, corners, cuv, diffuse[k], None if ids[k] < 0 else texs[ids[k]], H, W)
    cols = (x >= edges[k]) & (x < edges[k + 1])
    assert not np.isclose(x, edges[k]).any()
    exp[:, cols] = one[:, cols]
  img = render(t.cat(tris), t.arange(4, dtype=t.int32).repeat_interleave(2), flat_materials(diffuse), [[0, 8]],
               t.eye(4)[None], (H, W), tex_coords=t.cat(uvs), textures=t.from_numpy(texs),
               texture_indices=t.tensor(ids), **FLAT)[0]
  assert_close(img, exp, "layers")
  assert (img[:, :10].numpy() == np.rint(255 * np.array(diffuse[0], np.float32))).all()      # the plain strip, exactly


def lit_cube(normals: bool):
  """The cube of render_scenes.py seen by its camera, default lights: render_batch's positional arguments + normals."""
  from corenet_amd.geometry import transformations as T
  from corenet_amd.visualization import render as R
  tri = S.cube_mesh()
  cam = t.matmul(T.perspective_rh(70 * np.pi / 180, 1, 0.1, 10.0), T.look_at_rh((-1.2, -1.5, -1), (0, 0, 0), (0, 1, 0)))
  rng = np.random.RandomState(5)
  mids = t.from_numpy(rng.randint(0, 3, 12).astype(np.int32))
  mats = R.make_materials(t.from_numpy(rng.rand(3, 3).astype(np.float32)))
  nrm = t.from_numpy((tri.numpy() - 0.5 + 0.1 * rng.randn(12, 3, 3)).astype(np.float32)) if normals else None
  return (tri, mids, mats, [[0, 12]], cam[None], (61, 45)), nrm


def render_cpu_abi(args, nrm):
  """The scene of lit_cube through crn_render_cpu itself, the entry point as it was before textures."""
  from corenet_amd import _lib as L
  from corenet_amd.visualization import render as R
  tri, mids, mats, ranges, vps, (H, W) = args
  rec = np.zeros((1, 40), np.float32)                               # crnRenderImage, include/corenet_hip.h
  rec[0, :16] = vps[0].reshape(16).numpy()
  cam = R.camera_position(vps[0]).numpy()
  rec[0, 16:19] = cam
  rec[0, 19:22] = cam
  rec[0, 22:25] = 1.0
  rec[0, 25:28] = 0.2
  ints = rec.view(np.int32)
  ints[0, 32] = 1 if nrm is not None else 0
  ints[0, 34] = tri.shape[0]
  out = t.empty((1, H, W, 3), dtype=t.uint8)
  L.lib().crn_render_cpu(tri.data_ptr(), None if nrm is None else nrm.data_ptr(), mids.data_ptr(), mats.data_ptr(),
                         mats.shape[0], rec.ctypes.data, 1, H, W, out.data_ptr(), 1)
  return out


def case_identities(render, normals):
  """Case 5: all-255 textures, indices all -1 and tex_coords alone leave the lit image bit for bit as it was."""
  args, nrm = lit_cube(normals)
  rng = np.random.RandomState(6)
  uv = t.from_numpy((rng.rand(12, 3, 2) * 7 - 3).astype(np.float32))
  plain = render(*args, normals=nrm)
  assert plain.any() and t.equal(plain, render_cpu_abi(args, nrm))
  white = t.full((2, 5, 3, 3), 255, dtype=t.uint8)
  assert t.equal(render(*args, normals=nrm, tex_coords=uv, textures=white, texture_indices=t.tensor([1, 0, 1])), plain)
  assert t.equal(render(*args, normals=nrm, textures=white, texture_indices=t.tensor([0, 0, 0])), plain)
  noise = t.from_numpy(rng.randint(0, 256, (2, 5, 3, 3)).astype(np.uint8))
  assert t.equal(render(*args, normals=nrm, tex_coords=uv, textures=noise, texture_indices=t.tensor([-1, -1, -1])), plain)
  assert t.equal(render(*args, normals=nrm, tex_coords=uv), plain)
  # and a texture that is not white does change the image
  assert not t.equal(render(*args, normals=nrm, tex_coords=uv, textures=noise, texture_indices=t.tensor([1, 0, 1])), plain)


def case_non_finite(render):
  """Case 6: NaN, infinite and huge coordinates sample like coordinate 0; the indices are in range by construction."""
  H, W = 20, 32
  tex = random_texture(5, 7, 3)
  lc, rc = rect(-1.5, 0.03, -1.5, 1.5), rect(0.03, 1.5, -1.5, 1.5)
  ruv = rect_uv(0.2, 2.7, -1.1, 0.6)
  (lt, luv), (rt, ruv_t) = quad(lc, rect_uv(0, 0, 0, 0)), quad(rc, ruv)
  bad = luv.clone()
  bad[0] = t.tensor([[float("nan"), 0.3], [0.2, float("inf")], [float("-inf"), 1e30]])
  bad[1] = t.tensor([[1e30, -1e30], [1e30, -1e30], [3e38, float("inf")]])
  kw = dict(textures=t.from_numpy(tex)[None], texture_indices=t.tensor([0]), **FLAT)
  args = (t.cat([lt, rt]), t.zeros(4, dtype=t.int32), flat_materials([DIFFUSE]), [[0, 4]], t.eye(4)[None], (H, W))
  img = render(*args, tex_coords=t.cat([bad, ruv_t]), **kw)[0]
  zero = render(*args, tex_coords=t.cat([luv, ruv_t]), **kw)[0]
  assert t.equal(img, zero)                                          # left: as at (0, 0); right: untouched
  x = (np.arange(W) + 0.5) / W * 2 - 1
  exp = ref_quad_image(IDENTITY, rc, ruv, DIFFUSE, tex, H, W)
  exp[:, x < 0.03] = ref_quad_image(IDENTITY, lc, rect_uv(0, 0, 0, 0), DIFFUSE, tex, H, W)[:, x < 0.03]
  assert_close(img, exp, "non-finite")
  # coordinate 0 is the even blend of the first and last texel of both axes
  c = tex.astype(np.float64)[[0, 0, -1, -1], [0, -1, 0, -1]].mean(0) / 255
  assert np.abs(img[3, 2].numpy() - np.rint(255 * np.array(DIFFUSE) * c)).max() <= 1


def case_batching(render):
  """Case 7: two images over different ranges of shared buffers and different cameras == the two single calls."""
  H, W = 29, 37
  texs = np.stack([checker_texture(16, 16, 2), random_texture(16, 16, 9)])
  c0, u0 = receding_quad()
  (t0, uv0), (t1, uv1) = quad(c0, u0), quad(rect(-1.3, 1.7, -1.6, 1.2), rect_uv(-2.25, 3.5, -2.25, 3.5))
  tri, uv = t.cat([t0, t1]), t.cat([uv0, uv1])
  mids = t.tensor([0, 0, 1, 1], dtype=t.int32)
  kw = dict(textures=t.from_numpy(texs), texture_indices=t.tensor([0, 1]), tex_coords=uv, **FLAT)
  mats = flat_materials([DIFFUSE, (1.0, 1.0, 0.4)])
  vps, ranges = t.stack([perspective_vp(), t.eye(4)]), [[0, 2], [2, 4]]
  both = render(tri, mids, mats, ranges, vps, (H, W), **kw)
  for i in range(2):
    assert t.equal(both[i], render(tri, mids, mats, [ranges[i]], vps[i:i + 1], (H, W), **kw)[0]), i
  assert_close(both[0], ref_quad_image(vps[0].numpy(), c0, u0, DIFFUSE, texs[0], H, W), "batch 0")
  assert not t.equal(both[0], both[1])


def case_validation(render):
  """Case 8: every ValueError of render_batch's texture arguments."""
  import pytest
  tri, uv = quad(rect(-2, 2, -2, 2), rect_uv(0, 1, 0, 1))
  args = (tri, t.zeros(2, dtype=t.int32), flat_materials([DIFFUSE, DIFFUSE]), [[0, 2]], t.eye(4)[None], (8, 8))
  tex, ids = t.zeros((2, 4, 4, 3), dtype=t.uint8), t.tensor([0, 1])
  bad = [dict(tex_coords=uv[:1]), dict(tex_coords=uv.reshape(2, 2, 3)), dict(tex_coords=uv.double()),
         dict(textures=tex), dict(texture_indices=ids),
         dict(textures=tex.float(), texture_indices=ids), dict(textures=tex[..., :2], texture_indices=ids),
         dict(textures=tex[0], texture_indices=ids), dict(textures=tex[:, :0], texture_indices=ids),
         dict(textures=tex, texture_indices=ids[:1]), dict(textures=tex, texture_indices=ids.float()),
         dict(textures=tex, texture_indices=ids[None]), dict(textures=tex, texture_indices=t.tensor([0, 2]))]
  for kw in bad:
    with pytest.raises(ValueError):
      render(*args, **kw)
  render(*args, tex_coords=uv, textures=tex, texture_indices=ids)


# ---------------------------------------------------------------- load_textures and render_scenes
def png_bytes(array) -> bytes:
  buf = io.BytesIO()
  PIL.Image.fromarray(array).save(buf, format="PNG")
  return buf.getvalue()


def case_load_textures(R):
  """Case 9: the reference's own test of load_textures, on the two golden renderings."""
  def read(name):
    enc = open(os.path.join(S.GOLDEN_RENDER, name), "rb").read()
    im = PIL.Image.open(io.BytesIO(enc)).convert("RGB").resize((192, 128), resample=PIL.Image.BICUBIC)
    return np.array(im)[::-1], enc
  (im_a, a), (im_b, b) = read("expected_image_mesh.png"), read("expected_image_voxels.png")
  arr, idx = R.load_textures([a, b, b"", a], (128, 192))
  assert arr.dtype == t.uint8 and tuple(arr.shape) == (2, 128, 192, 3) and arr.is_contiguous()
  assert idx.dtype == t.int32 and idx.tolist() == [0, 1, -1, 0]
  assert np.array_equal(arr[0].numpy(), im_a) and np.array_equal(arr[1].numpy(), im_b)
  top = np.array(PIL.Image.open(io.BytesIO(a)).convert("RGB").resize((192, 128), resample=PIL.Image.BICUBIC))[0]
  assert np.array_equal(arr[0, -1].numpy(), top) and im_a.any()      # the image's top row is the last texture row
  arr, idx = R.load_textures([b"", b""], (128, 192))
  assert arr.dtype == t.uint8 and tuple(arr.shape) == (1, 1, 1, 3) and not arr.any() and idx.tolist() == [-1, -1]
  arr, idx = R.load_textures([], (4, 4))
  assert tuple(arr.shape) == (1, 1, 1, 3) and tuple(idx.shape) == (0,) and idx.dtype == t.int32


def make_scenes():
  """Two Scenes of two meshes with two materials each (one textured by an in-memory PNG, one plain), non-trivial
  object-to-world transforms, and every extra field."""
  from corenet_amd.data.scene import Scene
  from corenet_amd.geometry import transformations as T
  from corenet_amd.visualization import camera_util as C
  rng = np.random.RandomState(11)
  pngs = [png_bytes(random_texture(9, 13, 20 + k)) for k in range(3)]
  scenes = []
  for n in range(2):
    verts, nrms, uvs, mids, cols, texs, o2w = [], [], [], [], [], [], []
    for k in range(2):
      v = S.cube_mesh() - 0.5
      verts.append(v)
      nrms.append(t.from_numpy((v.numpy() + 0.2 * rng.randn(12, 3, 3)).astype(np.float32)))
      uvs.append(t.from_numpy((rng.rand(12, 3, 2) * 3 - 1).astype(np.float32)))
      mids.append(t.from_numpy(rng.randint(0, 2, 12).astype(np.int32)))
      cols.append(t.from_numpy((0.3 + 0.7 * rng.rand(2, 3)).astype(np.float32)))
      texs.append([pngs[(n + k) % 3], b""] if k == 0 else [b"", pngs[(n + 2 * k) % 3]])
      ang = 0.5 + n + 2 * k
      rot = t.tensor([[np.cos(ang), 0, np.sin(ang), 0], [0, 1, 0, 0], [-np.sin(ang), 0, np.cos(ang), 0], [0, 0, 0, 1]],
                     dtype=t.float32)
      shear = t.eye(4)
      shear[0, 1] = 0.3
      m = T.translate((0.6 * k - 0.3, 0.1 * n, 0.2 * k)) @ rot @ shear @ T.scale((0.5, 0.3 + 0.2 * k, 0.4))
      o2w.append(m)
    view = T.look_at_lh((0.4 * n - 0.2, 0.5, -2.0), (0, 0, 0), (0, 1, 0))
    scenes.append(Scene(mesh_vertices=verts, view_transform=view, o2w_transforms=t.stack(o2w),
                        camera_transform=C.perspective_projection(1.0, znear=0.1, zfar=10),
                        mesh_labels=["a", "b"], mesh_visible_fractions=t.ones(2), opengl_image=t.zeros(1, 1, 3, dtype=t.uint8),
                        pbrt_image=t.zeros(1, 1, 3, dtype=t.uint8), normals=nrms, texcoords=uvs, material_ids=mids,
                        diffuse_colors=cols, diffuse_texture_pngs=texs))
  return scenes


def case_render_scenes(R, device, render):
  """Case 10: render_scenes == the hand-assembled render_batch call (through `render`), default camera and errors."""
  import dataclasses
  import pytest
  from corenet_amd.geometry import transformations as T
  scenes = make_scenes()
  size, tsize = (40, 56), (8, 16)
  for shading_normals in (True, False):
    got = R.render_scenes(scenes, image_size=size, texture_size=tsize, device=device, shading_normals=shading_normals,
                          clear_colors=(0.1, 0.2, 0.3))
    assert got.device.type == device and tuple(got.shape) == (2, 40, 56, 3) and got.dtype == t.uint8
    tris, nrms, uvs, mids, cols, pngs, ranges, vps = [], [], [], [], [], [], [], []
    for sc in scenes:
      t0 = sum(x.shape[0] for x in tris)
      for k in range(2):
        tris.append(T.transform_mesh(sc.mesh_vertices[k], sc.o2w_transforms[k]))
        nrms.append(sc.normals[k] @ t.inverse(sc.o2w_transforms[k][:3, :3]))       # n^T M^-1 = (M^-T n)^T
        uvs.append(sc.texcoords[k])
        mids.append(sc.material_ids[k] + 2 * (len(tris) - 1))
        cols.append(sc.diffuse_colors[k])
        pngs += sc.diffuse_texture_pngs[k]
      ranges.append([t0, t0 + 24])
      vps.append(sc.camera_transform @ sc.view_transform)
    textures, ids = R.load_textures(pngs, tsize)
    assert tuple(textures.shape) == (3, 8, 16, 3) and (ids >= 0).sum() == 4
    exp = render(t.cat(tris), t.cat(mids), R.make_materials(t.cat(cols)), ranges, t.stack(vps), size,
                 normals=t.cat(nrms) if shading_normals else None, tex_coords=t.cat(uvs), textures=textures,
                 texture_indices=ids, clear_colors=(0.1, 0.2, 0.3))
    assert t.equal(got.cpu(), exp)
    covered = (exp != t.tensor([26, 51, 76], dtype=t.uint8)).any(-1)
    assert covered[0].float().mean() > 0.05 and covered[1].float().mean() > 0.05 and not t.equal(exp[0], exp[1])
    plain = render(t.cat(tris), t.cat(mids), R.make_materials(t.cat(cols)), ranges, t.stack(vps), size,
                   normals=t.cat(nrms) if shading_normals else None, clear_colors=(0.1, 0.2, 0.3))
    assert not t.equal(plain, exp)                                  # the textures are in the picture
  # an explicit camera replaces the default
  other = R.render_scenes(scenes, view_projections=t.stack(vps).flip(0), image_size=size, texture_size=tsize,
                          device=device, shading_normals=False, clear_colors=(0.1, 0.2, 0.3))
  assert not t.equal(other.cpu(), exp)
  bare = dataclasses.replace(scenes[1], normals=[], texcoords=[], material_ids=[], diffuse_colors=[],
                             diffuse_texture_pngs=[])
  with pytest.raises(ValueError, match="load_extra_fields"):
    R.render_scenes([scenes[0], bare], image_size=size, device=device)
