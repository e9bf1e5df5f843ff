"""Textured rendering through the library's host twin (no GPU): the texture rule against a float64 reference, row
orientation, layers, the bit-exact identities, non-finite coordinates, batching, validation, load_textures and
render_scenes.  The cases are in render_tex_check.py; test_render_tex_gpu.py runs them on the HIP kernel."""
import os

import pytest

import render_tex_check as X


@pytest.fixture(scope="module")
def R():
  from corenet_amd import build as B
  if not os.path.exists(B.LIB):
    B.build(verbose=False)
  from corenet_amd.visualization import render as R
  return R


@pytest.fixture(scope="module")
def render(R):
  return R.render_batch


@pytest.mark.parametrize("kind", ["random", "checker"])
@pytest.mark.parametrize("uv_range", list(X.UV_RANGES))
@pytest.mark.parametrize("tex_size", X.TEX_SIZES, ids=lambda s: "%dx%d" % s)
def test_orthographic_against_float64(render, tex_size, uv_range, kind):
  X.case_orthographic(render, tex_size, uv_range, kind)


def test_perspective_against_float64(render):
  X.case_perspective(render)


def test_row_orientation(render):
  X.case_row_orientation(render)


def test_layers_and_materials(render):
  X.case_layers_and_materials(render)


@pytest.mark.parametrize("normals", [True, False], ids=["normals", "geometric"])
def test_bit_exact_identities(render, normals):
  X.case_identities(render, normals)


def test_non_finite_and_huge_coordinates(render):
  X.case_non_finite(render)


def test_batching(render):
  X.case_batching(render)


def test_validation(render):
  X.case_validation(render)


def test_c_abi_rejects_bad_texture_sizes(R):
  """crn_render_cpu_tex: L, Ht or Wt < 1 with a texture pointer is CRN_EINVAL; NULL textures or ids mean none."""
  import numpy as np
  import torch as t
  from corenet_amd import _lib as L
  args, _ = X.lit_cube(False)
  tri, mids, mats, _, vps, (H, W) = args
  plain = X.render_cpu_abi(args, None)
  rec = np.zeros((1, 40), np.float32)
  rec[0, :16] = vps[0].reshape(16).numpy()
  rec[0, 16:19] = rec[0, 19:22] = R.camera_position(vps[0]).numpy()
  rec[0, 22:25], rec[0, 25:28] = 1.0, 0.2
  rec.view(np.int32)[0, 34] = 12
  tex, ids = t.zeros((1, 2, 2, 4), dtype=t.uint8), t.zeros(3, dtype=t.int32)
  out = t.empty((1, H, W, 3), dtype=t.uint8)
  fn = L.lib().cdll.crn_render_cpu_tex                               # the raw symbol: the status is the subject
  fn.argtypes, fn.restype = L._SIGS["crn_render_cpu_tex"], L.C.c_int

  def call(texels, tids, dims):
    return fn(tri.data_ptr(), None, mids.data_ptr(), mats.data_ptr(), 3, rec.ctypes.data, 1, H, W, out.data_ptr(), None,
              tids, texels, *dims, 1)
  for dims in ((0, 2, 2), (1, 0, 2), (1, 2, 0), (-1, 2, 2)):
    assert call(tex.data_ptr(), ids.data_ptr(), dims) != 0, dims
  for texels, tids in ((None, ids.data_ptr()), (tex.data_ptr(), None), (None, None)):
    assert call(texels, tids, (0, 0, 0) if texels is None else (1, 2, 2)) == 0
    assert t.equal(out, plain)
  assert call(tex.data_ptr(), ids.data_ptr(), (1, 2, 2)) == 0 and not t.equal(out, plain)      # black texels


def test_load_textures(R):
  X.case_load_textures(R)


def test_render_scenes(R, render):
  X.case_render_scenes(R, "cpu", render)


def test_render_scene_textures(R):
  """render_scene with the reference's texture arguments: indices cut to the used materials, textures to the used
  layers, mismatches are ValueErrors."""
  import numpy as np
  import torch as t
  tri, uv = X.quad(X.rect(-2, 2, -2, 2), X.rect_uv(-0.5, 1.5, -0.5, 1.5))
  texs = t.from_numpy(np.stack([X.random_texture(4, 4, 1), X.checker_texture(4, 4)]))
  kw = dict(material_ids=t.tensor([1, 1], dtype=t.int32), diffuse_coefficients=t.tensor([[0.5] * 3, [1.0, 0.9, 0.8], [0.1] * 3]),
            ambient_coefficients=t.zeros(3, 3), cull_back_facing=False, light_color=(0.0, 0.0, 0.0),
            ambient_light_color=(1.0, 1.0, 1.0))
  img = R.render_scene(tri, t.eye(4), (16, 24), tex_coords=uv, diffuse_textures=t.cat([texs, texs]),
                       diffuse_texture_indices=t.tensor([-1, 1, 7]), **kw)         # material 2 and layers 2, 3 are unused
  exp = X.ref_quad_image(X.IDENTITY, X.rect(-2, 2, -2, 2), X.rect_uv(-0.5, 1.5, -0.5, 1.5), (1.0, 0.9, 0.8),
                         texs[1].numpy(), 16, 24)
  X.assert_close(img, exp, "render_scene")
  plain = R.render_scene(tri, t.eye(4), (16, 24), **kw)
  assert t.equal(R.render_scene(tri, t.eye(4), (16, 24), tex_coords=uv, **kw), plain)
  assert t.equal(R.render_scene(tri, t.eye(4), (16, 24), tex_coords=uv, diffuse_textures=texs, **kw), plain)
  assert not t.equal(img, plain)
  for bad in (dict(diffuse_textures=texs[:1], diffuse_texture_indices=t.tensor([-1, 1])),
              dict(diffuse_textures=texs, diffuse_texture_indices=t.tensor([0])),
              dict(diffuse_texture_indices=t.tensor([-1, 1])),
              dict(diffuse_textures=texs[..., :2], diffuse_texture_indices=t.tensor([-1, 1]))):
    with pytest.raises(ValueError):
      R.render_scene(tri, t.eye(4), (16, 24), tex_coords=uv, **bad, **kw)
