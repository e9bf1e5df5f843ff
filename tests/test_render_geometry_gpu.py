"""render.render_geometry on the MI355X: the kernel of csrc/render.hip against the library's host twin, bit for bit on all
four outputs, determinism, long staged tile lists, and voxel faces against a brute-force ray caster.  Scenes and checks:
render_geometry_check.py."""
import numpy as np
import pytest
import torch as t

import render_geometry_check as K

pytestmark = pytest.mark.gpu
_gpu = K.gpu_step


@pytest.fixture(scope="module")
def R():
  from corenet_amd.visualization import render as R
  return R


def _same_bits(a, b, what):
  for name in a._fields:
    x, y = getattr(a, name), getattr(b, name)
    assert (x is None) == (y is None), (what, name)
    if x is not None:
      assert x.shape == y.shape and x.dtype == y.dtype, (what, name)
      assert t.equal(x.cpu().view(t.int32), y.cpu().view(t.int32)), (what, name)


def _both(R, case, **kw):
  g = _gpu(lambda: K.render_case(R, case, "cuda", **kw), 30)
  assert all(x is None or x.device.type == "cuda" for x in g)
  _same_bits(g, K.render_case(R, case, **kw), "twin")
  return g


def test_cases_equal_twin_colour_image_and_restatement(R):
  for name, case in K.cases().items():
    g = _both(R, case)
    _same_bits(g, _gpu(lambda: K.render_case(R, case, "cuda"), 30), "second run")
    ids = _gpu(lambda: K.id_colour_image(R, case, "cuda"), 30)
    assert np.array_equal(ids, g.triangle_index.cpu().numpy()), name
    ref = K.restate_case(case)
    assert (K.undecided_fraction(ref) <= K.MAX_UNDECIDED).all()
    for k, v in K.deviations(g, ref).items():
      assert v <= K.TOL[k], (name, k, v)


def test_outputs_and_background_on_gpu(R):
  case = K.soup_case()
  full = _both(R, case)
  bg = ~full.mask
  assert bool((full.triangle_index[bg] == -1).all()) and bool((full.barycentrics[bg] == 0).all())
  assert bool(t.isposinf(full.depth[bg]).all()) and bool(t.isposinf(full.z_ndc[bg]).all())
  for name in R.GEOMETRY_OUTPUTS:
    one = _both(R, case, outputs=(name,))
    assert [x is not None for x in one] == [o == name for o in R.GEOMETRY_OUTPUTS]
    assert t.equal(getattr(one, name).view(t.int32), getattr(full, name).view(t.int32)), name
  with pytest.raises(ValueError):
    R.render_geometry(case["triangles"].cuda(), case["ranges"], case["vps"], case["size"], outputs=())
  with pytest.raises(ValueError):
    R.render_geometry(case["triangles"].cuda(), case["ranges"], case["vps"], case["size"], outputs=("colour",))
  empty = _gpu(lambda: R.render_geometry(t.zeros(0, 3, 3).cuda(), [[0, 0]], case["vps"][:1], (5, 7)), 30)
  assert bool((empty.triangle_index == -1).all()) and bool(t.isposinf(empty.depth).all())


def test_long_tile_lists_equal_twin(R):
  """3000 triangles over a few of the 15 tiles: lists of several 64-record chunks with a partial last one, and empty
  tiles."""
  case = K.long_list_soup()
  g = _both(R, case)
  _same_bits(g, _gpu(lambda: K.render_case(R, case, "cuda"), 30), "second run")
  idx = g.triangle_index.cpu().numpy()
  tiles = (idx >= 0).reshape(2, 3, 16, 5, 16).any((2, 4))
  assert tiles.any() and not tiles.all()                                        # covered and empty tiles
  assert (idx[0] >= 0).sum() > 200 and len(np.unique(idx[0])) > 65              # more winners than one chunk holds
  assert idx[1][idx[1] >= 0].min() >= 100 and idx[1].max() < 1125


def test_voxel_faces_against_ray_caster(R):
  g = _gpu(lambda: K.check_label_grid(R, "cuda"), 30)
  _same_bits(g, K.check_label_grid(R, "cpu"), "twin")
