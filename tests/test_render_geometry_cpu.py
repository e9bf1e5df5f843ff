"""render.render_geometry through the library's host twin (crn_render_cpu_geometry): the winner against render_batch's
colour image, the golden silhouettes, a float64 restatement, known depths, output handling and the two gather helpers.
The checks and scenes are render_geometry_check.py; test_render_geometry_gpu.py runs them on the kernel."""
import math

import numpy as np
import pytest
import torch as t

import render_geometry_check as K
import render_scenes as S


@pytest.fixture(scope="module")
def R():
  from corenet_amd.visualization import render as R
  return R


@pytest.fixture(scope="module")
def rendered(R):
  """name -> (case, GeometryBuffers of the twin, float64 restatement), computed once."""
  return {name: (case, K.render_case(R, case), K.restate_case(case)) for name, case in K.cases().items()}


def test_triangle_index_equals_id_colour_image(R, rendered):
  for name, (case, buf, _) in rendered.items():
    ids = K.id_colour_image(R, case)
    idx = buf.triangle_index.numpy()
    assert np.array_equal(ids, idx), (name, int((ids != idx).sum()))
  case, buf, _ = rendered["soup"]
  idx = buf.triangle_index.numpy()
  T_ = case["triangles"].shape[0]
  assert (idx[0] == T_ - 3).sum() > 15 and not (idx == T_ - 4).any()        # coincident pair: the later one wins
  assert (idx[0] == T_ - 2).any()                                           # one vertex behind the eye: still drawn
  assert not (idx == T_ - 1).any()                                          # wholly beyond z_ndc = 1
  assert (idx[2] == -1).all()                                               # the empty range
  assert idx[1][idx[1] >= 0].min() >= 5 and idx[1].max() < T_ - 1           # indices into the shared buffer, not the range
  on, off = idx[3], idx[0]                                                  # same image with and without culling
  assert (on != off).any() and not (on[off < 0] >= 0).any() and (on >= 0).sum() < (off >= 0).sum()


def test_mask_covers_the_golden_silhouettes(R):
  from corenet_amd.geometry import transformations as T
  cam = t.matmul(T.perspective_rh(70 * math.pi / 180, 1, 0.1, 10.0), T.look_at_rh((-1.2, -1.5, -1), (0, 0, 0), (0, 1, 0)))
  mesh = R.render_geometry(S.cube_mesh(), [[0, 12]], cam[None], (256, 256), True, outputs=("triangle_index",))
  assert int(mesh.mask.sum()) == 6377
  assert np.array_equal(mesh.mask[0].numpy(), S.mesh_scene().numpy().any(-1))
  la = T.look_at_rh((-1.2 + 0.5, -1.5 + 0.5, -0.5 + 0.5), (0.5, 0.5, 0.5), (0, 1, 0))
  mv = t.matmul(T.perspective_rh(70 * math.pi / 180, 1, 0.1, 10.0), la)
  f = R.voxel_faces(t.tensor(S.VOXEL_GRID, dtype=t.int32)[None], ((-1, 0, 0), (1.0, 0, 0)), T.scale((1.0 / 3,) * 3))
  vox = R.render_geometry(f.triangles, [[0, f.triangles.shape[0]]], mv[None], (256, 256), outputs=("triangle_index",))
  assert int(vox.mask.sum()) == 10395


def test_against_float64_restatement(rendered):
  """The twin's largest deviations over these cases, measured here on the host: barycentrics 3.41e-5, depth 3.94e-6,
  z_ndc 7.85e-6; K.TOL is 8 times that (render_geometry_check.py)."""
  worst = {}
  for name, (case, buf, ref) in rendered.items():
    frac = K.undecided_fraction(ref)
    assert (frac <= K.MAX_UNDECIDED).all(), (name, frac)
    assert ref["covered"].sum() > 100
    for k, v in K.deviations(buf, ref).items():
      worst[k] = max(worst.get(k, 0.0), v)
  print("largest deviations from the restatement:", worst)
  for k, v in worst.items():
    assert v <= K.TOL[k], (k, v)
  case, buf, ref = rendered["receding"]
  assert ref["depth"][ref["covered"]].max() / ref["depth"][ref["covered"]].min() > 4   # perspective matters here


def test_known_depths(R, rendered):
  from corenet_amd.visualization import camera_util as C
  import render_tex_check as X
  d = 2.75
  rect, _ = X.quad(X.rect(-0.9, 1.1, -0.7, 0.8, z=d), X.rect_uv(0, 1, 0, 1))
  buf = R.render_geometry(rect, [[0, 2]], C.perspective_projection(1.0, znear=0.1, zfar=10)[None], (29, 37))
  assert int(buf.mask.sum()) > 100 and not bool(buf.mask.all())
  assert float((buf.depth[buf.mask] - d).abs().max()) <= K.TOL["depth"]
  assert bool(t.isinf(buf.depth[~buf.mask]).all())
  # the receding quad: the eye ray through the pixel centre meets the plane z = 1.6 + 1.2 x; w = z of the hit
  case, buf, ref = rendered["receding"]
  H, W = case["size"]
  vp = case["vps"][0].numpy().astype(np.float64)
  x_ndc = (np.arange(W) + 0.5) / W * 2 - 1
  y_ndc = (np.arange(H) + 0.5) / H * 2 - 1
  X_, Y_ = np.meshgrid(x_ndc, y_ndc)
  dx = X_ / vp[0, 0]                                                 # the ray (dx, dy, 1) z: clip x = vp00 x, w = z
  z_hit = 1.6 / (1 - 1.2 * dx)
  ok = ref["decided"][0] & ref["covered"][0]
  assert ok.sum() > 0.9 * H * W
  got = buf.depth[0].numpy().astype(np.float64)
  assert np.abs(got[ok] - z_hit[ok]).max() <= K.TOL["depth"]
  assert z_hit[ok].max() / z_hit[ok].min() > 4


def test_outputs_background_and_errors(R, rendered):
  case, full, _ = rendered["soup"]
  bg = ~full.mask
  assert bool(bg.any()) and bool(full.mask.any())
  assert bool((full.triangle_index[bg] == -1).all()) and bool((full.barycentrics[bg] == 0).all())
  assert bool((full.depth[bg] == math.inf).all()) and bool((full.z_ndc[bg] == math.inf).all())
  assert bool(t.isfinite(full.depth[~bg]).all()) and bool((full.z_ndc[~bg].abs() <= 1).all())
  assert float((full.barycentrics[~bg].sum(-1) - 1).abs().max()) < 1e-6
  assert full.triangle_index.dtype == t.int32 and full.barycentrics.shape == (4, 29, 37, 3)
  for name in R.GEOMETRY_OUTPUTS:
    one = K.render_case(R, case, outputs=(name,))
    for other in R.GEOMETRY_OUTPUTS:
      x = getattr(one, other)
      assert (x is None) == (other != name)
    assert t.equal(getattr(one, name).view(t.int32), getattr(full, name).view(t.int32)), name
  with pytest.raises(ValueError, match="mask needs"):
    K.render_case(R, case, outputs=("depth",)).mask
  tri, rg, vps = case["triangles"], case["ranges"], case["vps"]
  for bad in (dict(outputs=()), dict(outputs=("depth", "normals")), dict(triangles=tri[:, :2]),
              dict(ranges=[[0, 2], [3, 1], [0, 0], [0, 0]]), dict(ranges=[[0, tri.shape[0] + 1]] * 4),
              dict(ranges=[[-1, 2]] * 4), dict(size=(0, 5)), dict(size=(5, -1)), dict(ranges=t.zeros(0, 2))):
    kw = dict(triangles=tri, ranges=rg, vps=vps, size=(8, 8), outputs=R.GEOMETRY_OUTPUTS)
    kw.update(bad)
    with pytest.raises(ValueError):
      R.render_geometry(kw["triangles"], kw["ranges"], kw["vps"], kw["size"], outputs=kw["outputs"])
  # the C ABI refuses a call without any output
  from corenet_amd import _lib as L
  images = t.zeros(1, 40)
  with pytest.raises(L.HipError):
    L.lib().crn_render_cpu_geometry(tri.data_ptr(), images.data_ptr(), 1, 8, 8, None, None, None, None, 1)


def test_gather_and_interpolate_helpers(R, rendered):
  case, buf, _ = rendered["soup"]
  tri = case["triangles"]
  T_ = tri.shape[0]
  idx = buf.triangle_index.numpy()
  per_tri = t.arange(T_, dtype=t.int64) * 3 + 7
  got = R.gather_triangle_attribute(buf, per_tri, -5).numpy()
  vec = t.from_numpy(np.random.RandomState(0).rand(T_, 2, 2).astype(np.float32))
  got_vec = R.gather_triangle_attribute(buf, vec, 0.25).numpy()
  pos = R.interpolate_vertex_attribute(buf, tri, float("nan")).numpy()
  assert got.shape == idx.shape and got_vec.shape == idx.shape + (2, 2) and pos.shape == idx.shape + (3,)
  b = buf.barycentrics.numpy()
  for i, r, c in np.ndindex(*idx.shape):
    k = idx[i, r, c]
    if k < 0:
      assert got[i, r, c] == -5 and (got_vec[i, r, c] == 0.25).all() and np.isnan(pos[i, r, c]).all()
    else:
      assert got[i, r, c] == 3 * k + 7 and np.array_equal(got_vec[i, r, c], vec[k].numpy())
      v = tri[k].numpy()
      assert np.array_equal(pos[i, r, c], (b[i, r, c, 0] * v[0] + b[i, r, c, 1] * v[1]) + b[i, r, c, 2] * v[2])
  # the interpolated view-space position projects to the pixel it was found at, and its clip w is the depth output
  vp = case["vps"][0].numpy().astype(np.float64)
  m = idx[0] >= 0
  clip = np.concatenate([pos[0][m].astype(np.float64), np.ones((m.sum(), 1))], -1) @ vp.T
  rows, cols = np.nonzero(m)
  assert np.abs((clip[:, 0] / clip[:, 3] + 1) / 2 * 37 - (cols + 0.5)).max() < 1e-3
  assert np.abs((clip[:, 1] / clip[:, 3] + 1) / 2 * 29 - (rows + 0.5)).max() < 1e-3
  assert np.abs(clip[:, 3] - buf.depth[0].numpy()[m]).max() < 1e-4
  with pytest.raises(ValueError):
    R.interpolate_vertex_attribute(buf, tri[:, :2], 0.0)
  with pytest.raises(ValueError):
    R.gather_triangle_attribute(K.render_case(R, case, outputs=("depth",)), per_tri, 0)
