"""corenet_amd.visualization rendering through the library's host twin (no GPU): the reference's two GL golden images,
the camera and transform helpers, voxel-face extraction, the coverage / depth rules and the qualitative-results path."""
import math
import os

import numpy as np
import PIL.Image
import pytest
import torch as t

import render_scenes as S


@pytest.fixture(scope="module")
def R():
  from corenet_amd import build as B
  if not os.path.exists(B.LIB):
    B.build(verbose=False)
  from corenet_amd.visualization import render as R
  return R


def _ortho_scene(R, tris, colors, size=(32, 32), **kw):
  """Flat-shaded triangles seen through the identity view-projection (world = NDC), one material per triangle."""
  tris = t.as_tensor(tris, dtype=t.float32).reshape(-1, 3, 3)
  mats = R.make_materials(t.as_tensor(colors, dtype=t.float32), 0.0, (0.0, 0.0, 0.0), 1.0)
  mats[:, 3:6] = 0.0
  mats[:, 0:3] = t.as_tensor(colors, dtype=t.float32)          # ambient only: colour = material colour
  return R.render_batch(tris, t.arange(len(tris), dtype=t.int32), mats, [[0, len(tris)]], t.eye(4)[None], size, **kw)[0]


def test_golden_mesh_image(R):
  img = S.mesh_scene().numpy()
  assert img.dtype == np.uint8 and img.shape == (256, 256, 3)
  l1, ndiff, cov, cov_ref = S.golden_stats(img, "mesh")
  assert l1 <= 1024 and cov == cov_ref, (l1, ndiff, cov, cov_ref)
  assert np.abs(img.astype(int) - S.golden("mesh")).max() <= 1
  flipped = np.abs(img[::-1].astype(int) - S.golden("mesh")).sum()
  assert flipped > 100 * 1024                                       # the row order matters


def test_golden_voxel_image(R):
  img = S.voxel_scene().numpy()
  l1, ndiff, cov, cov_ref = S.golden_stats(img, "voxels")
  assert l1 <= 1024 and cov == cov_ref, (l1, ndiff, cov, cov_ref)
  assert np.abs(img.astype(int) - S.golden("voxels")).max() <= 1


def test_camera_util_matrices():
  from corenet_amd.visualization import camera_util as C
  np.testing.assert_allclose(C.cameras_on_tetrahedron_vertices()[1].numpy(),
                             [[-0.86603, 0., -0.5, -0.], [0.16667, 0.94281, -0.28868, 0.], [0.4714, -0.33333, -0.8165, 1.],
                              [0., 0., 0., 1.]], atol=1e-4)
  np.testing.assert_allclose(C.cameras_on_tetrahedron_vertices()[3].numpy(),
                             [[0., 0., 1., 0.], [1., 0., 0., 0.], [0., 1., 0., 1.], [0., 0., 0., 1.]], atol=1e-6)
  np.testing.assert_allclose(C.frontal_camera(1.5).numpy(), [[-1, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 1.5], [0, 0, 0, 1]])
  f = 1 / math.tan(math.pi / 6)                                      # fovy 60 degrees
  np.testing.assert_allclose(C.perspective_projection().numpy(),
                             [[f, 0, 0, 0], [0, -f, 0, 0], [0, 0, 10.0001 / 9.9999, -2 * 10 * 1e-4 / 9.9999], [0, 0, 1, 0]],
                             rtol=1e-5, atol=1e-6)
  np.testing.assert_allclose(C.get_ortho_matrix().numpy(), [[2, 0, 0, 0], [0, -2, 0, 0], [0, 0, 2, 0], [0, 0, 0, 1]])
  mesh = (((12, 34, 56), (34, 32, 30), (11, 11, 18)), ((1, 2, 3), (4, 5, 6), (6, 5, 4)))
  np.testing.assert_allclose(C.get_default_camera_for_mesh(mesh).numpy(),
                             [[-1.4999999, 0., -0.86602527, 51.79774], [-0.2886751, -1.632993, 0.49999994, 19.695688],
                              [0.47177827, -0.33359763, -0.817144, 59.858547], [0.47140452, -0.33333334, -0.8164966, 59.937073]],
                             rtol=1e-5, atol=1e-5)


def test_transformations():
  from corenet_amd.geometry import transformations as T
  # left-handed look-at: the eye maps to the origin, the target onto +z
  m = T.look_at_lh((1.0, 2.0, 3.0), (1.0, 2.0, 7.0), (0, 1, 0))
  np.testing.assert_allclose(m.numpy(), [[1, 0, 0, -1], [0, 1, 0, -2], [0, 0, 1, -3], [0, 0, 0, 1]], atol=1e-6)
  p = T.perspective_lh(math.pi / 2, 2.0, 1.0, 3.0)
  np.testing.assert_allclose(p.numpy(), [[0.5, 0, 0, 0], [0, 1, 0, 0], [0, 0, 2, -3], [0, 0, 1, 0]], atol=1e-6)
  np.testing.assert_allclose(T.ortho_lh(0, 2, 0, 4, 1, 3).numpy(),
                             [[1, 0, 0, -1], [0, 0.5, 0, -1], [0, 0, 1, -2], [0, 0, 0, 1]], atol=1e-6)
  a, b = T.translate([1.0, 2.0, 3.0]), T.scale([2.0, 2.0, 2.0])
  assert t.equal(T.chain([a, b]), a @ b)
  pts = t.tensor([[1.0, 1.0, 1.0], [0.0, -1.0, 2.0]])
  np.testing.assert_allclose(T.transform_points(pts, T.chain([a, b])).numpy(), [[3, 4, 5], [1, 0, 7]])
  proj = t.tensor([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 1, 0]])
  np.testing.assert_allclose(T.transform_points(t.tensor([[2.0, 4.0, 2.0]]), proj).numpy(), [[1, 2, 1]])
  tri = t.tensor([[[1.0, 0, 0], [0, 1, 0], [0, 0, 1]]])
  np.testing.assert_allclose(T.transform_mesh(tri, a).numpy(), (tri + t.tensor([1.0, 2, 3])).numpy())
  np.testing.assert_allclose(T.transform_mesh(tri, a, False).numpy(), tri.numpy())


def test_voxel_face_counts_and_order(R):
  pal = t.tensor([[-1.0, -1, -1], [1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]])
  one = t.zeros(1, 3, 3, 3, dtype=t.int32)
  one[0, 1, 1, 1] = 2
  f = R.voxel_faces(one, pal, t.eye(4))
  assert f.num_triangles.tolist() == [12] and f.material_ids.tolist() == [2] * 12
  full = t.ones(1, 3, 4, 5, dtype=t.int32)
  assert R.voxel_faces(full, pal, t.eye(4)).num_triangles.tolist() == [2 * 2 * (3 * 4 + 4 * 5 + 3 * 5)]
  # exposed faces == drawn voxels' neighbours that are void or outside, counted with torch
  g = t.from_numpy(np.random.RandomState(3).randint(0, 5, (3, 7, 6, 5)).astype(np.int32))
  drawn = ((g >= 1) & (g <= 3)).to(t.int32)                        # label 4 is outside the palette
  pd = t.nn.functional.pad(drawn, (1, 1, 1, 1, 1, 1))
  exp = 0
  for ax in (1, 2, 3):
    for s in (1, -1):
      exp = exp + (drawn * (1 - t.roll(pd, s, ax)[:, 1:-1, 1:-1, 1:-1])).sum((1, 2, 3))
  f = R.voxel_faces(g, pal, t.eye(4), material_base=10)
  assert f.num_triangles.tolist() == (2 * exp).tolist()
  assert set(f.material_ids.tolist()) <= {11, 12, 13}
  # two voxels side by side along x: voxel (0,0,0) has +x hidden -> its faces -x +y -y +z -z, then voxel (1,0,0)
  two = t.tensor([[[[1, 1]]]], dtype=t.int32)
  f = R.voxel_faces(two, pal, t.eye(4))
  assert f.num_triangles.tolist() == [20]
  n = f.normals[0::2, 0]
  assert t.equal(f.normals[:, 0], f.normals[:, 1]) and t.equal(f.normals[:, 0], f.normals[:, 2])
  axes = [(n[k].abs().argmax().item(), int(t.sign(n[k][n[k].abs().argmax()]).item())) for k in range(10)]
  # flat normal = normalize(cross(dx, dy)) of the shader's (center, dy, dx) quads
  ref = {0: (0, -1), 1: (0, 1), 2: (1, -1), 3: (1, 1), 4: (2, -1), 5: (2, 1)}
  assert axes == [ref[f_] for f_ in (1, 2, 3, 4, 5)] + [ref[f_] for f_ in (0, 2, 3, 4, 5)]
  c = f.triangles.reshape(-1, 9, 1).reshape(-1, 3, 3).mean(1)[0::2]
  assert (c[:5, 0] < 1.01).all() and (c[5:, 0] > 0.99).all()
  # the quad (v0, v1, v2), (v2, v1, v3) of the +x face of voxel 1: x = 2, spanning y, z in [0, 1]
  q = f.triangles[10:12]
  assert t.equal(q[0, 2], q[1, 0]) and t.equal(q[0, 1], q[1, 1]) and (q[:, :, 0] == 2).all()


def test_voxel_box_of_occupied_centres(R):
  g = t.zeros(1, 4, 5, 6, dtype=t.int32)
  g[0, 1, 2, 3] = 1
  g[0, 3, 0, 5] = 2
  pal = t.tensor([[-1.0, -1, -1], [1.0, 0, 0]])                     # label 2 is not drawn, but occupies the box
  f = R.voxel_faces(g, pal, t.eye(4), box_matrices=t.diag(t.tensor([2.0, 2.0, 2.0, 1.0])))
  np.testing.assert_allclose(f.boxes[0].numpy(), [[7, 1, 3], [11, 5, 7]])
  assert f.num_triangles.tolist() == [12]
  f = R.voxel_faces(t.zeros(1, 2, 2, 2, dtype=t.int32), pal, t.eye(4), box_matrices=t.eye(4))
  assert f.boxes.abs().sum() == 0 and f.triangles.shape == (0, 3, 3)


def test_equal_depth_later_triangle_wins(R):
  tri = [[-1, -1, 0], [3, -1, 0], [-1, 3, 0]]
  img = _ortho_scene(R, [tri, tri], [[1.0, 0, 0], [0, 1.0, 0]])
  assert (img[..., 1] == 255).all() and (img[..., 0] == 0).all()
  nearer = [[-1, -1, -0.5], [3, -1, -0.5], [-1, 3, -0.5]]
  img = _ortho_scene(R, [nearer, tri], [[1.0, 0, 0], [0, 1.0, 0]])
  assert (img[..., 0] == 255).all()


def test_near_plane_and_behind_the_eye(R):
  from corenet_amd.geometry import transformations as T
  proj = T.perspective_rh(math.pi / 2, 1.0, 1.0, 10.0)
  mats = R.make_materials(t.tensor([[1.0, 1.0, 1.0]]), 1.0, (0.0, 0.0, 0.0), 1.0)
  def draw(tri, cull=False):
    return R.render_batch(t.tensor([tri], dtype=t.float32), t.zeros(1, dtype=t.int32), mats, [[0, 1]], proj[None],
                          (32, 32), cull_back_facing=cull)[0].any(-1)
  # a floor crossing the near plane (z_view = -1) and going behind the eye: only the part at z_view <= -1 shows
  cov = draw([[-4.0, -1.0, 2.0], [4.0, -1.0, 2.0], [0.0, -1.0, -8.0]])
  assert cov.any() and not cov[16:].any()                          # below the horizon only, no wrap-around to the top
  # fully behind the eye: nothing
  assert not draw([[-1.0, -1.0, 3.0], [1.0, -1.0, 3.0], [0.0, 1.0, 3.0]]).any()
  # one vertex behind the eye (w < 0): the coverage equals that of the visible part cut by hand at the near plane
  a, b, c = np.array([-2.0, -0.5, -4.0]), np.array([2.0, -0.5, -4.0]), np.array([0.0, -0.5, 2.0])
  ta = (-1.0 - a[2]) / (c[2] - a[2])
  pa, pb = a + (c - a) * ta, b + (c - b) * ta
  full = draw([a.tolist(), b.tolist(), c.tolist()])
  part = draw([a.tolist(), b.tolist(), pb.tolist()]) | draw([a.tolist(), pb.tolist(), pa.tolist()])
  assert (full ^ part).sum() <= 2 * 32                              # only along the cut (z_ndc = -1 rounding)
  assert full.sum() > 0


def test_fullscreen_quad_of_many_triangles_has_no_holes(R):
  rng = np.random.RandomState(0)
  xs = np.concatenate([[-1.0], np.sort(rng.uniform(-1, 1, 9)), [1.0]])
  ys = np.concatenate([[-1.0], np.sort(rng.uniform(-1, 1, 7)), [1.0]])
  tris = []
  for i in range(len(xs) - 1):
    for j in range(len(ys) - 1):
      p00, p10 = [xs[i], ys[j], 0.0], [xs[i + 1], ys[j], 0.0]
      p01, p11 = [xs[i], ys[j + 1], 0.0], [xs[i + 1], ys[j + 1], 0.0]
      tris += [[p00, p10, p11], [p00, p11, p01]]
  # a fan around an interior point too
  c = [0.1, -0.2, 0.0]
  ring = [[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]]
  fan = [[ring[k], ring[(k + 1) % 4], c] for k in range(4)]
  for tt in (tris, fan):
    n = len(tt)
    colors = np.full((n, 3), 1.0)
    img = _ortho_scene(R, tt, colors, size=(61, 67))
    assert (img == 255).all()
    # and no pixel is drawn twice: with additive-looking colours every pixel has exactly one winner, which the
    # ids of a second render show; count per-triangle coverage
    cov = 0
    for k in range(n):
      one = _ortho_scene(R, [tt[k]], [[1.0, 1.0, 1.0]], size=(61, 67))
      cov = cov + (one[..., 0] == 255).to(t.int32)
    assert (cov == 1).all()


def test_scene_defaults_and_culling(R):
  from corenet_amd.visualization import camera_util as C
  mesh = S.cube_mesh()
  a = R.render_scene(mesh)                                           # default camera, white-ish 0.8 diffuse
  assert a.shape == (256, 256, 3) and a.any()
  cam = C.get_default_camera_for_mesh(mesh)
  assert t.equal(a, R.render_scene(mesh, cam))
  # the cube is wound clockwise from outside in the GL sense of this camera: culling keeps the inside faces only
  b = R.render_scene(mesh, cam, cull_back_facing=False)
  assert b.any()
  four = R.render_scene(mesh, cam, return_rgb=False)
  assert four.shape == (256, 256, 4) and (four[..., 3] == 255).all()


def test_visualize_output_and_qualitative_results(tmp_path, R):
  from corenet_amd import evaluation_results as ER
  from corenet_amd.visualization import artifacts as A
  pmf, ex = S.synthetic_example(B=2, R=24)
  rows = ER.visualize_output(pmf, ex, "fg_bg")
  assert len(rows) == 2 and all(len(r) == 5 for r in rows)
  for r in rows:
    for img in r:
      assert img.dtype == t.uint8 and img.shape == (384, 1920, 3)
  # the input image panel: 64 x 48 scaled by 6 to 384 x 288, padded by 48 columns on both sides
  assert (rows[0][0][:, :48] == 0).all() and (rows[0][0][:, 336:384] == 0).all() and rows[0][0][:, 48:336].any()
  # every 3D panel shows something from every camera
  for c in range(5):
    for p in range(1, 5):
      assert rows[0][c][:, 384 * p:384 * (p + 1)].any(), (c, p)
  # one batched render == the artifact-by-artifact path
  b = 1
  v2x = ex.v2x_transform[b].inverse()
  label = int(ex.mesh_labels[b][0])
  pal = t.as_tensor(A.colors.DEFAULT_COLOR_PALETTE)
  pred, gt = ER.extract_labels(pmf, ex, "fg_bg")
  arts = [A.MarchingCubesArtifact(pmf[b], v2x, pal[[0, label]]),
          A.MultiMeshArtifact(ex.vertices[12 * b:12 * (b + 1)], ex.mesh_num_tri[b], mesh_colors=pal[[label]]),
          A.VoxelGridArtifact(pred[b], v2x), A.VoxelGridArtifact(gt[b], v2x)]
  ref = A.visualize_artifacts([A.ImageArtifact(ex.input_image[b]), arts], ex.camera_transform[b], ex.view_transform[b])
  one = ER.visualize_output(pmf, ex, "fg_bg", [b])[0]
  for c in range(5):
    assert t.equal(one[c], ref[c]), c
    assert t.equal(one[c], rows[b][c]), c
  # QualitativeResults writes the first num_qualitative_results scenes
  class DS:
    def __init__(self, ids): self.ids = ids
    def __len__(self): return len(self.ids)
    def __getitem__(self, i):
      class El: pass
      e = El(); e.scene_id = self.ids[i]; return e
  qr = ER.QualitativeResults(DS(["x/s1", "x/s0"]), str(tmp_path), "fg_bg", num_qualitative_results=1)
  qr.add_batch(pmf, ex)
  files = sorted(os.listdir(tmp_path))
  assert files == ["img_x_s1.png"]
  png = np.array(PIL.Image.open(tmp_path / files[0]))
  assert png.shape == (5 * 384, 1920, 3) and np.array_equal(png, t.cat(rows[1], 0).numpy())


def test_semantic_labels(R):
  from corenet_amd import evaluation_results as ER
  pmf, ex = S.synthetic_example(B=1, R=16)
  pmf3 = t.cat([pmf, t.zeros(1, 1, 16, 16, 16)], 1)
  pmf3[0, 2, :8] = 2.0
  pred, gt = ER.extract_labels(pmf3, ex, "semantic")
  assert set(pred.unique().tolist()) == {0, 1, 2} and t.equal(gt, ex.grid)
  rows = ER.visualize_output(pmf3, ex, "semantic")
  assert rows[0][1].shape == (384, 1920, 3)
  predf, _ = ER.extract_labels(pmf, ex, "fg_bg")
  assert predf.max() == 1


def test_visualize_output_rejects_bad_indices(R):
  from corenet_amd import evaluation_results as ER
  pmf, ex = S.synthetic_example(B=2, R=8)
  with pytest.raises(ValueError):
    ER.visualize_output(pmf, ex, "fg_bg", [2])
  with pytest.raises(ValueError):
    ER.visualize_output(pmf[:1], ex, "fg_bg")
