"""corenet_amd.visualization rendering on the MI355X: the HIP renderer and voxel-face kernels against the library's
host twin, bit for bit, the reference's golden images, determinism, batching and the qualitative-results path."""
import os
import signal

import numpy as np
import pytest
import torch as t

import mesh_check as MC
import render_scenes as S

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def R():
  from corenet_amd.visualization import render as R
  return R


class limit:
  """Wall-clock limit of one GPU step (SIGALRM); a step that overruns fails its test instead of hanging the run."""

  def __init__(self, seconds: int):
    self.seconds = seconds

  def __enter__(self):
    def boom(*_):
      raise TimeoutError(f"GPU step exceeded {self.seconds} s")
    self.prev = signal.signal(signal.SIGALRM, boom)
    signal.alarm(self.seconds)

  def __exit__(self, *exc):
    signal.alarm(0)
    signal.signal(signal.SIGALRM, self.prev)
    return False


def _gpu(fn, seconds=120):
  with limit(seconds):
    out = fn()
    t.cuda.synchronize()
  return out


def _soup(rng, T, spread=1.0):
  tri = (rng.rand(T, 3, 3).astype(np.float32) - 0.5) * 2 * spread
  tri[:, :, 2] = tri[:, :, 2] * 0.5 + 2.5                            # in front of a camera at the origin looking +z
  tri[T // 2:T // 2 + T // 8] = tri[:T // 8]                         # coplanar duplicates
  return t.from_numpy(tri)


def _both(R, tri, mids, mats, ranges, vps, size, **kw):
  g = _gpu(lambda: R.render_batch(tri.cuda(), mids.cuda(), mats.cuda(), ranges, vps, size,
                                  **{k: (v.cuda() if k == "normals" and v is not None else v) for k, v in kw.items()}))
  c = R.render_batch(tri, mids, mats, ranges, vps, size, **kw)
  assert g.device.type == "cuda" and g.dtype == t.uint8
  assert t.equal(g.cpu(), c), int((g.cpu() != c).any(-1).sum())
  return g


def _lh_camera(eye, at=(0.0, 0.0, 2.5)):
  from corenet_amd.geometry import transformations as T
  from corenet_amd.visualization import camera_util as C
  return t.matmul(C.perspective_projection(1.0, znear=0.1, zfar=10), T.look_at_lh(eye, at, (0, 1, 0)))


def test_golden_images_on_gpu_equal_twin():
  for name, fn in (("mesh", S.mesh_scene), ("voxels", S.voxel_scene)):
    g = _gpu(lambda: fn("cuda"))
    assert g.device.type == "cuda"
    c = fn("cpu")
    assert t.equal(g.cpu(), c), name
    l1, ndiff, cov, cov_ref = S.golden_stats(g.cpu().numpy(), name)
    assert l1 <= 1024 and cov == cov_ref, (name, l1, ndiff)


def test_triangle_soups_equal_twin_and_deterministic(R):
  rng = np.random.RandomState(1)
  tri = _soup(rng, 3000)
  nrm = t.from_numpy(rng.randn(3000, 3, 3).astype(np.float32))
  mids = t.from_numpy(rng.randint(0, 5, 3000).astype(np.int32))
  mats = R.make_materials(t.from_numpy(rng.rand(5, 3).astype(np.float32)))
  cams = [_lh_camera((0.0, 0.0, 0.0)), _lh_camera((0.5, 0.3, -0.2)), _lh_camera((-1.0, 2.0, 0.5))]
  ranges = [[0, 3000], [100, 2500], [0, 0], [2999, 3000], [0, 3000]]
  vps = t.stack(cams + cams[:2])
  modes = [0, 1, 1, 0, 2]
  a = _both(R, tri, mids, mats, ranges, vps, (200, 300), normals=nrm, normal_modes=modes,
            cull_back_facing=[False, True, False, False, True])
  b = _gpu(lambda: R.render_batch(tri.cuda(), mids.cuda(), mats.cuda(), ranges, vps, (200, 300), normals=nrm.cuda(),
                                  normal_modes=modes, cull_back_facing=[False, True, False, False, True]))
  assert t.equal(a, b)
  # one batched call == the same images one by one
  for i in range(5):
    one = _gpu(lambda: R.render_batch(tri.cuda(), mids.cuda(), mats.cuda(), [ranges[i]], vps[i:i + 1], (200, 300),
                                      normals=nrm.cuda(), normal_modes=[modes[i]],
                                      cull_back_facing=[False, True, False, False, True][i]))
    assert t.equal(one[0], a[i]), i
  # specular materials: powf may differ by one level
  mats_s = R.make_materials(t.from_numpy(rng.rand(5, 3).astype(np.float32)), 0.05, (0.5, 0.5, 0.5), 16.0)
  g = _gpu(lambda: R.render_batch(tri.cuda(), mids.cuda(), mats_s.cuda(), ranges[:2], vps[:2], (128, 128),
                                  normals=nrm.cuda(), normal_modes=[1, 1]))
  c = R.render_batch(tri, mids, mats_s, ranges[:2], vps[:2], (128, 128), normals=nrm, normal_modes=[1, 1])
  assert (g.cpu().to(t.int32) - c.to(t.int32)).abs().max() <= 1


def test_near_plane_cases_equal_twin(R):
  from corenet_amd.geometry import transformations as T
  rng = np.random.RandomState(2)
  tri = t.from_numpy((rng.rand(500, 3, 3).astype(np.float32) - 0.5) * 6)    # around and behind the eye
  mats = R.make_materials(t.from_numpy(rng.rand(3, 3).astype(np.float32)))
  mids = t.from_numpy(rng.randint(0, 3, 500).astype(np.int32))
  proj = T.perspective_rh(1.2, 1.0, 0.5, 4.0)
  vps = t.stack([proj, t.matmul(proj, T.look_at_rh((0.3, 0.2, 0.1), (0, 0, -1), (0, 1, 0)))])
  _both(R, tri, mids, mats, [[0, 500], [0, 500]], vps, (96, 128))


def test_marching_cubes_sphere_128_equal_twin(R):
  from corenet_amd.visualization import camera_util as C
  from corenet_amd.visualization.marching_cubes import to_marching_cubes
  g = t.from_numpy(MC.ellipsoid_fields(1, 128, seed=3))
  m = _gpu(lambda: to_marching_cubes(g.cuda()))
  tri, nrm, cnt = (x.cpu() for x in m)
  mats = R.make_materials(t.tensor([[0.7, 0.4, 0.2]]))
  cam = C.get_default_camera_for_mesh(tri)
  views = t.stack([cam] + [t.matmul(C.perspective_projection(), v) @ t.diag(t.tensor([1 / 128.0] * 3 + [1.0]))
                           for v in C.cameras_on_tetrahedron_vertices()])
  views[1:, :, 3] += views[1:, :, 2] * 1.5
  T_ = tri.shape[0]
  _both(R, tri, t.zeros(T_, dtype=t.int32), mats, [[0, T_]] * 5, views, (384, 384), normals=nrm)


def test_voxel_faces_and_grids_equal_twin(R):
  from corenet_amd.visualization import artifacts as A
  from corenet_amd.visualization import camera_util as C
  from corenet_amd.visualization.colors import DEFAULT_COLOR_PALETTE
  rng = np.random.RandomState(4)
  pal = t.as_tensor(DEFAULT_COLOR_PALETTE)
  rand = t.from_numpy(rng.randint(0, 20, (3, 32, 32, 32)).astype(np.int32) * (rng.rand(3, 32, 32, 32) < 0.3))
  z = t.linspace(-1, 1, 128)
  blob = ((z[:, None, None] ** 2 + 1.5 * z[None, :, None] ** 2 + z[None, None, :] ** 2) < 0.5).to(t.int32) * 3
  blob = A.VoxelGridArtifact.draw_frame(blob.clone(), 5)[None]
  for grid, side in ((rand, 32), (blob, 128)):
    N = grid.shape[0]
    mats = t.stack([t.diag(t.tensor([1 / side] * 3 + [1.0])) for _ in range(N)])
    mats[:, :3, 3] = t.from_numpy(rng.randn(N, 3).astype(np.float32)) * 0.01
    box = t.stack([C.frontal_camera(0.3) @ m for m in mats])
    fg = _gpu(lambda: R.voxel_faces(grid.cuda(), pal, mats, material_base=3, box_matrices=box))
    fc = R.voxel_faces(grid, pal, mats, material_base=3, box_matrices=box)
    for x, y in zip(fg, fc):
      assert t.equal(x.cpu(), y)
    T_ = fc.triangles.shape[0]
    vm = R.voxel_materials(t.cat([t.zeros(3, 3), pal], 0))
    starts = t.cumsum(fc.num_triangles, 0) - fc.num_triangles
    ranges = [[int(s), int(s + c)] for s, c in zip(starts, fc.num_triangles)]
    cams = [C.get_default_camera_for_mesh(fc.triangles[r[0]:r[1]]) for r in ranges]
    _both(R, fc.triangles, fc.material_ids, vm, ranges, t.stack(cams), (384, 384), normals=fc.normals,
          normal_modes=[2] * N)
    img = _gpu(lambda: R.render_voxel_grid(grid[0].cuda()))
    assert t.equal(img.cpu(), R.render_voxel_grid(grid[0]))


def test_visualize_output_on_fixture_batch():
  import dataclasses
  from corenet_amd import evaluation_results as ER
  from corenet_amd import pipeline
  from corenet_amd.data import batched_example as B, dataset as D
  root = os.path.join(G, "n2_dataset")
  ds = D.CoReNetDatasetImpl(os.path.join(root, "dataset.json"), os.path.join(root, "meshes"))
  els = [ds[0], ds[1]]
  for task in ("semantic",):             # fg_bg needs one mesh per scene (the reference asserts it); the scenes have 2 and 3
    ex = _gpu(lambda: pipeline.voxelize_batch(B.batch(els), task))
    nc = 2 if task == "fg_bg" else 4
    rng = t.Generator(device="cuda").manual_seed(7)
    logits = t.randn((2, nc) + tuple(ex.grid.shape[1:]), device="cuda", generator=rng) * 0.3
    onehot = t.nn.functional.one_hot(ex.grid.to(t.int64).clamp(0, nc - 1), nc).permute(0, 4, 1, 2, 3).float()
    pmf = (logits + 2 * onehot).softmax(1)
    gpu = _gpu(lambda: ER.visualize_output(pmf, ex, task), 300)
    cpu = ER.visualize_output(pmf.cpu(), ex.cpu(), task)
    for rg, rc in zip(gpu, cpu):
      assert len(rg) == 5
      for a, b in zip(rg, rc):
        assert a.device.type == "cuda" and a.shape == (384, 1920, 3)
        assert t.equal(a.cpu(), b), int((a.cpu() != b).any(-1).sum())
      assert all(r[:, 384:].any() for r in rg)


def test_qualitative_png_of_fixture_scene_is_golden(tmp_path):
  """QualitativeResults' PNG of the first fixture scene, on the GPU and through the host twin, equals the committed
  image bit for bit (tests/golden/render/qualitative_n2_s0.png, made by this recipe on an MI355X)."""
  import PIL.Image
  pmf, ex = _gpu(lambda: S.fixture_eval_batch(), 300)
  gpu = _gpu(lambda: S.write_qualitative(pmf, ex, str(tmp_path / "gpu")), 300)
  cpu = S.write_qualitative(pmf.cpu(), ex.cpu(), str(tmp_path / "cpu"))
  a, b = np.array(PIL.Image.open(gpu)), np.array(PIL.Image.open(cpu))
  assert a.shape == (5 * 384, 1920, 3) and np.array_equal(a, b)
  golden = np.array(PIL.Image.open(S.QUALITATIVE_GOLDEN))
  assert np.array_equal(a, golden), int((a != golden).any(-1).sum())
