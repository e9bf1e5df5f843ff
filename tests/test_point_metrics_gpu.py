"""corenet_amd.mesh_metrics on the MI355X: the kernels of csrc/point_metrics.hip against the library's host twin, bit for
bit, the split-candidate path, determinism, and the evaluation plumbing (surface_metrics_for_batch, SurfaceResults)."""
import math
import os

import numpy as np
import pytest
import torch as t

import point_metrics_check as PC

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def MM():
  from corenet_amd import mesh_metrics as MM
  return MM


def _t(x):
  return t.from_numpy(np.array(x))


@pytest.mark.parametrize("kind", ["sizes", "ties", "nan"])
def test_nearest_gpu_equals_twin_and_numpy(MM, kind):
  a, a_off, b, b_off, d2, idx = PC.nearest_case(kind)
  g_d2, g_idx = MM.nearest_distances(_t(a).cuda(), _t(a_off).cuda(), _t(b).cuda(), _t(b_off))
  c_d2, c_idx = MM.nearest_distances(_t(a), _t(a_off), _t(b), _t(b_off))
  assert g_d2.is_cuda and g_idx.is_cuda and g_d2.dtype == t.float32 and g_idx.dtype == t.int32
  assert t.equal(g_idx.cpu(), c_idx) and t.equal(g_d2.cpu(), c_d2)
  assert np.array_equal(g_idx.cpu().numpy(), idx) and np.array_equal(g_d2.cpu().numpy(), d2)


def test_nearest_split_candidates_is_exact_and_deterministic(MM):
  """2 objects x 3000 queries x 20000 candidates: too few query tiles to fill the chip, so the candidates of an object
  are split over workgroups and merged with the 64-bit atomicMin; duplicated candidates across the shares make the
  tie rule visible; one query is NaN, one candidate is NaN."""
  rng = np.random.RandomState(21)
  a = (rng.randint(-64, 65, (6000, 3)) / 64.0).astype(np.float32)
  b = (rng.randint(-64, 65, (40000, 3)) / 64.0).astype(np.float32)
  b[30000:40000] = b[20000:30000]                        # object 1: the second half repeats the first
  a[17, 1] = np.nan
  b[123, 2] = np.nan
  a_off, b_off = PC.offsets([3000, 3000]), PC.offsets([20000, 20000])
  args = (_t(a).cuda(), _t(a_off), _t(b).cuda(), _t(b_off))
  d2_1, i_1 = MM.nearest_distances(*args)
  d2_2, i_2 = MM.nearest_distances(*args)
  assert t.equal(d2_1, d2_2) and t.equal(i_1, i_2)
  c_d2, c_idx = MM.nearest_distances(_t(a), _t(a_off), _t(b), _t(b_off))
  assert t.equal(i_1.cpu(), c_idx) and t.equal(d2_1.cpu(), c_d2)
  assert int(i_1[17]) == -1 and math.isinf(float(d2_1[17])) and int((i_1 == 123)[:3000].sum()) == 0
  assert int(i_1[3000:].max()) < 10000                   # ties went to the lower index, across the shares
  r_d2, r_idx = PC.np_nearest(a[:3000], PC.offsets([3000]), b[:20000], PC.offsets([20000]))
  assert np.array_equal(i_1[:3000].cpu().numpy(), r_idx) and np.array_equal(d2_1[:3000].cpu().numpy(), r_d2)


@pytest.mark.parametrize("S", [1000, 7, 2500])
def test_sample_surface_gpu_equals_twin(MM, S):
  tri, counts = PC.sampling_soup()
  big = (np.random.RandomState(8).rand(3000, 3, 3) * 2 - 1).astype(np.float32)       # more than one scan round of 1024
  tri, counts = np.concatenate([tri, big]), counts + [len(big)]
  g = MM.sample_surface_points(_t(tri).cuda(), counts, num_samples=S, seed=12345)
  c = MM.sample_surface_points(_t(tri), counts, num_samples=S, seed=12345)
  assert g.points.is_cuda and g.valid.dtype == t.bool and g.valid.tolist() == [True, True, False, False, True, True]
  for x, y in zip(g, c):
    assert t.equal(x.cpu(), y)
  again = MM.sample_surface_points(_t(tri).cuda(), counts, num_samples=S, seed=12345)
  assert all(t.equal(x, y) for x, y in zip(g, again))


def test_chamfer_fscore_gpu_against_twin(MM):
  tri, counts = PC.sampling_soup()
  p = MM.sample_surface_points(_t(tri), counts, num_samples=1500, seed=1)
  q = MM.sample_surface_points(_t(tri + np.float32(0.03)), counts, num_samples=1100, seed=2)
  keep = t.tensor([0, 1, 4])
  pp, qq = p.points[keep].reshape(-1, 3), q.points[keep].reshape(-1, 3)
  # objects: both present (x2), pred empty, both empty, gt empty
  p_off = t.tensor([0, 1500, 3000, 3000, 3000, 4500])
  q_off = t.tensor([0, 1100, 2200, 3300, 3300, 3300])
  taus = [0.02, 0.04, 0.2]
  c = MM.chamfer_fscore(pp, p_off, qq, q_off, taus)
  g = MM.chamfer_fscore(pp.cuda(), p_off, qq.cuda(), q_off.cuda(), taus)
  for name in ("precision_count", "recall_count", "num_pred", "num_gt"):
    assert t.equal(getattr(g, name).cpu(), getattr(c, name)), name
  for name in ("accuracy", "completeness", "chamfer_l1", "chamfer_l2", "precision", "recall", "fscore"):
    x, y = getattr(g, name).cpu(), getattr(c, name)
    assert x.dtype == t.float64 and t.equal(t.isnan(x), t.isnan(y)) and t.equal(t.isinf(x), t.isinf(y)), name
    fin = t.isfinite(y)
    # float64 sums of identical float32 values in another order
    assert bool(((x[fin] - y[fin]).abs() <= 1e-12 * y[fin].abs()).all()), name
  assert t.isnan(c.chamfer_l1[3]) and math.isinf(float(c.chamfer_l1[2])) and c.fscore[2].tolist() == [0, 0, 0]
  assert math.isinf(float(c.chamfer_l1[4])) and c.fscore[4].tolist() == [0, 0, 0]


def _synthetic_batch(R=32):
  """A box and an L-shaped solid written straight into `grid` (fg_bg: labels 0 / 1), nothing touching the border."""
  from corenet_amd.data.batched_example import BatchedExample
  from corenet_amd.geometry import transformations as T
  grid = t.zeros((2, R, R, R), dtype=t.int32)
  grid[0, 6:14, 8:18, 5:13] = 1
  grid[1, 4:16, 6:11, 7:15] = 1
  grid[1, 4:9, 11:18, 7:15] = 1
  one = t.tensor([[[0.1, 0.1, 0.1], [0.9, 0.1, 0.1], [0.1, 0.9, 0.1]]])
  ex = BatchedExample(
      vertices=t.cat([one, one]), view_transform=t.eye(4).expand(2, 4, 4).clone(),
      camera_transform=t.eye(4).expand(2, 4, 4).clone(), mesh_num_tri=[t.tensor([1], dtype=t.int32)] * 2,
      mesh_labels=[t.tensor([1], dtype=t.int32)] * 2, input_image=t.zeros((2, 3, 8, 8), dtype=t.uint8),
      scene_id=["syn/box", "syn/ell"], grid_sampling_offset=t.full((2, 3), 0.5),
      v2x_transform=T.scale([float(R)] * 3).expand(2, 4, 4).clone(), grid=grid)
  return ex.cuda()


def test_surface_metrics_on_synthetic_grids():
  from corenet_amd import evaluation_results as ER
  from corenet_amd.visualization import marching_cubes
  R, S = 32, 16384
  ex = _synthetic_batch(R)
  onehot = t.stack([(ex.grid == 0), (ex.grid == 1)], 1).float()
  rows = ER.surface_metrics_for_batch(onehot, ex, "fg_bg", num_samples=S, thresholds=[1e-6, 3 / R], gt_source="grid")
  m = rows.metrics
  assert rows.scene_index.tolist() == [0, 1] and rows.class_index.tolist() == [1, 1] and rows.scene_id == ["syn/box", "syn/ell"]
  assert m.chamfer_l1.tolist() == [0, 0] and m.chamfer_l2.tolist() == [0, 0] and (m.fscore == 1).all()
  assert m.num_pred.tolist() == [S, S] and m.accuracy.is_cuda
  # the prediction shifted one voxel along w: every predicted point is 1 / R from a ground-truth surface point.  Every
  # triangle with S a_k / A > 2.5 holds a sample (its interval covers more than two strata; the half is the weight
  # quantisation), and a marching-cubes triangle lies inside one cell, so a sample of the same triangle is at most a
  # cell diagonal sqrt(3) / R away: the sampler's spacing bound here.
  mesh = marching_cubes(onehot[:, 1], level=0.5)
  nv = t.cumsum(mesh.num_vertices, 0) - mesh.num_vertices
  own = t.repeat_interleave(t.arange(2, device="cuda"), mesh.num_faces)
  tri = mesh.vertices[mesh.faces.long() + nv[own][:, None]].cpu().numpy()
  area = PC.areas64(tri)
  for n in range(2):
    a = area[(own == n).cpu().numpy()]
    assert S * a.min() / a.sum() > 2.5
  shifted = onehot.roll(1, dims=4)
  rows = ER.surface_metrics_for_batch(shifted, ex, "fg_bg", num_samples=S, thresholds=[3 / R], gt_source="grid")
  m = rows.metrics
  bound = 1 / R + math.sqrt(3) / R
  assert bound < 3 / R
  for v in m.accuracy.tolist() + m.completeness.tolist():
    assert 0 < v <= bound
  assert (m.fscore == 1).all() and (m.precision_count == S).all() and (m.recall_count == S).all()


@pytest.fixture(scope="module")
def fixture_batch():
  """The two fixture scenes voxelized at 32^3 (semantic) and a pmf near the ground truth, on the GPU."""
  from corenet_amd import pipeline
  from corenet_amd.data import batched_example as B, dataset as D
  root = os.path.join(G, "n2_dataset")
  ds = D.CoReNetDatasetImpl(os.path.join(root, "dataset.json"), os.path.join(root, "meshes"))
  ex = pipeline.voxelize_batch(B.batch([ds[0], ds[1]]), "semantic", resolution=(32, 32, 32))
  nc = 4
  noise = t.randn((2, nc, 32, 32, 32), generator=t.Generator().manual_seed(7)) * 0.3
  onehot = t.nn.functional.one_hot(ex.grid.to(t.int64).clamp(0, nc - 1), nc).permute(0, 4, 1, 2, 3).float()
  return (noise.cuda() + 2 * onehot).softmax(1), ex


def test_surface_metrics_against_fixture_meshes(MM, fixture_batch):
  from corenet_amd import evaluation_results as ER
  from corenet_amd.visualization import marching_cubes
  pmf, ex = fixture_batch
  S, taus, C = 2048, [0.02, 0.05, 0.2], pmf.shape[1]
  rows = ER.surface_metrics_for_batch(pmf, ex, "semantic", num_samples=S, thresholds=taus, seed=3)
  m = rows.metrics
  assert rows.scene_index.tolist() == [0, 0, 0, 1, 1, 1] and rows.class_index.tolist() == [1, 2, 3, 1, 2, 3]
  # the composition by hand: one marching-cubes call through inverse(v2x), the class meshes in batch order, same seed
  K = C - 1
  inv = [ex.v2x_transform[b].cpu().float().inverse() for b in range(2)]
  mats = t.stack([inv[b] for b in range(2) for _ in range(K)]).cuda()
  mesh = marching_cubes(pmf[:, 1:].reshape(2 * K, 32, 32, 32), level=0.5, matrices=mats)
  nv = t.cumsum(mesh.num_vertices, 0) - mesh.num_vertices
  own = t.repeat_interleave(t.arange(2 * K, device="cuda"), mesh.num_faces)
  pred = MM.sample_surface_points(mesh.vertices[mesh.faces.long() + nv[own][:, None]], mesh.num_faces, S, seed=3)
  num_tri = [v.long() for v in ex.mesh_num_tri]
  labels = [t.as_tensor(v).long().reshape(-1) for v in ex.mesh_labels]
  pieces, cnt, start, present = [], [], 0, []
  for b in range(2):
    for k in range(1, C):
      n = 0
      for j in range(len(num_tri[b])):
        first = start + int(num_tri[b][:j].sum())
        if int(labels[b][j]) == k:
          pieces.append(ex.vertices[first:first + int(num_tri[b][j])])
          n += int(num_tri[b][j])
      cnt.append(n)
      present.append(n > 0 or int(mesh.num_faces[b * K + k - 1]) > 0)
    start += int(num_tri[b].sum())
  gt = MM.sample_surface_points(t.cat(pieces), cnt, S, seed=3)

  def pack(s):
    v = s.valid.cpu()
    return s.points[v.cuda()].reshape(-1, 3), t.cat([t.zeros(1, dtype=t.int64), t.cumsum(v.long() * S, 0)])
  hand = MM.chamfer_fscore(*pack(pred), *pack(gt), taus)
  for x, y in zip(m, hand):
    assert t.equal(t.isnan(x), t.isnan(y)) and t.equal(x[~t.isnan(x)], y[~t.isnan(y)])
  # one finite-or-inf row per class present on either side, NaN rows for the others; F in [0, 1]
  assert (~t.isnan(m.chamfer_l1)).cpu().tolist() == present and sum(present) >= 2
  both = t.tensor([c > 0 for c in cnt]) & (mesh.num_faces > 0).cpu()
  assert bool(t.isfinite(m.chamfer_l1.cpu()[both]).all()) and bool(both.any())
  f = m.fscore[~t.isnan(m.fscore)]
  assert bool(((f >= 0) & (f <= 1)).all())
  # fg_bg: all meshes of a scene against the one foreground class
  fg = t.stack([pmf[:, 0], pmf[:, 1:].sum(1)], 1)
  r2 = ER.surface_metrics_for_batch(fg, ex, "fg_bg", num_samples=S, thresholds=taus)
  assert r2.class_index.tolist() == [1, 1] and bool(t.isfinite(r2.metrics.chamfer_l1).all())
  assert r2.metrics.num_gt.tolist() == [S, S]


def test_surface_results_summary(fixture_batch):
  from corenet_amd import evaluation_results as ER
  pmf, ex = fixture_batch
  res = ER.SurfaceResults("semantic", num_samples=1024, thresholds=[0.05, 0.2], gt_source="grid")
  r1 = res.add_batch(pmf, ex)
  r2 = res.add_batch(pmf.flip(0), ex)                    # a second batch with the predictions swapped
  s = res.summary()
  cd = np.concatenate([r1.metrics.chamfer_l1.cpu().numpy(), r2.metrics.chamfer_l1.cpu().numpy()])
  f = np.concatenate([r1.metrics.fscore.cpu().numpy(), r2.metrics.fscore.cpu().numpy()])
  cls = np.concatenate([r1.class_index.numpy(), r2.class_index.numpy()])
  assert len(cd) == 12

  def same(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == pytest.approx(b, rel=1e-12)
  with np.errstate(invalid="ignore"):
    assert same(s["overall"]["chamfer_l1"], np.nanmean(cd))
    for k in range(2):
      assert same(s["overall"]["fscore"][k], np.nanmean(f[:, k]))
    assert sorted(s["per_class"]) == [1, 2, 3] and s["thresholds"] == [0.05, 0.2]
    for c in (1, 2, 3):
      if np.isnan(cd[cls == c]).all():
        assert np.isnan(s["per_class"][c]["chamfer_l1"]) and s["per_class"][c]["num_rows"] == 0
      else:
        assert same(s["per_class"][c]["chamfer_l1"], np.nanmean(cd[cls == c]))
        assert same(s["per_class"][c]["fscore"][1], np.nanmean(f[cls == c][:, 1]))
