"""Point-to-triangle distances and the mesh metrics built on them (corenet_amd.mesh_metrics), on CPU
tensors: the library's host twin against known answers and the float64 region-walk oracle of point_triangle_check.py."""
import math

import numpy as np
import pytest
import torch as t

import point_triangle_check as TC


@pytest.fixture(scope="module")
def MM():
  from corenet_amd import mesh_metrics as MM
  return MM


def _t(x):
  return t.from_numpy(np.array(x))


def _run(MM, pts, p_off, tri, t_off):
  d2, idx = MM.point_triangle_distances(_t(pts), _t(p_off), _t(tri), _t(t_off))
  assert d2.dtype == t.float32 and idx.dtype == t.int32 and d2.shape == idx.shape == (len(pts),)
  return d2.numpy(), idx.numpy()


def test_known_answers_in_every_region(MM):
  pts = np.array([q for q, _ in TC.REGIONS], np.float32)
  want = np.array([d for _, d in TC.REGIONS], np.float64)
  assert np.array_equal(pts.astype(np.float64), np.array([q for q, _ in TC.REGIONS]))       # exact in float32
  d2, idx = _run(MM, pts, TC.offsets([len(pts)]), TC.ONE, TC.offsets([1]))
  oracle = TC.closest_distances(pts, TC.ONE)[:, 0]
  assert (np.abs(oracle ** 2 - want) <= 1e-12 * want).all()                                  # the oracle knows them too
  assert (idx == 0).all()
  assert (np.abs(d2 - oracle ** 2) <= 1e-6 * want).all() and (np.abs(d2 - want) <= 1e-6 * want).all()
  assert (d2[want == 0] == 0).all()                                                          # on the triangle: exactly 0


def test_only_eligible_triangles_are_chosen(MM):
  pts, p_off, tri, t_off, want_idx, want_d2 = TC.eligibility_case()
  assert TC.eligible(tri).tolist() == [False, False, True] + [False] * 6 + [True]
  d2, idx = _run(MM, pts, p_off, tri, t_off)
  assert idx.tolist() == want_idx.tolist()
  assert np.array_equal(d2, want_d2)
  # the ineligible triangles really are closer: the oracle's distance to the point triangle is smaller
  o = TC.closest_distances(pts[:3], tri[:1])[:, 0]
  assert (o < np.sqrt(want_d2[:3])).all()


def test_ties_go_to_the_lowest_index(MM):
  pts, p_off, tri, t_off = TC.ties_case()
  d2, idx = _run(MM, pts, p_off, tri, t_off)
  n0 = p_off[1]
  oracle = TC.closest_distances(pts[:n0], tri[:2])
  assert np.array_equal(oracle[:, 0], oracle[:, 1])                                          # both triangles tie
  assert (idx[:n0] == 0).all() and d2[:n0].tolist() == [2, 4.25, 0, 3, 4.25]
  assert (np.abs(oracle[:, 0] ** 2 - d2[:n0]) <= 1e-12).all()
  dup = idx[n0:]
  assert (dup >= 0).all() and (dup < 200).all()                                              # never the copy
  # and the copy alone gives the same distances, 200 places later
  d2b, idxb = _run(MM, pts[n0:], TC.offsets([len(pts) - n0]), tri[202:], TC.offsets([200]))
  assert np.array_equal(d2b, d2[n0:]) and np.array_equal(idxb, dup)


def test_accuracy_against_the_oracle(MM):
  case = TC.accuracy_case()
  tri = case[2]
  e = TC.edge_lengths(tri)
  assert e.min() >= 0.01 and e.max() <= 0.2 and TC.min_angle_deg(tri).min() >= 15 and tri.min() >= 0 and tri.max() <= 1
  TC.check_accuracy(*_run(MM, *case[:4]), case, TC.TOL)


def test_slivers_stay_within_the_two_sided_bound(MM):
  case = TC.sliver_case()
  ang = TC.min_angle_deg(case[2])
  assert 0.01 <= ang.min() < 0.02 and ang.max() <= 1
  TC.check_slivers(*_run(MM, *case[:4]), case, TC.TOL_SLIVER)


def test_sizes_and_size_rule(MM):
  QT, TT = MM.point_triangle_tiles()
  assert (QT, TT) == (1024, 256)                          # what include/corenet_hip.h states
  # the constants are the kernel's: one share per tile of triangles, 1024 workgroups wanted
  assert MM.point_triangle_splits(1, 1, TT) == 1 and MM.point_triangle_splits(1, 1, TT + 1) == 2
  assert MM.point_triangle_splits(1, QT, 1 << 30) == 1024 and MM.point_triangle_splits(1, QT + 1, 1 << 30) == 512
  assert MM.point_triangle_splits(1024, QT, 1 << 20) == 1
  pts, p_off, tri, t_off = TC.sizes_case(QT, TT)
  d2, idx = _run(MM, pts, p_off, tri, t_off)
  for n in range(len(p_off) - 1):
    q = slice(p_off[n], p_off[n + 1])
    nt = t_off[n + 1] - t_off[n]
    if nt == 0:
      assert (idx[q] == -1).all() and np.isinf(d2[q]).all()
    elif p_off[n + 1] > p_off[n]:
      o = TC.closest_distances(pts[q], tri[t_off[n]:t_off[n + 1]])
      assert (np.abs(np.sqrt(d2[q].astype(np.float64)) - o.min(1)) <= TC.TOL).all()
      assert (o[np.arange(o.shape[0]), idx[q]] <= o.min(1) + TC.TOL).all()


def _soup(*pieces):
  return np.concatenate(pieces).astype(np.float32), TC.offsets([len(p) for p in pieces])


def test_same_square_in_two_tessellations(MM):
  """The reason the feature exists: the unit square as 2 triangles against the same square as 8 triangles."""
  a, a_off = _soup(TC.square(2, 0.0, 1))
  b, b_off = _soup(TC.square(2, 0.0, 2))
  assert len(a) == 2 and len(b) == 8
  m = MM.mesh_chamfer_fscore(_t(a), _t(a_off), _t(b), _t(b_off), TC.TAUS, num_samples=1024)
  assert isinstance(m, MM.MeshSurfaceMetrics) and m._fields[:11] == MM.SurfaceMetrics._fields
  assert float(m.accuracy[0]) <= 1e-6 and float(m.completeness[0]) <= 1e-6
  assert m.fscore.tolist() == [[1, 1, 1]] and m.precision_count.tolist() == [[1024] * 3]
  assert m.normal_consistency.tolist() == [1.0] and m.normal_consistency_pred.tolist() == [1.0]
  assert m.normal_consistency_gt.tolist() == [1.0] and m.normal_consistency.dtype == t.float64
  # sample to sample on the same two soups: the sampling floor, about 0.5 sqrt(1 / 1024) = 1.5e-2
  sa = MM.sample_surface_points(_t(a), offsets=_t(a_off), num_samples=1024)
  sb = MM.sample_surface_points(_t(b), offsets=_t(b_off), num_samples=1024)
  off = t.tensor([0, 1024])
  old = MM.chamfer_fscore(sa.points.reshape(-1, 3), off, sb.points.reshape(-1, 3), off, TC.TAUS)
  print("sample-to-sample chamfer_l1 of one square in two tessellations:", float(old.chamfer_l1[0]))
  assert float(old.chamfer_l1[0]) > 1e-4


def test_parallel_and_perpendicular_squares(MM):
  a, a_off = _soup(TC.square(2, 0.0), TC.square(2, 0.0))
  b, b_off = _soup(TC.square(2, 0.25), TC.square(0, 0.0))
  m = MM.mesh_chamfer_fscore(_t(a), _t(a_off), _t(b), _t(b_off), TC.TAUS, num_samples=1024)
  assert abs(float(m.accuracy[0]) - 0.25) <= 1e-6 and abs(float(m.completeness[0]) - 0.25) <= 1e-6
  assert m.precision[0].tolist() == [0, 0, 0] and m.fscore[0].tolist() == [0, 0, 0]
  assert float(m.normal_consistency[0]) == 1.0
  # z = 0 against x = 0, edges on the axes: the normals are e_z and e_x
  assert float(m.normal_consistency[1]) == 0.0 and float(m.normal_consistency_pred[1]) == 0.0
  assert float(m.normal_consistency_gt[1]) == 0.0 and 0 < float(m.accuracy[1]) < 1


def test_empty_objects_follow_the_chamfer_rules(MM):
  sq, bad = TC.square(2, 0.0), TC.bad_triangles()
  none = np.zeros((0, 3, 3), np.float32)
  # objects: both present, pred empty, gt without an eligible triangle (counts as empty), both empty
  a, a_off = _soup(sq, none, sq, bad)
  b, b_off = _soup(sq, sq, bad, none)
  m = MM.mesh_chamfer_fscore(_t(a), _t(a_off), _t(b), _t(b_off), TC.TAUS, num_samples=256, seed=5)
  assert m.num_pred.tolist() == [256, 0, 256, 0] and m.num_gt.tolist() == [256, 256, 0, 0]
  assert float(m.chamfer_l1[0]) <= 1e-6 and float(m.normal_consistency[0]) == 1.0
  for n in (1, 2):
    assert math.isinf(float(m.accuracy[n])) and math.isinf(float(m.completeness[n])) and math.isinf(float(m.chamfer_l1[n]))
    assert m.fscore[n].tolist() == [0, 0, 0]
    assert [float(x[n]) for x in (m.normal_consistency, m.normal_consistency_pred, m.normal_consistency_gt)] == [0, 0, 0]
  for field in m:
    if field.dtype == t.float64:
      assert bool(t.isnan(field[3]).all())
  again = MM.mesh_chamfer_fscore(_t(a), _t(a_off), _t(b), _t(b_off), TC.TAUS, num_samples=256, seed=5)
  for x, y in zip(m, again):
    assert t.equal(t.isnan(x), t.isnan(y)) and t.equal(x[~t.isnan(x)], y[~t.isnan(y)])    # bit for bit


def test_bad_arguments_raise_value_error(MM):
  p, tri = t.zeros((4, 3)), t.zeros((2, 3, 3))
  off = t.tensor([0, 4])
  with pytest.raises(ValueError):
    MM.point_triangle_distances(p.double(), off, tri, t.tensor([0, 2]))
  with pytest.raises(ValueError):
    MM.point_triangle_distances(p, off, tri.reshape(2, 9), t.tensor([0, 2]))
  with pytest.raises(ValueError):
    MM.point_triangle_distances(p, off, tri, t.tensor([0, 3]))
  with pytest.raises(ValueError):
    MM.point_triangle_distances(p, off, tri, t.tensor([0, 1, 2]))
  with pytest.raises(ValueError):
    MM.mesh_chamfer_fscore(tri, t.tensor([0, 2]), tri, t.tensor([0, 2]), [-0.1])
  with pytest.raises(ValueError):
    MM.mesh_chamfer_fscore(tri, t.tensor([0, 2]), tri, t.tensor([0, 1, 2]), [0.1])
  d2, idx = MM.point_triangle_distances(t.zeros((0, 3)), t.tensor([0, 0]), tri, t.tensor([0, 2]))
  assert d2.shape == (0,) and idx.shape == (0,)


@pytest.fixture(scope="module")
def fixture_batch():
  return TC.fixture_batch_cpu()


def test_triangle_distance_never_exceeds_the_sample_distance(MM, fixture_batch):
  """The gt samples lie on the gt triangles, so for the same pred samples the distance to the triangles is at most the
  distance to the nearest sample, for every query."""
  from corenet_amd import evaluation_results as ER
  from corenet_amd.visualization import marching_cubes
  pmf, ex = fixture_batch
  S, seed = 1024, 3
  fg = t.stack([pmf[:, 0], pmf[:, 1:].max(1)[0]], 1)
  inv = t.stack([ex.v2x_transform[b].inverse() for b in range(2)])
  mesh = marching_cubes(fg[:, 1], level=0.5, matrices=inv)
  nv = t.cumsum(mesh.num_vertices, 0) - mesh.num_vertices
  own = t.repeat_interleave(t.arange(2), mesh.num_faces)
  pred_tri = mesh.vertices[mesh.faces.long() + nv[own][:, None]]
  assert int(mesh.num_faces.min()) > 0
  gt_tri = ex.vertices
  gt_off = t.tensor([0] + [int(v.sum()) for v in ex.mesh_num_tri]).cumsum(0)
  pred = MM.sample_surface_points(pred_tri, mesh.num_faces, S, seed)
  gt = MM.sample_surface_points(gt_tri, offsets=gt_off, num_samples=S, seed=seed)
  assert bool(pred.valid.all()) and bool(gt.valid.all())
  off = t.arange(3) * S
  d2_nn, _ = MM.nearest_distances(pred.points.reshape(-1, 3), off, gt.points.reshape(-1, 3), off)
  d2_tri, idx = MM.point_triangle_distances(pred.points.reshape(-1, 3), off, gt_tri, gt_off)
  assert bool((idx >= 0).all())
  gap = d2_tri.double().sqrt() - d2_nn.double().sqrt()
  print("largest sqrt(d2_triangle) - sqrt(d2_sample):", float(gap.max()), "mean gain:", float(-gap.mean()))
  assert bool((gap <= 1e-6).all())
  # and this is what surface_metrics_for_batch measures in either mode
  rows_t = ER.surface_metrics_for_batch(fg, ex, "fg_bg", num_samples=S, thresholds=TC.TAUS, seed=seed, distance="triangles")
  rows_p = ER.surface_metrics_for_batch(fg, ex, "fg_bg", num_samples=S, thresholds=TC.TAUS, seed=seed)
  want_t = d2_tri.double().sqrt().reshape(2, S).mean(1)
  want_p = d2_nn.double().sqrt().reshape(2, S).mean(1)
  assert bool(((rows_t.metrics.accuracy - want_t).abs() <= 1e-12 * want_t).all())
  assert bool(((rows_p.metrics.accuracy - want_p).abs() <= 1e-12 * want_p).all())
  assert bool((rows_t.metrics.accuracy <= rows_p.metrics.accuracy + 1e-6).all())


def test_distance_modes_of_surface_metrics_for_batch(MM, fixture_batch):
  from corenet_amd import evaluation_results as ER
  pmf, ex = fixture_batch
  kw = dict(num_samples=512, thresholds=TC.TAUS, seed=1)
  default = ER.surface_metrics_for_batch(pmf, ex, "semantic", **kw)
  points = ER.surface_metrics_for_batch(pmf, ex, "semantic", distance="points", **kw)
  tri = ER.surface_metrics_for_batch(pmf, ex, "semantic", distance="triangles", **kw)
  assert type(default.metrics) is MM.SurfaceMetrics and type(points.metrics) is MM.SurfaceMetrics
  for x, y in zip(default.metrics, points.metrics):
    assert x.dtype == y.dtype and t.equal(t.isnan(x), t.isnan(y)) and t.equal(x[~t.isnan(x)], y[~t.isnan(y)])
  assert type(tri.metrics) is MM.MeshSurfaceMetrics
  assert tri.scene_index.tolist() == default.scene_index.tolist() == [0, 0, 0, 1, 1, 1]
  assert tri.class_index.tolist() == default.class_index.tolist() and tri.scene_id == default.scene_id
  assert tri.thresholds == default.thresholds
  assert t.equal(tri.metrics.num_pred, default.metrics.num_pred) and t.equal(tri.metrics.num_gt, default.metrics.num_gt)
  both = (default.metrics.num_pred > 0) & (default.metrics.num_gt > 0)
  assert bool(both.any())
  assert bool((tri.metrics.chamfer_l1[both] <= default.metrics.chamfer_l1[both] + 1e-6).all())
  nc = tri.metrics.normal_consistency[both]
  assert bool(((nc >= 0) & (nc <= 1)).all())
  assert t.equal(t.isnan(tri.metrics.chamfer_l1), t.isnan(default.metrics.chamfer_l1))
  for gt_source in ("mesh", "grid"):
    with pytest.raises(ValueError):
      ER.surface_metrics_for_batch(pmf, ex, "semantic", distance="voxels", gt_source=gt_source, **kw)
  with pytest.raises(ValueError):
    ER.SurfaceResults("semantic", distance="voxels")
  grid = ER.surface_metrics_for_batch(pmf, ex, "semantic", distance="triangles", gt_source="grid", **kw)
  assert type(grid.metrics) is MM.MeshSurfaceMetrics and grid.class_index.tolist() == default.class_index.tolist()


def test_surface_results_carry_normal_consistency(fixture_batch):
  from corenet_amd import evaluation_results as ER
  pmf, ex = fixture_batch
  old = ER.SurfaceResults("semantic", num_samples=256, thresholds=[0.05])
  old.add_batch(pmf, ex)
  s_old = old.summary()
  assert sorted(s_old["overall"]) == ["chamfer_l1", "fscore", "num_rows"]                   # the default is what it was
  res = ER.SurfaceResults("semantic", num_samples=256, thresholds=[0.05], distance="triangles")
  rows = res.add_batch(pmf, ex)
  s = res.summary()
  nc, cls = rows.metrics.normal_consistency.numpy(), rows.class_index.numpy()
  assert sorted(s["overall"]) == ["chamfer_l1", "fscore", "normal_consistency", "num_rows"]
  with np.errstate(invalid="ignore"):
    assert s["overall"]["normal_consistency"] == pytest.approx(np.nanmean(nc), rel=1e-12)
    for c in sorted(s["per_class"]):
      sel = nc[cls == c]
      if np.isnan(sel).all():
        assert math.isnan(s["per_class"][c]["normal_consistency"])
      else:
        assert s["per_class"][c]["normal_consistency"] == pytest.approx(np.nanmean(sel), rel=1e-12)
