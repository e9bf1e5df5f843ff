"""Point-to-triangle distances on the MI355X (csrc/point_metrics.hip): the kernel equals the host twin
bit for bit on every input of the CPU tests, on the tile edges and through the split launch; the mesh metrics and the
evaluation plumbing on the GPU equal their CPU results."""
import math

import numpy as np
import pytest
import torch as t

import point_triangle_check as TC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def MM():
  from corenet_amd import mesh_metrics as MM
  return MM


def _t(x):
  return t.from_numpy(np.array(x))


def _both(MM, pts, p_off, tri, t_off):
  """The kernel's (d2, index) as numpy, after asserting that the host twin returns the same bits."""
  g_d2, g_idx = MM.point_triangle_distances(_t(pts).cuda(), _t(p_off), _t(tri).cuda(), _t(t_off).cuda())
  c_d2, c_idx = MM.point_triangle_distances(_t(pts), _t(p_off), _t(tri), _t(t_off))
  assert g_d2.is_cuda and g_idx.is_cuda and g_d2.dtype == t.float32 and g_idx.dtype == t.int32
  assert t.equal(g_idx.cpu(), c_idx)
  assert t.equal(g_d2.cpu().view(t.int32), c_d2.view(t.int32))
  return g_d2.cpu().numpy(), g_idx.cpu().numpy()


def _regions():
  pts = np.array([q for q, _ in TC.REGIONS], np.float32)
  return pts, TC.offsets([len(pts)]), TC.ONE, TC.offsets([1])


@pytest.mark.parametrize("kind", ["regions", "eligibility", "ties", "slivers", "accuracy", "sizes"])
def test_gpu_equals_twin_bit_for_bit(MM, kind):
  if kind == "regions":
    d2, idx = _both(MM, *_regions())
    want = np.array([d for _, d in TC.REGIONS], np.float64)
    assert (idx == 0).all() and (np.abs(d2 - want) <= 1e-6 * want).all() and (d2[want == 0] == 0).all()
  elif kind == "eligibility":
    case = TC.eligibility_case()
    d2, idx = _both(MM, *case[:4])
    assert idx.tolist() == case[4].tolist() and np.array_equal(d2, case[5])
  elif kind == "ties":
    pts, p_off, tri, t_off = TC.ties_case()
    d2, idx = _both(MM, pts, p_off, tri, t_off)
    assert (idx[:p_off[1]] == 0).all() and (idx[p_off[1]:] >= 0).all() and (idx[p_off[1]:] < 200).all()
  elif kind == "slivers":
    case = TC.sliver_case()
    TC.check_slivers(*_both(MM, *case[:4]), case, TC.TOL_SLIVER)
  elif kind == "accuracy":
    case = TC.accuracy_case()
    TC.check_accuracy(*_both(MM, *case[:4]), case, TC.TOL)
  else:
    QT, TT = MM.point_triangle_tiles()
    pts, p_off, tri, t_off = TC.sizes_case(QT, TT)
    nq, nt = np.diff(p_off), np.diff(t_off)
    assert {0, 1, QT + 1} <= set(nq.tolist()) and {0, 1, 3, TT + 1} <= set(nt.tolist())
    d2, idx = _both(MM, pts, p_off, tri, t_off)
    for n in range(len(nq)):
      q = slice(p_off[n], p_off[n + 1])
      assert ((idx[q] == -1) & np.isinf(d2[q])).all() if nt[n] == 0 else ((idx[q] >= 0) & (idx[q] < nt[n])).all()


def test_split_triangles_is_exact_and_deterministic(MM):
  """1 object x 100 queries x 40000 triangles: one query tile cannot fill the chip, so the triangles are cut into shares
  of whole tiles that merge through the 64-bit atomicMin.  The second half of the soup repeats the first, so every
  minimum has a tie in another share; some triangles are not eligible and one query is NaN."""
  rng = np.random.RandomState(31)
  half = TC.well_shaped(rng, 20000)
  half[::97] = TC.bad_triangles()[rng.randint(0, 4, len(half[::97]))]
  tri = np.concatenate([half, half])
  pts = rng.rand(100, 3).astype(np.float32)
  pts[41, 0] = np.nan
  p_off, t_off = TC.offsets([100]), TC.offsets([40000])
  splits = MM.point_triangle_splits(1, 100, 40000)
  TT = MM.point_triangle_tiles()[1]
  assert splits == (40000 + TT - 1) // TT > 1                                             # the split launch, a tile a share
  d2, idx = _both(MM, pts, p_off, tri, t_off)
  args = (_t(pts).cuda(), _t(p_off), _t(tri).cuda(), _t(t_off))
  first, second = MM.point_triangle_distances(*args), MM.point_triangle_distances(*args)
  assert t.equal(first[0].view(t.int32), second[0].view(t.int32)) and t.equal(first[1], second[1])
  keep = np.arange(100) != 41
  assert idx[41] == -1 and np.isinf(d2[41])
  assert (idx[keep] >= 0).all() and (idx[keep] < 20000).all()                             # ties across shares: the lower index
  assert TC.eligible(tri)[idx[keep]].all()
  o = TC.closest_distances(pts[keep][:20], half[TC.eligible(half)])
  assert (np.abs(np.sqrt(d2[keep][:20].astype(np.float64)) - o.min(1)) <= TC.TOL).all()


def test_one_workgroup_walks_several_tiles_without_split(MM):
  """1024 objects x 1 query x 257 / 600 triangles: objects x query tiles fill the chip, so nothing is split and one
  workgroup of the plain kernel walks 2 or 3 tiles, the last one partial (restaging LDS behind the barrier, the index
  base advancing, the NaN tail of a later tile).  The second half of every 600-triangle object repeats the first, so
  its minimum has a tie in a later tile."""
  QT, TT = MM.point_triangle_tiles()
  pts, p_off, tri, t_off = TC.many_tiles_case("plain", TT)
  nt = np.diff(t_off)
  assert len(nt) == 1024 and set(nt.tolist()) == {TT + 1, 600} and 600 > 2 * TT
  assert MM.point_triangle_splits(1024, 1, int(nt.max())) == 1                              # the plain launch
  d2, idx = _both(MM, pts, p_off, tri, t_off)
  assert (idx >= 0).all() and (idx < np.where(nt == 600, 300, nt)).all()                    # never the copy
  assert (idx >= TT).any()                                                                  # winners beyond the first tile
  for n in (0, 1, 1023):
    o = TC.closest_distances(pts[n:n + 1], tri[t_off[n]:t_off[n + 1]])
    assert abs(math.sqrt(float(d2[n])) - o.min()) <= TC.TOL and o[0, idx[n]] <= o.min() + TC.TOL


def test_split_shares_of_several_tiles(MM):
  """8 objects x 100 queries x (2 * 128 * tile + 1) triangles: 128 shares are wanted and there are 257 tiles, so a
  share holds 3 tiles (the last one 2, one of them a single record) and the shares behind it are empty.  A block of
  the soup is repeated 40000 places later, in another share; one query is NaN."""
  QT, TT = MM.point_triangle_tiles()
  pts, p_off, tri, t_off = TC.many_tiles_case("split", TT)
  nt = 2 * 128 * TT + 1
  assert np.diff(t_off).tolist() == [nt] * 8 and np.diff(p_off).tolist() == [100] * 8
  splits, tiles = MM.point_triangle_splits(8, 100, nt), (nt + TT - 1) // TT
  assert 1 < splits < tiles and -(-tiles // splits) == 3                                    # several tiles a share
  d2, idx = _both(MM, pts, p_off, tri, t_off)
  args = (_t(pts).cuda(), _t(p_off), _t(tri).cuda(), _t(t_off))
  again = MM.point_triangle_distances(*args)
  assert np.array_equal(again[0].cpu().numpy().view(np.int32), d2.view(np.int32)) and np.array_equal(again[1].cpu().numpy(), idx)
  assert idx[5] == -1 and np.isinf(d2[5]) and (np.delete(idx, 5) >= 0).all()
  assert not ((idx >= 40000) & (idx < 50000)).any()                                         # the copy never wins a tie
  assert (idx >= 3 * TT).any() and (idx % (3 * TT) >= TT).any()                             # later shares, later tiles
  for q in (0, 799):
    n = q // 100
    o = TC.closest_distances(pts[q:q + 1], tri[t_off[n]:t_off[n + 1]])
    assert abs(math.sqrt(float(d2[q])) - o.min()) <= TC.TOL and o[0, idx[q]] <= o.min() + TC.TOL


def _same_metrics(g, c):
  """Counts equal; float64 fields equal where the padded reduction gives the same bits, else within 1e-12 relative
  (the samples and d2 are identical: only the order of float64 sums inside torch's reduction may differ)."""
  assert type(g) is type(c)
  for name in g._fields:
    x, y = getattr(g, name).cpu(), getattr(c, name)
    assert x.dtype == y.dtype and x.shape == y.shape, name
    if x.dtype == t.int64:
      assert t.equal(x, y), name
      continue
    assert t.equal(t.isnan(x), t.isnan(y)) and t.equal(t.isinf(x), t.isinf(y)), name
    fin = t.isfinite(y)
    assert bool(((x[fin] - y[fin]).abs() <= 1e-12 * y[fin].abs()).all()), name


def test_mesh_chamfer_fscore_gpu_against_cpu(MM):
  rng = np.random.RandomState(32)
  a, b = TC.well_shaped(rng, 700), TC.well_shaped(rng, 500)
  bad, none = TC.bad_triangles(), np.zeros((0, 3, 3), np.float32)
  sq2, sq8 = TC.square(2, 0.0, 1), TC.square(2, 0.0, 2)
  # objects: two soups, one square in two tessellations, pred empty, gt not eligible, both empty
  pred = np.concatenate([a, sq2, none, b[:40], bad]).astype(np.float32)
  gt = np.concatenate([b, sq8, a[:30], bad, none]).astype(np.float32)
  p_off, g_off = TC.offsets([700, 2, 0, 40, 4]), TC.offsets([500, 8, 30, 4, 0])
  kw = dict(thresholds=TC.TAUS, num_samples=1500, seed=9)
  c = MM.mesh_chamfer_fscore(_t(pred), _t(p_off), _t(gt), _t(g_off), **kw)
  g = MM.mesh_chamfer_fscore(_t(pred).cuda(), _t(p_off), _t(gt).cuda(), _t(g_off).cuda(), **kw)
  assert g.accuracy.is_cuda and g.normal_consistency.is_cuda
  _same_metrics(g, c)
  assert float(g.chamfer_l1[1]) <= 1e-6 and float(g.normal_consistency[1]) == 1.0 and g.fscore[1].tolist() == [1, 1, 1]
  assert g.num_pred.tolist() == [1500, 1500, 0, 1500, 0] and g.num_gt.tolist() == [1500, 1500, 1500, 0, 0]
  assert bool(t.isinf(g.chamfer_l1[2:4]).all()) and bool(t.isnan(g.chamfer_l1[4]))
  assert g.normal_consistency[2:4].tolist() == [0, 0] and bool(t.isnan(g.normal_consistency[4]))
  again = MM.mesh_chamfer_fscore(_t(pred).cuda(), _t(p_off), _t(gt).cuda(), _t(g_off).cuda(), **kw)
  for x, y in zip(g, again):
    assert t.equal(t.isnan(x), t.isnan(y)) and t.equal(x[~t.isnan(x)], y[~t.isnan(y)])    # two runs: bit for bit


def test_surface_metrics_for_batch_triangles_gpu_against_cpu(MM):
  from corenet_amd import evaluation_results as ER
  pmf, ex = TC.fixture_batch_cpu()
  kw = dict(num_samples=1024, thresholds=TC.TAUS, seed=2, distance="triangles")
  for gt_source in ("mesh", "grid"):
    ex_c = ex
    if gt_source == "grid":                                # labels for the grid source: the argmax of the pmf, shifted
      import dataclasses
      lab = t.where(pmf.max(1)[0] > 0.5, pmf.argmax(1), t.zeros(pmf.shape[:1] + pmf.shape[2:], dtype=t.int64))
      ex_c = dataclasses.replace(ex, grid=lab.roll(1, dims=3).to(t.int32))
    c = ER.surface_metrics_for_batch(pmf, ex_c, "semantic", gt_source=gt_source, **kw)
    g = ER.surface_metrics_for_batch(pmf.cuda(), ex_c.cuda(), "semantic", gt_source=gt_source, **kw)
    assert g.metrics.accuracy.is_cuda and type(g.metrics) is MM.MeshSurfaceMetrics
    assert g.scene_id == c.scene_id and g.class_index.tolist() == c.class_index.tolist()
    _same_metrics(g.metrics, c.metrics)
    assert bool(t.isfinite(c.metrics.chamfer_l1).any())
