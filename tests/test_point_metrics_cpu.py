"""corenet_amd.mesh_metrics through the library's host twin (csrc/point_metrics_cpu.cpp) against plain numpy written
here and in point_metrics_check.py: nearest neighbours bit for bit, the sampler's properties, known answers of the
metric, the empty-set rules and the argument checks.  No GPU."""
import math

import numpy as np
import pytest
import torch as t

import point_metrics_check as PC


@pytest.fixture(scope="module")
def MM():
  from corenet_amd import mesh_metrics as MM
  return MM


def _t(x):
  return t.from_numpy(np.array(x))


@pytest.mark.parametrize("kind", ["sizes", "ties", "nan"])
def test_nearest_equals_numpy_bit_for_bit(MM, kind):
  a, a_off, b, b_off, d2, idx = PC.nearest_case(kind)
  got_d2, got_idx = MM.nearest_distances(_t(a), _t(a_off), _t(b), _t(b_off))
  assert got_d2.dtype == t.float32 and got_idx.dtype == t.int32
  assert np.array_equal(got_idx.numpy(), idx)
  assert np.array_equal(got_d2.numpy(), d2)              # equal, not close (+inf == +inf)
  if kind == "ties":                                     # the case does contain ties, and they went to the lower index
    h = PC.NEAREST_SIZES[5][1] // 2
    assert ((idx[a_off[5]:a_off[6]] < h) | (idx[a_off[5]:a_off[6]] >= 2 * h)).all()
  if kind == "nan":
    assert idx[0] == -1 and np.isinf(d2[0])              # its only candidate is NaN
    assert idx[a_off[4] + 5] == -1 and np.isinf(d2[a_off[4] + 5])     # a NaN query
    assert (idx[a_off[5]:a_off[6]] != 3).all() and (idx[a_off[5]:a_off[6]] != PC.NEAREST_SIZES[5][1] - 1).all()


def _barycentric(tri, p):
  """float64 barycentrics of p in the plane of tri [3, 3] (least squares) and the reproduced point."""
  A, B, C = tri.astype(np.float64)
  x, *_ = np.linalg.lstsq(np.stack([B - A, C - A], 1), p.astype(np.float64) - A, rcond=None)
  bary = np.array([1 - x[0] - x[1], x[0], x[1]])
  return bary, bary @ tri.astype(np.float64)


def test_samples_lie_in_their_triangles(MM):
  rng = np.random.RandomState(11)
  tri = (rng.rand(400, 3, 3) * 2 - 1).astype(np.float32)
  ext = np.linalg.norm(tri.max(1) - tri.min(1), axis=1)
  tri = tri[PC.areas64(tri) > 0.1 * ext ** 2][:64]       # well shaped: the least-squares barycentrics are well conditioned
  s = MM.sample_surface_points(_t(tri), [40, len(tri) - 40], num_samples=500, seed=3)
  assert s.points.shape == (2, 500, 3) and s.tri_index.shape == (2, 500) and s.valid.tolist() == [True, True]
  pts, ti = s.points.numpy(), s.tri_index.numpy()
  for n, (t0, cnt) in enumerate(((0, 40), (40, len(tri) - 40))):
    assert ti[n].min() >= 0 and ti[n].max() < cnt
    for i in range(500):
      tr = tri[t0 + ti[n, i]]
      extent = np.linalg.norm(tr.max(0) - tr.min(0))
      bary, back = _barycentric(tr, pts[n, i])
      # float32 rounding of three products and two sums: a few 1e-7 of the extent; 1e-5 as stated
      assert np.linalg.norm(back - pts[n, i]) <= 1e-5 * extent
      assert (bary >= -1e-5).all() and (bary <= 1 + 1e-5).all() and abs(bary.sum() - 1) < 1e-12


@pytest.mark.parametrize("S", [1000, 7])
def test_stratification_by_area(MM, S):
  """Every stratum of 1 / S of the total weight holds exactly one sample, so a triangle whose interval has length
  S a_k / A strata meets at most that many + 2 and at least that many - 2 of them (strictly); the spare half covers
  the quantisation of the weights (50 triangles x 2^-25 of the largest area x S: far below 0.5)."""
  tri = PC.decade_mesh(0)
  a = PC.areas64(tri)
  assert a.max() / a.min() > 900
  s = MM.sample_surface_points(_t(tri), [len(tri)], num_samples=S, seed=9)
  counts = np.bincount(s.tri_index.numpy()[0], minlength=len(tri))
  assert counts.sum() == S
  assert (np.abs(counts - S * a / a.sum()) < 2.5).all(), np.abs(counts - S * a / a.sum()).max()


def test_degenerate_triangles_get_no_sample_and_rows_do_not_depend_on_the_batch(MM):
  tri, counts = PC.sampling_soup()
  off = PC.offsets(counts)
  s = MM.sample_surface_points(_t(tri), counts, num_samples=777, seed=4)
  assert s.valid.tolist() == [True, True, False, False, True]
  ti = s.tri_index.numpy()
  assert not np.isin(ti[1], [20, 21, 52, 53]).any()      # the zero-area, NaN and infinite-area triangles of object 1
  assert (ti[2] == -1).all() and (ti[3] == -1).all()
  assert (s.points.numpy()[2:4] == 0).all() and np.isfinite(s.points.numpy()).all()
  # the same object alone, through offsets instead of counts: identical rows
  for n in (0, 1, 4):
    alone = MM.sample_surface_points(_t(tri[off[n]:off[n + 1]]), num_samples=777, seed=4, offsets=[0, counts[n]])
    assert t.equal(alone.points[0], s.points[n]) and t.equal(alone.tri_index[0], s.tri_index[n])
  # as object 3 of 5 in another call
  other = MM.sample_surface_points(_t(np.concatenate([tri[off[4]:], tri[:off[1]], tri[off[1]:off[2]], tri[off[4]:]])),
                                   [1, counts[0], 0, counts[1], 1], num_samples=777, seed=4)
  assert t.equal(other.points[3], s.points[1]) and t.equal(other.tri_index[3], s.tri_index[1])
  assert t.equal(other.points[1], s.points[0])
  # same seed: identical; another seed: different
  again = MM.sample_surface_points(_t(tri), counts, num_samples=777, seed=4)
  assert all(t.equal(x, y) for x, y in zip(again, s))
  diff = MM.sample_surface_points(_t(tri), counts, num_samples=777, seed=5)
  assert not t.equal(diff.points[0], s.points[0]) and not t.equal(diff.tri_index[1], s.tri_index[1])


def _square_gap2(S, p_fail=1e-12):
  """Bound on the squared in-plane gap between a point of a unit square and the nearest of S samples of the same square
  (two triangles), for the sampler as built.  Both triangles have the same area, hence the same integer weight, so each
  owns exactly S / 2 strata and receives exactly S / 2 samples; INSIDE a triangle the position comes from two hashed
  uniforms, i.e. the samples of a triangle are independent and uniform on it (the stratification is across triangles
  only, so no deterministic spacing exists).  A disc of radius r <= 1 around a point of the square covers at least
  pi r^2 / 4 of the square (the point in a corner); if it covers a1 and a2 of the two triangles (area 1 / 2 each) it is
  empty with probability (1 - 2 a1)^(S/2) (1 - 2 a2)^(S/2) <= exp(-S (a1 + a2)) <= exp(-S pi r^2 / 4).  Over the 2 S
  queries of both directions, some gap exceeds r with probability <= 2 S exp(-S pi r^2 / 4); r^2 below makes that
  p_fail (S = 4096: r^2 = 0.0114, r = 0.107)."""
  return 4.0 * math.log(2.0 * S / p_fail) / (math.pi * S)


def test_two_parallel_squares(MM):
  S, d = 4096, 0.25
  gap2 = _square_gap2(S)
  assert math.sqrt(d * d + gap2) < 1.5 * d
  p = MM.sample_surface_points(_t(PC.unit_square(0.0)), [2], num_samples=S, seed=1)
  g = MM.sample_surface_points(_t(PC.unit_square(d)), [2], num_samples=S, seed=2)
  assert np.bincount(p.tri_index.numpy()[0]).tolist() == [S // 2, S // 2]
  off = t.tensor([0, S])
  d2_pg, _ = MM.nearest_distances(p.points[0], off, g.points[0], off)
  d2_gp, _ = MM.nearest_distances(g.points[0], off, p.points[0], off)
  for d2 in (d2_pg, d2_gp):
    dist = d2.double().sqrt()
    assert float(dist.min()) >= d * (1 - 1e-6) and float(dist.max()) <= math.sqrt(d * d + gap2)
  m = MM.chamfer_fscore(p.points[0], off, g.points[0], off, [1.5 * d, 0.5 * d])
  # at or just above d: sqrt(d^2 + g^2) - d <= g^2 / (2 d), and the mean of g^2 is at most 4 / (pi S) even for a corner
  # point (a quarter disc); four times that as slack for the spread of the mean of 4096 gaps
  for v in (m.accuracy, m.completeness, m.chamfer_l1):
    assert d * (1 - 1e-6) <= float(v) <= d + 4 * (4 / (math.pi * S)) / (2 * d)
  assert d * d * (1 - 1e-6) <= float(m.chamfer_l2) <= d * d + gap2
  assert m.fscore.tolist() == [[1.0, 0.0]] and m.precision.tolist() == [[1.0, 0.0]] and m.recall.tolist() == [[1.0, 0.0]]
  assert m.precision_count.tolist() == [[S, 0]] and m.num_pred.tolist() == [S] and m.num_gt.tolist() == [S]


def test_surface_against_itself_and_empty_sets(MM):
  tri, counts = PC.sampling_soup()
  s = MM.sample_surface_points(_t(tri), counts, num_samples=256, seed=0)
  pts = s.points[t.tensor([0, 1, 4])].reshape(-1, 3)
  off = t.tensor([0, 256, 512, 768])
  m = MM.chamfer_fscore(pts, off, pts.clone(), off, [0.0, 0.1])
  assert (m.chamfer_l1 == 0).all() and (m.chamfer_l2 == 0).all() and (m.fscore == 1).all()
  # objects: both present, pred empty, gt empty, both empty
  p_off, g_off = t.tensor([0, 256, 256, 512, 512]), t.tensor([0, 256, 512, 512, 512])
  m = MM.chamfer_fscore(pts[:512], p_off, pts[:512], g_off, [0.1, 10.0])
  assert float(m.chamfer_l1[0]) == 0 and m.fscore[0].tolist() == [1, 1]
  for n in (1, 2):
    for f in (m.accuracy, m.completeness, m.chamfer_l1, m.chamfer_l2):
      assert float(f[n]) == float("inf")
    for f in (m.precision, m.recall, m.fscore):
      assert f[n].tolist() == [0, 0]
  for f in m[:7]:
    assert t.isnan(f[3]).all()
  assert m.num_pred.tolist() == [256, 0, 256, 0] and m.num_gt.tolist() == [256, 256, 0, 0]


def test_bad_arguments_raise_value_error(MM):
  tri = _t(PC.unit_square(0.0))
  pts = t.zeros(4, 3)
  off = t.tensor([0, 4])
  bad = [
      lambda: MM.sample_surface_points(tri.reshape(-1, 3), [2], 8),                 # rank
      lambda: MM.sample_surface_points(tri.double(), [2], 8),                       # dtype
      lambda: MM.sample_surface_points(tri, [2], 0),                                # num_samples < 1
      lambda: MM.sample_surface_points(tri, [3], 8),                                # counts do not cover the soup
      lambda: MM.sample_surface_points(tri, None, 8, offsets=[0, 2, 1, 2]),         # non-monotone
      lambda: MM.sample_surface_points(tri, [2], 8, offsets=[0, 2]),                # both
      lambda: MM.sample_surface_points(tri, t.tensor([2.0]), 8),                    # float counts
      lambda: MM.nearest_distances(pts.reshape(2, 6), off, pts, off),               # rank
      lambda: MM.nearest_distances(pts.double(), off, pts, off),                    # dtype
      lambda: MM.nearest_distances(pts, t.tensor([0, 3, 2, 4]), pts, t.tensor([0, 1, 2, 4])),   # non-monotone
      lambda: MM.nearest_distances(pts, t.tensor([0, 3]), pts, off),                # does not end at Na
      lambda: MM.nearest_distances(pts, off, pts, t.tensor([0, 2, 4])),             # object counts differ
      lambda: MM.nearest_distances(pts, off.float(), pts, off),                     # offsets dtype
      lambda: MM.chamfer_fscore(pts, off, pts, off, [-1.0]),
  ]
  for fn in bad:
    with pytest.raises(ValueError):
      fn()
