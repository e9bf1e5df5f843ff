"""Voxel connected components (corenet_amd.voxel_components) on CPU tensors: the library's host twin
against the flood-fill oracle of voxel_components_check.py, the wrapper's behaviour, and the two integrations."""
import dataclasses

import numpy as np
import pytest
import torch as t

import voxel_components_check as VC

CONNECTIVITIES = (6, 18, 26)


@pytest.fixture(scope="module")
def M():
  from corenet_amd import voxel_components as M
  return M


def _check(M, grid, msg=""):
  """Twin == oracle on one grid [D, H, W] (numpy): labels, count and stats, for every connectivity and by_value."""
  tg = t.from_numpy(np.ascontiguousarray(grid))[None]
  out = {}
  for c in CONNECTIVITIES:
    for bv in (True, False):
      want, K, stats = VC.oracle_label(grid, c, bv)
      comps = M.connected_components(tg, c, bv)
      assert comps.labels.dtype == t.int32 and comps.labels.shape == tg.shape and comps.labels.is_contiguous()
      assert comps.num_components.dtype == t.int64 and comps.num_components.tolist() == [K], (msg, c, bv)
      assert np.array_equal(comps.labels[0].numpy(), want), (msg, c, bv)
      s = M.component_stats(comps, tg)
      assert s.offsets.tolist() == [0, K]
      assert s.size.dtype == t.int64 and s.bbox.dtype == t.int32 and s.first.dtype == t.int64 and s.value.dtype == t.int32
      assert np.array_equal(s.size.numpy(), stats["size"]) and np.array_equal(s.bbox.numpy(), stats["bbox"]), (msg, c, bv)
      assert np.array_equal(s.first.numpy(), stats["first"]), (msg, c, bv)
      first_value = VC.foreground_keys(grid, True).reshape(-1)[stats["first"]] if K else np.zeros(0)
      assert np.array_equal(s.value.numpy(), first_value), (msg, c, bv)
      assert M.component_stats(comps).value is None
      out[c, bv] = K
  return out


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 9), (7, 1, 1), (3, 5, 7), (24, 24, 24)])
def test_random_grids(M, shape):
  rng = np.random.default_rng(sum(shape))
  for density in (0.2, 0.5, 0.8):
    for classes in (1, 3):
      _check(M, VC.random_grid(rng, shape, density, classes), (shape, density, classes))
      _check(M, VC.random_grid(rng, shape, density, classes, np.uint8), (shape, density, classes, "u8"))


def test_all_background_and_all_foreground(M):
  assert set(_check(M, np.zeros((3, 4, 5), np.int32)).values()) == {0}
  assert set(_check(M, np.full((3, 4, 5), 7, np.int32)).values()) == {1}


def test_checkerboard(M):
  g = VC.checkerboard((5, 6, 7))
  k = _check(M, g)
  assert k[6, True] == int(g.sum()) and k[26, True] == 1


@pytest.mark.parametrize("other,want", [((1, 1, 2), (1, 1, 1)), ((1, 2, 2), (2, 1, 1)), ((2, 2, 2), (2, 2, 1))])
def test_two_voxels_in_contact(M, other, want):
  g = np.zeros((4, 4, 4), np.uint8)
  g[1, 1, 1] = g[other] = 1
  k = _check(M, g)
  assert tuple(k[c, True] for c in CONNECTIVITIES) == want


def test_different_classes(M):
  g = np.zeros((2, 2, 3), np.int32)
  g[0, 0, 0], g[0, 0, 1] = 1, 2
  k = _check(M, g)
  assert k[6, True] == 2 and k[6, False] == 1


def test_float_grid_with_nan_and_negatives(M):
  g = np.array([[[0.5, np.nan, 2.0, -1.0, 3.0, 0.0, -np.inf, np.inf]]], np.float32)
  comps = M.connected_components(t.from_numpy(g)[None])
  assert comps.labels.reshape(-1).tolist() == [1, 0, 2, 0, 3, 0, 0, 4]
  _check(M, g)
  b = M.connected_components(t.from_numpy(g > 0)[None])
  assert t.equal(b.labels, comps.labels)
  i64 = M.connected_components(t.tensor([[[[5, 5, -5, 1 << 20, 1 << 20]]]], dtype=t.int64))
  assert i64.labels.reshape(-1).tolist() == [1, 1, 0, 2, 2]


def test_numbering_restarts_per_grid(M):
  rng = np.random.default_rng(3)
  grids = [VC.random_grid(rng, (4, 5, 6), 0.4, 2), np.zeros((4, 5, 6), np.int32), VC.random_grid(rng, (4, 5, 6), 0.6, 2)]
  tg = t.from_numpy(np.stack(grids))
  comps = M.connected_components(tg, 18)
  s = M.component_stats(comps, tg)
  off = [0]
  for n, g in enumerate(grids):
    want, K, stats = VC.oracle_label(g, 18, True)
    assert np.array_equal(comps.labels[n].numpy(), want) and int(comps.num_components[n]) == K
    sl = slice(off[-1], off[-1] + K)
    assert np.array_equal(s.size[sl].numpy(), stats["size"]) and np.array_equal(s.bbox[sl].numpy(), stats["bbox"])
    assert np.array_equal(s.first[sl].numpy(), stats["first"]) and np.array_equal(s.value[sl].numpy(), stats["value"])
    off.append(off[-1] + K)
  assert s.offsets.tolist() == off and int(comps.num_components[1]) == 0
  empty = M.connected_components(t.zeros((0, 4, 5, 6), dtype=t.int32))
  assert empty.labels.shape == (0, 4, 5, 6) and empty.num_components.shape == (0,)
  assert M.component_stats(empty).offsets.tolist() == [0]


def test_strided_view(M):
  rng = np.random.default_rng(5)
  full = t.from_numpy(VC.random_grid(rng, (3, 2, 5, 6, 7), 0.5, 3))
  view = full[:, 1]
  assert not view.is_contiguous()
  a, b = M.connected_components(view, 26), M.connected_components(view.contiguous(), 26)
  assert t.equal(a.labels, b.labels) and t.equal(a.num_components, b.num_components)
  sa, sb = M.component_stats(a, view), M.component_stats(b, view.contiguous())
  assert all(t.equal(x, y) for x, y in zip(sa, sb))
  wview = full[:, 0, :, :, ::2]                                          # W stride 2: copied first
  c = M.connected_components(wview)
  assert t.equal(c.labels, M.connected_components(wview.contiguous()).labels)


def test_matches_scipy_on_binary_inputs(M):
  ndimage = pytest.importorskip("scipy.ndimage")
  rng = np.random.default_rng(11)
  for shape in [(1, 1, 9), (3, 5, 7), (11, 11, 11)]:
    for density in (0.2, 0.5, 0.8):
      g = VC.random_grid(rng, shape, density, 1, np.uint8)
      for rank, c in ((1, 6), (2, 18), (3, 26)):
        want, K = ndimage.label(g, ndimage.generate_binary_structure(3, rank))
        comps = M.connected_components(t.from_numpy(g)[None], c)
        assert int(comps.num_components[0]) == K and np.array_equal(comps.labels[0].numpy(), want)


def test_filter_components(M):
  g = t.tensor([[[[1, 1, 0, 2, 2, 0, 2],
                  [0, 0, 0, 0, 0, 0, 0],
                  [3, 0, 3, 3, 0, 1, 0]]]], dtype=t.int32)
  assert M.filter_components(g, min_voxels=2).tolist() == [[[[1, 1, 0, 2, 2, 0, 0], [0, 0, 0, 0, 0, 0, 0], [0, 0, 3, 3, 0, 0, 0]]]]
  # per (grid, value): the largest of each class; the tie between the two 1-voxel ... sizes (2, 2, 1 | 1, 2, 1)
  assert M.filter_components(g, keep_largest=1).tolist() == [[[[1, 1, 0, 2, 2, 0, 0], [0, 0, 0, 0, 0, 0, 0], [0, 0, 3, 3, 0, 0, 0]]]]
  # per grid without by_value: components (1,1), (2,2), (2), (3), (3,3), (1): the tie of three 2-voxel ones goes to the first
  assert M.filter_components(g, keep_largest=1, by_value=False).tolist() == [[[[1, 1, 0, 0, 0, 0, 0], [0] * 7, [0] * 7]]]
  assert M.filter_components(g, keep_largest=2, by_value=False).tolist() == [[[[1, 1, 0, 2, 2, 0, 0], [0] * 7, [0] * 7]]]
  assert M.filter_components(g, min_voxels=2, keep_largest=5).tolist() == M.filter_components(g, min_voxels=2).tolist()
  assert t.equal(M.filter_components(g), g) and t.equal(M.filter_components(g, keep_largest=0), t.zeros_like(g))
  two = t.cat([g, g.flip(3)])                                            # counted per grid
  out = M.filter_components(two, keep_largest=1, by_value=False)
  assert t.equal(out[0], M.filter_components(g, keep_largest=1, by_value=False)[0])
  assert t.equal(out[1], M.filter_components(g.flip(3), keep_largest=1, by_value=False)[0])
  for dtype in (t.float32, t.bool, t.uint8, t.int64):
    x = (g > 0).to(dtype) if dtype in (t.bool, t.float32) else g.to(dtype)
    y = M.filter_components(x, min_voxels=2)
    assert y.dtype == dtype and y.shape == x.shape
    assert t.equal(y != 0, (x != 0) & (M.filter_components(x.to(t.int32), min_voxels=2) != 0))
  f = t.tensor([[[[0.7, 0.9, 0.0, 0.6]]]])
  assert t.equal(M.filter_components(f, min_voxels=2), t.tensor([[[[0.7, 0.9, 0.0, 0.0]]]]))     # values kept, not the mask


def test_errors(M):
  with pytest.raises(ValueError):
    M.connected_components(t.zeros((4, 5, 6), dtype=t.int32))
  with pytest.raises(ValueError):
    M.connected_components(t.zeros((1, 1, 4, 5, 6), dtype=t.int32))
  with pytest.raises(ValueError):
    M.connected_components(t.zeros((1, 4, 0, 6), dtype=t.int32))
  for c in (4, 8, 0, 27):
    with pytest.raises(ValueError):
      M.connected_components(t.zeros((1, 2, 2, 2), dtype=t.int32), connectivity=c)
    with pytest.raises(ValueError):
      M.filter_components(t.zeros((1, 2, 2, 2), dtype=t.int32), connectivity=c)
  big = t.zeros((1, 1, 1, 1), dtype=t.uint8).expand(1, 2048, 1024, 1024)                     # 2^31 voxels, no storage
  with pytest.raises(ValueError):
    M.connected_components(big)
  with pytest.raises(ValueError):
    M.connected_components(t.empty((2, 1 << 11, 1 << 10, 1 << 10), dtype=t.int32, device="meta"))
  with pytest.raises(ValueError):
    M.filter_components(big)


def test_bricks(M):
  bd, bh, bw = M.component_bricks()
  assert bd >= 1 and bh >= 1 and bw == 64                                                  # a wave owns a row of a brick


def test_instance_meshes_of_two_cubes():
  from corenet_amd.visualization import instance_meshes, marching_cubes
  g = t.zeros((2, 10, 10, 12), dtype=t.int32)
  g[0, 1:4, 1:4, 1:4] = 2
  g[0, 5:9, 5:8, 6:10] = 2                                               # more than one voxel from the first
  g[1, 2:4, 2:4, 2:4] = 1
  g[1, 7, 7, 7] = 3
  mats = t.eye(4).repeat(2, 1, 1)
  mats[1, :3, 3] = t.tensor([10.0, 20.0, 30.0])
  meshes, table = instance_meshes(g, matrices=mats)
  assert table.grid_index.tolist() == [0, 0, 1, 1] and table.value.tolist() == [2, 2, 1, 3]
  assert table.size.tolist() == [27, 48, 8, 1]
  assert table.bbox.tolist() == [[1, 1, 1, 4, 4, 4], [5, 5, 6, 9, 8, 10], [2, 2, 2, 4, 4, 4], [7, 7, 7, 8, 8, 8]]
  masks = t.stack([(g[0] == 2) & (t.arange(10)[:, None, None] < 4), (g[0] == 2) & (t.arange(10)[:, None, None] >= 4), g[1] == 1,
                   g[1] == 3]).float()
  want = marching_cubes(masks, matrices=mats[[0, 0, 1, 1]])
  assert all(t.equal(a, b) for a, b in zip(meshes, want))
  cls = marching_cubes((g[:1] == 2).float())
  assert int(meshes.num_faces[:2].sum()) == int(cls.num_faces[0]) > 0
  assert int(meshes.num_vertices[:2].sum()) == int(cls.num_vertices[0])
  big, tbig = instance_meshes(g, min_voxels=8)
  assert tbig.size.tolist() == [27, 48, 8] and big.num_faces.tolist() == meshes.num_faces[:3].tolist()
  none, tnone = instance_meshes(t.zeros((1, 4, 4, 4), dtype=t.int32))
  assert none.faces.shape == (0, 3) and none.num_faces.shape == (0,) and tnone.size.shape == (0,)


@pytest.fixture(scope="module")
def fixture_batch():
  import point_triangle_check as TC
  return TC.fixture_batch_cpu()


def _same(a, b):
  return a.dtype == b.dtype and t.equal(t.isnan(a), t.isnan(b)) and t.equal(a[~t.isnan(a)], b[~t.isnan(b)])


def test_min_component_voxels_zero_changes_nothing(fixture_batch):
  from corenet_amd import evaluation_results as ER
  pmf, ex = fixture_batch
  for kw in (dict(), dict(distance="triangles"), dict(gt_source="grid")):
    kw = dict(num_samples=512, thresholds=(0.02, 0.05), seed=1, **kw)
    a = ER.surface_metrics_for_batch(pmf, ex, "semantic", **kw)
    b = ER.surface_metrics_for_batch(pmf, ex, "semantic", min_component_voxels=0, **kw)
    assert type(a.metrics) is type(b.metrics) and a.scene_id == b.scene_id and a.thresholds == b.thresholds
    assert t.equal(a.scene_index, b.scene_index) and t.equal(a.class_index, b.class_index)
    for x, y in zip(a.metrics, b.metrics):
      assert _same(x, y)
  assert "min_component_voxels" not in ER.SurfaceResults("semantic").kwargs
  assert ER.SurfaceResults("semantic", min_component_voxels=3).kwargs["min_component_voxels"] == 3


def test_floater_removal_lowers_the_accuracy_side(fixture_batch):
  """The prediction is the ground-truth grid plus one voxel far from everything.  The floater's samples are the only
  ones off the ground-truth surface, so removing it must lower the accuracy side (prediction -> truth) strictly; it is
  never the nearest triangle of a ground-truth sample, so the completeness side stays as it is."""
  from corenet_amd import evaluation_results as ER
  from corenet_amd.voxel_components import connected_components, component_stats
  pmf, ex = fixture_batch
  C = pmf.shape[1]
  grid = (pmf[:, 1:] > 0.5).to(t.int32)
  grid = (grid * t.arange(1, C, dtype=t.int32)[None, :, None, None, None]).max(1)[0]
  assert int(component_stats(connected_components(grid)).size.min()) >= 2          # nothing else for the filter to take
  ex = dataclasses.replace(ex, grid=grid)
  onehot = t.nn.functional.one_hot(grid.long(), C).permute(0, 4, 1, 2, 3).float().contiguous()
  k = int(grid[0].max())                                                            # a class scene 0 has
  assert k >= 1 and bool((onehot[0, 1:, :4, :4, :4] == 0).all())
  planted = onehot.clone()
  planted[0, k, 1, 1, 1], planted[0, 0, 1, 1, 1] = 1.0, 0.0
  kw = dict(num_samples=2048, thresholds=(0.02, 0.05), seed=1, gt_source="grid", distance="triangles")
  base = ER.surface_metrics_for_batch(onehot, ex, "semantic", **kw).metrics
  with_floater = ER.surface_metrics_for_batch(planted, ex, "semantic", **kw).metrics
  removed = ER.surface_metrics_for_batch(planted, ex, "semantic", min_component_voxels=2, **kw).metrics
  row = k - 1
  print("accuracy with floater / removed / base:", float(with_floater.accuracy[row]), float(removed.accuracy[row]),
        float(base.accuracy[row]), "completeness:", float(with_floater.completeness[row]), float(removed.completeness[row]))
  for x, y in zip(removed, base):
    assert _same(x, y)                                                              # exactly the grid without the floater
  assert float(removed.accuracy[row]) < float(with_floater.accuracy[row])
  assert float(removed.completeness[row]) == float(with_floater.completeness[row])
  rest = [r for r in range(base.accuracy.numel()) if r != row]
  assert _same(with_floater.accuracy[rest], base.accuracy[rest])
