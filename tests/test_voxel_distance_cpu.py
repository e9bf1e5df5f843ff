"""Exact Euclidean distance transform (corenet_amd.voxel_distance) on CPU tensors: the library's host
twin against the brute-force oracle of voxel_distance_check.py and against scipy, the wrapper's derived functions, the
voxel surface measure against chamfer_fscore on the surface voxels as points, and the evaluation integration."""
import dataclasses

import numpy as np
import pytest
import torch as t

import voxel_distance_check as VD

try:
  import scipy.ndimage as ndi
except ImportError:                                          # the oracle stands alone; scipy is a second opinion
  ndi = None

NT = VD.NO_TARGET


@pytest.fixture(scope="module")
def M():
  from corenet_amd import voxel_distance as M
  return M


def _check(M, grid, msg="", modes=VD.MODES, brute=VD.MODES):
  """Twin == oracle on one grid [D, H, W] (numpy) for every mode: d2 against the brute force over the target list, index
  against the recurrence, and the index points at a target at exactly d2; scipy where it is there.  brute: the modes
  whose target list is short enough for the brute force (voxels x targets pairs)."""
  tg = t.from_numpy(np.ascontiguousarray(grid))[None]
  for mode in modes:
    target = VD.targets_of(grid, mode)
    got = M.squared_distance_to(tg, mode, return_index=True)
    assert got.d2.dtype == t.int32 and got.d2.shape == tg.shape and got.d2.is_contiguous(), (msg, mode)
    assert got.index.dtype == t.int32 and got.index.shape == tg.shape and got.index.is_contiguous(), (msg, mode)
    d2, index = got.d2[0].numpy(), got.index[0].numpy()
    rd2, rindex = VD.recurrence(target)
    if mode in brute:
      assert np.array_equal(VD.brute_d2(target), rd2), (msg, mode)          # the recurrence attains the 3-D minimum
    assert np.array_equal(d2, rd2), (msg, mode)
    assert np.array_equal(index, rindex), (msg, mode)
    VD.check_index(target, d2, index)
    only = M.squared_distance_to(tg, mode)
    assert only.index is None and t.equal(only.d2, got.d2), (msg, mode)
    if ndi is not None and target.any():
      edt = ndi.distance_transform_edt(~target)
      assert np.array_equal(np.rint(edt * edt).astype(np.int64), d2), (msg, mode)


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 9), (7, 1, 1), (3, 5, 7), (24, 40, 72)])
def test_shapes(M, shape):
  rng = np.random.default_rng(sum(shape))
  big = shape[0] > 8                                         # there the background is 67 000 targets for 69 000 voxels
  _check(M, VD.random_grid(rng, shape, 0.03 if big else 0.3), shape, brute=("foreground", "surface") if big else VD.MODES)


@pytest.mark.parametrize("W", [63, 64, 65, 130])
def test_word_seams_of_the_row_pass(M, W):
  rng = np.random.default_rng(W)
  for density in (0.02, 0.5):
    _check(M, VD.random_grid(rng, (2, 3, W), density), (W, density))
  g = np.zeros((1, 2, W), np.uint8)
  g[0, 0, 0] = g[0, 1, W - 1] = 1                           # the carry crosses every word, upwards and downwards
  _check(M, g, (W, "ends"))


def test_line_lengths_around_the_register_tile_and_beyond_the_lds_capacity(M):
  R, cap, _ = M.distance_tiles()
  assert R >= 1 and cap >= R
  rng = np.random.default_rng(5)
  for L in (R - 1, R, R + 1):
    if L < 1:
      continue
    _check(M, VD.random_grid(rng, (3, L, 5), 0.1), ("H", L))
    _check(M, VD.random_grid(rng, (L, 3, 5), 0.1), ("D", L))
  _check(M, VD.random_grid(rng, (1, cap + 1, 3), 0.01), "H beyond the capacity")
  _check(M, VD.random_grid(rng, (cap + 1, 1, 3), 0.01), "D beyond the capacity")


@pytest.mark.parametrize("dtype", [np.uint8, np.int32, np.bool_, np.float32])
@pytest.mark.parametrize("density", [0.001, 0.03, 0.5, 0.97])
def test_densities_and_dtypes(M, density, dtype):
  rng = np.random.default_rng(int(density * 1000) + np.dtype(dtype).itemsize)
  grid = VD.random_grid(rng, (9, 11, 70), density, dtype)
  if np.issubdtype(dtype, np.floating):
    grid[0, 0, 0] = np.nan
  _check(M, grid, (density, dtype))


def test_single_target_in_a_corner(M):
  for corner in ((0, 0, 0), (11, 13, 69)):
    g = np.zeros((12, 14, 70), np.uint8)
    g[corner] = 1
    _check(M, g, corner, modes=("foreground", "surface"))


def test_batches_do_not_leak_and_empty_and_full_grids(M):
  rng = np.random.default_rng(11)
  shape = (6, 7, 66)
  grids = np.stack([VD.random_grid(rng, shape, 0.05), np.zeros(shape, np.uint8), VD.random_grid(rng, shape, 0.6)])
  for mode in ("foreground", "surface"):
    got = M.squared_distance_to(t.from_numpy(grids), mode, return_index=True)
    for n in range(3):
      rd2, rindex = VD.recurrence(VD.targets_of(grids[n], mode))
      assert np.array_equal(got.d2[n].numpy(), rd2) and np.array_equal(got.index[n].numpy(), rindex), (mode, n)
    assert bool((got.d2[1] == NT).all()) and bool((got.index[1] == -1).all())
    assert bool(t.isinf(M.distance_to(t.from_numpy(grids), mode)[1]).all())
  full = M.squared_distance_to(t.ones((2,) + shape, dtype=t.uint8), "foreground", return_index=True)
  assert bool((full.d2 == 0).all())
  assert t.equal(full.index, t.arange(int(np.prod(shape)), dtype=t.int32).reshape(shape).expand((2,) + shape))
  none = M.squared_distance_to(t.ones((1,) + shape, dtype=t.uint8), "background", return_index=True)
  assert bool((none.d2 == NT).all()) and bool((none.index == -1).all())
  empty = M.squared_distance_to(t.zeros((0, 3, 4, 5), dtype=t.uint8), return_index=True)
  assert empty.d2.shape == (0, 3, 4, 5) and empty.index.shape == (0, 3, 4, 5)


def test_strided_view_is_used_without_a_copy(M, monkeypatch):
  rng = np.random.default_rng(12)
  x = t.from_numpy(np.stack([VD.random_grid(rng, (3, 5, 6, 9), d, np.int32) for d in (0.1, 0.4)]))     # [N, K, D, H, W]
  view = x[:, 1]
  assert not view.is_contiguous() and view.stride(-1) == 1
  monkeypatch.setattr(t.Tensor, "contiguous", lambda self, *a, **k: pytest.fail("the view was copied"))
  got = M.squared_distance_to(view, "surface", return_index=True)
  monkeypatch.undo()
  want = M.squared_distance_to(view.contiguous(), "surface", return_index=True)
  assert t.equal(got.d2, want.d2) and t.equal(got.index, want.index)
  for n in range(2):
    assert np.array_equal(got.d2[n].numpy(), VD.brute_d2(VD.targets_of(view[n].numpy(), "surface")))
  wstrided = x[:, 1, :, :, ::2]                              # W stride 2: copied first
  assert t.equal(M.squared_distance_to(wstrided).d2, M.squared_distance_to(wstrided.contiguous()).d2)


def _ball_structure(radius):
  r = int(np.floor(radius))
  a = np.arange(-r, r + 1)
  d, h, w = np.meshgrid(a, a, a, indexing="ij")
  return d * d + h * h + w * w <= radius * radius


@pytest.mark.skipif(ndi is None, reason="needs scipy")
@pytest.mark.parametrize("radius", [1, 1.5, 2, 3.3])
def test_dilate_and_erode_against_scipy(M, radius):
  rng = np.random.default_rng(int(radius * 10))
  st = _ball_structure(radius)
  for density in (0.02, 0.9):
    mask = rng.random((13, 12, 15)) < density
    tm = t.from_numpy(mask)[None]
    assert np.array_equal(M.dilate(tm, radius)[0].numpy(), ndi.binary_dilation(mask, st)), (radius, density)
    assert np.array_equal(M.erode(tm, radius)[0].numpy(), ndi.binary_erosion(mask, st, border_value=1)), (radius, density)


def test_signed_distance_and_surface_voxels(M):
  occ = VD.ball((15, 16, 17), (7, 8, 8), 5.2)
  tm = t.from_numpy(occ)[None]
  sd = M.signed_distance(tm)[0].numpy()
  assert sd.dtype == np.float32
  inside = occ > 0
  assert (sd[inside] < 0).all() and (sd[~inside] > 0).all()
  want = np.where(inside, -np.sqrt(VD.brute_d2(~inside).astype(np.float64)), np.sqrt(VD.brute_d2(inside).astype(np.float64)))
  assert np.array_equal(sd, want.astype(np.float32))         # the square root of an exact integer, rounded once
  assert bool((M.signed_distance(t.zeros((1, 3, 3, 3))) == float("inf")).all())
  assert bool((M.signed_distance(t.ones((1, 3, 3, 3))) == float("-inf")).all())
  assert np.array_equal(M.surface_voxels(tm)[0].numpy(), VD.targets_of(occ, "surface"))
  assert int(M.surface_voxels(tm).sum()) < int(inside.sum())


def _as_points(grids):
  """The surface voxels of every grid as float32 points in raster order, with CSR offsets."""
  pts, off = [], [0]
  for g in grids:
    p = np.argwhere(VD.targets_of(g, "surface")).astype(np.float32)
    pts.append(p)
    off.append(off[-1] + len(p))
  return t.from_numpy(np.concatenate(pts).reshape(-1, 3)), t.tensor(off, dtype=t.int64)


def _close(a, b, rel=1e-12):
  a, b = a.to(t.float64), b.to(t.float64)
  same = (a == b) | (t.isnan(a) & t.isnan(b))                # equal infinities and NaNs
  return bool((same | ((a - b).abs() <= rel * b.abs())).all())


def test_voxel_surface_metrics_against_chamfer_fscore_on_the_surface_voxels(M):
  from corenet_amd import mesh_metrics as MM
  rng = np.random.default_rng(21)
  shape = (14, 15, 16)
  a, b = VD.ball(shape, (6, 7, 7), 4.3), VD.ball(shape, (7, 7, 9), 4.3)
  pred = np.stack([a, a, rng.random(shape) < 0.1, np.zeros(shape, bool), a]).astype(np.uint8)
  gt = np.stack([a, b, rng.random(shape) < 0.1, np.zeros(shape, bool), np.zeros(shape, bool)]).astype(np.uint8)
  taus = [0.0, 1.0, 2.5]
  got = M.voxel_surface_metrics(t.from_numpy(pred), t.from_numpy(gt), taus)
  want = MM.chamfer_fscore(*_as_points(pred), *_as_points(gt), taus)
  assert type(got) is MM.SurfaceMetrics
  for name in ("precision_count", "recall_count", "num_pred", "num_gt"):
    assert t.equal(getattr(got, name), getattr(want, name)), name
  for name in ("accuracy", "completeness", "chamfer_l1", "chamfer_l2", "precision", "recall", "fscore"):
    assert _close(getattr(got, name), getattr(want, name)), name
  assert float(got.chamfer_l1[0]) == 0.0 and got.fscore[0].tolist() == [1.0, 1.0, 1.0]       # identical grids
  assert 0 < float(got.chamfer_l1[1]) < 3 and 0 < float(got.fscore[1, 1]) < 1
  assert bool(t.isnan(got.chamfer_l1[3])) and bool(t.isnan(got.fscore[3]).all())              # empty on both sides
  assert float(got.chamfer_l1[4]) == float("inf") and got.fscore[4].tolist() == [0.0, 0.0, 0.0]
  # voxel_size scales distances and thresholds together
  scaled = M.voxel_surface_metrics(t.from_numpy(pred), t.from_numpy(gt), [x * 0.25 for x in taus], voxel_size=0.25)
  assert t.equal(scaled.precision_count, got.precision_count) and _close(scaled.chamfer_l1, got.chamfer_l1 * 0.25)
  per_grid = M.voxel_surface_metrics(t.from_numpy(pred), t.from_numpy(gt), taus, voxel_size=t.tensor([1, 2, 1, 1, 1.0]))
  assert _close(per_grid.chamfer_l1[1], got.chamfer_l1[1] * 2) and _close(per_grid.chamfer_l1[2], got.chamfer_l1[2])


def test_value_errors(M):
  with pytest.raises(ValueError):
    M.squared_distance_to(t.zeros((3, 4, 5), dtype=t.uint8))
  with pytest.raises(ValueError):
    M.squared_distance_to(t.zeros((2, 3, 0, 5), dtype=t.uint8))
  with pytest.raises(ValueError):
    M.squared_distance_to(t.zeros((1, 1, 1, 46342), dtype=t.uint8))
  assert M.squared_distance_to(t.zeros((1, 1, 1, 46341), dtype=t.uint8)).d2.shape == (1, 1, 1, 46341)
  with pytest.raises(ValueError):
    M.squared_distance_to(t.zeros((1, 2, 2, 2), dtype=t.uint8), target="edges")
  with pytest.raises(ValueError):
    M.voxel_surface_metrics(t.zeros((1, 2, 2, 2)), t.zeros((1, 2, 2, 3)), [1.0])
  # the library itself refuses what the wrapper refuses
  from corenet_amd import _lib as L
  import ctypes as C
  out = t.zeros(8, dtype=t.int32)
  g = t.zeros(8, dtype=t.uint8)
  st = (C.c_int64 * 4)(8, 8, 8, 1)
  for dims, mode in (((1, 1, 1, 46342), 0), ((1, 0, 1, 1), 0), ((1, 2, 2, 2), 3)):
    with pytest.raises(L.HipError):
      L.lib().crn_voxel_distance_cpu(g.data_ptr(), st, 1, *dims, mode, out.data_ptr(), None, 1)


@pytest.fixture(scope="module")
def fixture_batch():
  import point_triangle_check as TC
  pmf, ex = TC.fixture_batch_cpu()
  C = pmf.shape[1]
  grid = ((pmf[:, 1:] > 0.5).to(t.int32) * t.arange(1, C, dtype=t.int32)[None, :, None, None, None]).max(1)[0]
  onehot = t.nn.functional.one_hot(grid.long(), C).permute(0, 4, 1, 2, 3).float().contiguous()
  return onehot, dataclasses.replace(ex, grid=grid)


def test_voxel_surface_metrics_for_batch_and_results(fixture_batch):
  from corenet_amd import evaluation_results as ER
  from corenet_amd import mesh_metrics as MM
  onehot, ex = fixture_batch
  B, C = onehot.shape[:2]
  K = C - 1
  present = t.stack([(ex.grid[b] == k).any() for b in range(B) for k in range(1, C)])
  assert bool(present.any())
  rows = ER.voxel_surface_metrics_for_batch(onehot, ex, "semantic", thresholds=(0.0, 0.05))
  assert type(rows.metrics) is MM.SurfaceMetrics and rows.thresholds == (0.0, 0.05)
  assert rows.scene_index.tolist() == [b for b in range(B) for _ in range(K)]
  assert rows.class_index.tolist() == [k for _ in range(B) for k in range(1, C)]
  assert rows.scene_id == [ex.scene_id[b] for b in range(B) for _ in range(K)]
  cd, f = rows.metrics.chamfer_l1, rows.metrics.fscore
  assert bool((cd[present] == 0).all()) and bool((f[present] == 1).all())
  assert bool(t.isnan(cd[~present]).all()) and bool(t.isnan(f[~present]).all())
  # one class erased from the prediction: that row alone turns to +inf / 0
  row = int(present.nonzero()[0])
  erased = onehot.clone()
  erased[row // K, row % K + 1] = 0.0
  r2 = ER.voxel_surface_metrics_for_batch(erased, ex, "semantic", thresholds=(0.0, 0.05))
  assert float(r2.metrics.chamfer_l1[row]) == float("inf") and r2.metrics.fscore[row].tolist() == [0.0, 0.0]
  rest = t.arange(B * K) != row
  assert bool((r2.metrics.chamfer_l1[rest & present] == 0).all())
  # a one-voxel shift of a class is one voxel edge of accuracy at most, in view-space units
  R = onehot.shape[-1]
  shifted = t.roll(onehot, 1, dims=-1)
  r3 = ER.voxel_surface_metrics_for_batch(shifted, ex, "semantic", thresholds=(1.0 / R,))
  assert 0 < float(r3.metrics.accuracy[row]) <= 1.0 / R * (1 + 1e-6) and float(r3.metrics.fscore[row, 0]) == 1.0
  # the accumulator
  res = ER.VoxelSurfaceResults("semantic", thresholds=(0.0, 0.05))
  assert isinstance(res, ER.SurfaceResults)
  res.add_batch(onehot, ex)
  res.add_batch(erased, ex)
  cls, cds, fs = res.rows()
  assert cls.tolist() == rows.class_index.tolist() * 2 and cds.shape == (2 * B * K,) and fs.shape == (2 * B * K, 2)
  s = res.summary()
  assert s["thresholds"] == [0.0, 0.05] and s["overall"]["num_rows"] == 2 * int(present.sum())
  assert s["overall"]["chamfer_l1"] == float("inf") and 0 < s["overall"]["fscore"][0] < 1
  other = [k for k in s["per_class"] if k != row % K + 1 and s["per_class"][k]["num_rows"]]
  assert all(s["per_class"][k]["chamfer_l1"] == 0.0 and s["per_class"][k]["fscore"] == [1.0, 1.0] for k in other)
  # anisotropic voxels are refused
  bad = ex.v2x_transform.clone()
  bad[0, 0, 0] *= 1.01
  with pytest.raises(ValueError):
    ER.voxel_surface_metrics_for_batch(onehot, dataclasses.replace(ex, v2x_transform=bad), "semantic")
  with pytest.raises(ValueError):
    ER.voxel_surface_metrics_for_batch(onehot, ex, "fg_bg")                # fg_bg takes two classes
