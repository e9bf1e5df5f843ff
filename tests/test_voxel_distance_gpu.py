"""Exact Euclidean distance transform on the GPU (csrc/voxel_distance.hip) against the library's host
twin: d2 and index are equal exactly, in all three modes.  The twin itself is anchored to the brute-force oracle in
test_voxel_distance_cpu.py.  Shapes come from distance_tiles(), so they stay the smallest that reach each path: the word
seams of the row pass, lines around the register tile, one line beyond the LDS capacity along each axis, and both forms of
the index (packed into one word, compare and select)."""
import numpy as np
import pytest
import torch as t

import voxel_distance_check as VD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
  from corenet_amd import voxel_distance as M
  return M


def _equal(M, grid, msg="", modes=VD.MODES):
  """GPU == twin on grid (a CPU tensor [N, D, H, W], any strides), with and without the index."""
  dev = grid.cuda()
  for mode in modes:
    want = M.squared_distance_to(grid, mode, return_index=True)
    got = M.squared_distance_to(dev, mode, return_index=True)
    assert got.d2.is_cuda and got.d2.dtype == t.int32 and got.d2.is_contiguous() and got.index.dtype == t.int32
    assert t.equal(got.d2.cpu(), want.d2), (msg, mode)
    assert t.equal(got.index.cpu(), want.index), (msg, mode)
    only = M.squared_distance_to(dev, mode)
    assert only.index is None and t.equal(only.d2.cpu(), want.d2), (msg, mode)


def _batch(rng, shape, densities=(0.001, 0.03, 0.5, 0.97), dtype=np.uint8):
  return t.from_numpy(np.stack([VD.random_grid(rng, shape, d, dtype) for d in densities]))


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 9), (7, 1, 1), (3, 5, 7), (24, 40, 72)])
def test_shapes(M, shape):
  _equal(M, _batch(np.random.default_rng(sum(shape)), shape), shape)


@pytest.mark.parametrize("W", [63, 64, 65, 130])
def test_word_seams_of_the_row_pass(M, W):
  rng = np.random.default_rng(W)
  g = np.zeros((2, 3, W), np.uint8)
  g[0, 0, 0] = g[1, 1, W - 1] = 1                           # the carry crosses every word, upwards and downwards
  _equal(M, t.cat([_batch(rng, (2, 3, W)), t.from_numpy(g)[None]]), W)


@pytest.mark.parametrize("dtype", [np.uint8, np.int32, np.bool_, np.float32])
def test_dtypes(M, dtype):
  _equal(M, _batch(np.random.default_rng(3), (9, 11, 70), dtype=dtype), dtype)


def test_line_lengths_around_the_register_tile(M):
  R = M.distance_tiles()[0]
  rng = np.random.default_rng(5)
  for L in (R - 1, R, R + 1, 2 * R + 1):
    _equal(M, _batch(rng, (3, L, 67)), ("H", L))
    _equal(M, _batch(rng, (L, 3, 67)), ("D", L))


def test_lines_at_and_beyond_the_lds_capacity(M):
  cap = M.distance_tiles()[1]
  rng = np.random.default_rng(6)
  dens = (0.002, 0.3)
  _equal(M, _batch(rng, (1, cap, 3), dens), "H at the capacity")                   # the largest LDS tile
  _equal(M, _batch(rng, (cap, 1, 3), dens), "D at the capacity")
  _equal(M, _batch(rng, (1, cap + 1, 3), dens), "H beyond the capacity")           # read from global memory
  _equal(M, _batch(rng, (cap + 1, 1, 3), dens), "D beyond the capacity")
  _equal(M, _batch(rng, (cap + 1, 2, 70), (0.002,)), "D beyond, H within", modes=("foreground",))


def _packs(M, shape):
  """Per line pass (h, d) of a grid [D, H, W]: whether the index is packed into one word (None: no such pass)."""
  _, cap, pack_bits = M.distance_tiles()
  D, H, W = shape
  out, bound = [], (W - 1) ** 2
  for L in (H, D):
    bound += (L - 1) ** 2
    out.append(None if L == 1 or L > cap else ((bound + 1) << int(np.ceil(np.log2(L)))) <= (1 << pack_bits))
  return out


def test_packed_and_unpacked_index(M):
  """The same content through both forms of the index: a wide grid leaves no room for the row in the packed word."""
  rng = np.random.default_rng(7)
  narrow, wide = (5, 6, 70), (5, 6, 23200)
  assert _packs(M, narrow) == [True, True] and _packs(M, wide) == [False, False]
  _equal(M, _batch(rng, narrow, (0.01, 0.4)), "packed")
  g = np.zeros((2,) + wide, np.uint8)
  g[0, 2, 3, 5] = g[0, 4, 0, 23199] = g[0, 0, 5, 11000] = 1                        # distances beyond 2^28: ties and far winners
  g[1] = VD.random_grid(rng, wide, 0.0005)
  _equal(M, t.from_numpy(g), "select")
  mixed = (500, 3, 2048)                                                           # the h pass packs, the longer d lines do not
  assert _packs(M, mixed) == [True, False]
  _equal(M, _batch(rng, mixed, (0.0005,)), "mixed", modes=("foreground",))


def test_single_target_empty_full_and_strided(M):
  shape = (12, 14, 70)
  g = np.zeros((4,) + shape, np.uint8)
  g[0, 0, 0, 0] = 1
  g[1, 11, 13, 69] = 1
  g[3] = 1                                                                          # grid 2 stays empty
  _equal(M, t.from_numpy(g), "corners")
  got = M.squared_distance_to(t.from_numpy(g).cuda(), "foreground", return_index=True)
  assert bool((got.d2[2] == VD.NO_TARGET).all()) and bool((got.index[2] == -1).all())
  assert bool(t.isinf(M.distance_to(t.from_numpy(g).cuda())[2]).all())
  x = t.from_numpy(np.stack([VD.random_grid(np.random.default_rng(8), (3, 5, 6, 70), d, np.int32) for d in (0.1, 0.4)]))
  view = x.cuda()[:, 1]
  assert not view.is_contiguous()
  want = M.squared_distance_to(x[:, 1], "surface", return_index=True)
  got = M.squared_distance_to(view, "surface", return_index=True)
  assert t.equal(got.d2.cpu(), want.d2) and t.equal(got.index.cpu(), want.index)
  empty = M.squared_distance_to(t.zeros((0, 3, 4, 5), dtype=t.uint8, device="cuda"), return_index=True)
  assert empty.d2.shape == (0, 3, 4, 5) and empty.index.is_cuda


def test_fixture_of_four_128_cubes(M):
  grids = t.from_numpy(VD.fixture_grids(4, 128, seed=1))
  assert 0 < float((grids > 0).float().mean()) < 0.02
  _equal(M, grids, "4 x 128^3", modes=("surface", "background"))


def test_derived_functions_and_surface_metrics_equal_the_cpu_results(M):
  rng = np.random.default_rng(9)
  shape = (14, 15, 66)
  a, b = VD.ball(shape, (6, 7, 30), 4.3), VD.ball(shape, (7, 7, 32), 4.3)
  pred = t.from_numpy(np.stack([a, a, rng.random(shape) < 0.1, np.zeros(shape, bool), a]).astype(np.uint8))
  gt = t.from_numpy(np.stack([a, b, rng.random(shape) < 0.1, np.zeros(shape, bool), np.zeros(shape, bool)]).astype(np.uint8))
  for f in (M.signed_distance, M.surface_voxels, lambda x: M.dilate(x, 2.5), lambda x: M.erode(x, 1.5), M.distance_to):
    assert t.equal(f(pred.cuda()).cpu(), f(pred))
  taus, vs = [0.0, 0.5, 1.25], t.tensor([0.5, 0.5, 1.0, 1.0, 2.0])
  want = M.voxel_surface_metrics(pred, gt, taus, voxel_size=vs)
  got = M.voxel_surface_metrics(pred.cuda(), gt.cuda(), taus, voxel_size=vs)
  for name in ("precision_count", "recall_count", "num_pred", "num_gt"):
    assert getattr(got, name).is_cuda and t.equal(getattr(got, name).cpu(), getattr(want, name)), name
  for name in ("accuracy", "completeness", "chamfer_l1", "chamfer_l2", "precision", "recall", "fscore"):
    x, y = getattr(got, name).cpu(), getattr(want, name)
    assert x.dtype == t.float64
    assert bool(((x == y) | (t.isnan(x) & t.isnan(y)) | ((x - y).abs() <= 1e-12 * y.abs())).all()), name


def test_non_default_stream(M):
  grids = _batch(np.random.default_rng(10), (20, 33, 70))
  want = M.squared_distance_to(grids, "surface", return_index=True)
  s = t.cuda.Stream()
  with t.cuda.stream(s):
    dev = grids.cuda()
    got = M.squared_distance_to(dev, "surface", return_index=True)
  s.synchronize()
  assert t.equal(got.d2.cpu(), want.d2) and t.equal(got.index.cpu(), want.index)
