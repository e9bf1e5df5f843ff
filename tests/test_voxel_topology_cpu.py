"""Voxel topology on the host (csrc/voxel_topology_cpu.cpp, corenet_amd/voxel_topology.py): the twin's
configuration histogram against shifted slices plus np.bincount, the derived quantities against direct counts of the two
cell complexes, Betti numbers against scipy.ndimage.label, shapes with known topology, the Crofton area of a digitised
ball, and every ValueError of the contract.  The GPU is compared with the twin in test_voxel_topology_gpu.py."""
import math

import numpy as np
import pytest
import torch as t

import voxel_topology_check as TC


@pytest.fixture(scope="module")
def M():
  from corenet_amd import voxel_topology as M
  return M


def _check(M, grid, num_labels=None, want_labels=None, mask_grid=False):
  """configuration_histogram(grid) == the reference, exactly; grid: CPU tensor or array [N, D, H, W]."""
  grid = t.as_tensor(grid)
  got = M.configuration_histogram(grid, num_labels)
  L = want_labels if want_labels is not None else num_labels
  table, bad = TC.table_of(grid.numpy(), L, mask_grid)
  assert got.table.dtype == t.int64 and got.bad.dtype == t.int64
  assert tuple(got.table.shape) == table.shape and np.array_equal(got.table.numpy(), table)
  assert np.array_equal(got.bad.numpy(), bad)
  N, D, H, W = grid.shape
  assert bool((got.table.sum(-1) == (D + 1) * (H + 1) * (W + 1)).all())
  return got


@pytest.mark.parametrize("density", [0.05, 0.3, 0.5, 0.8])
def test_random_masks(M, density):
  rng = np.random.default_rng(int(density * 100))
  grid = rng.random((3, 7, 9, 11)) < density
  got = _check(M, grid, mask_grid=True)
  for n in range(3):
    assert int(M.volume(got.table)[n, 0]) == TC.volume_of(grid[n])
    assert int(M.exposed_faces(got.table)[n, 0]) == TC.exposed_faces_of(grid[n])
    assert int(M.euler_characteristic(got.table, 26)[n, 0]) == TC.chi26_of(grid[n])
    assert int(M.euler_characteristic(got.table, 6)[n, 0]) == TC.chi6_of(grid[n])


def test_labelled_grids(M):
  cap = M.topology_tiles().max_labels
  assert cap >= 31                                                           # CRN_EVAL_MAX_CLASSES - 1
  rng = np.random.default_rng(1)
  for L in (1, 3, cap):
    grid = TC.random_labels(rng, (2, 7, 9, 11), L, density=0.7)
    grid[0, 0, 0, :3] = [L, 0, L]
    got = _check(M, grid, want_labels=L)                                     # num_labels=None: the call's maximum
    _check(M, grid, num_labels=L)
    masks = TC.masks_of(grid[1], L)[0]
    for row in range(L + 1):
      assert int(M.volume(got.table)[1, row]) == TC.volume_of(masks[row])
      assert int(M.exposed_faces(got.table)[1, row]) == TC.exposed_faces_of(masks[row])
      assert int(M.euler_characteristic(got.table, 26)[1, row]) == TC.chi26_of(masks[row])
      assert int(M.euler_characteristic(got.table, 6)[1, row]) == TC.chi6_of(masks[row])
  _check(M, np.zeros((1, 3, 3, 3), np.int32) - 2, want_labels=0)             # the maximum is clamped at 0: everything is bad


def test_bad_labels(M):
  rng = np.random.default_rng(2)
  grid = TC.random_labels(rng, (3, 7, 9, 11), 4, bad=0.2)
  assert (grid < 0).any() and (grid > 4).any()
  got = _check(M, grid, num_labels=4)
  assert int(got.bad.sum()) > 0
  _check(M, TC.random_labels(rng, (2, 5, 6, 7), 4, bad=0.2, dtype=np.uint8), num_labels=4)
  _check(M, grid, num_labels=0)                                              # every non-zero voxel is out of range


@pytest.mark.parametrize("shape", [(1, 9, 11), (7, 1, 11), (7, 9, 1), (1, 1, 1), (1, 1, 13)])
def test_flat_grids(M, shape):
  rng = np.random.default_rng(sum(shape))
  _check(M, TC.random_labels(rng, (2,) + shape, 3, density=0.6), num_labels=3)
  _check(M, rng.random((2,) + shape) < 0.5, mask_grid=True)


def test_strided_views(M):
  rng = np.random.default_rng(3)
  base = t.from_numpy(TC.random_labels(rng, (4, 8, 10, 23), 3, density=0.6))
  for sl in ((Ellipsis, slice(1, None)), (slice(None), slice(None, None, 2)), (slice(None), slice(None), slice(1, None, 3)),
             (slice(1, None, 2),), (Ellipsis, slice(None, None, 2))):
    view = base[sl]
    got = M.configuration_histogram(view, 3)
    want = M.configuration_histogram(view.contiguous(), 3)
    assert t.equal(got.table, want.table) and t.equal(got.bad, want.bad), sl
    _check(M, view, num_labels=3)
  _check(M, base[:1].expand(3, -1, -1, -1), num_labels=3)


def test_dtypes(M):
  rng = np.random.default_rng(4)
  grid = TC.random_labels(rng, (2, 6, 7, 19), 5, density=0.5)
  want = _check(M, grid, num_labels=5)
  for dtype in (t.uint8, t.int8, t.int16, t.int64):
    got = M.configuration_histogram(t.from_numpy(grid).to(dtype), 5)
    assert t.equal(got.table, want.table) and t.equal(got.bad, want.bad), dtype
  mask = grid > 0
  for dtype in (t.bool, t.float32, t.float64, t.float16):
    got = M.configuration_histogram(t.from_numpy(mask).to(dtype))
    assert tuple(got.table.shape) == (2, 1, 256) and t.equal(got.table[:, 0], want.table[:, 0]) and int(got.bad.sum()) == 0, dtype
  nan = t.full((1, 2, 2, 2), float("nan"))
  assert int(M.volume(M.configuration_histogram(nan).table)) == 0


def test_no_grids(M):
  got = M.configuration_histogram(t.zeros((0, 4, 5, 6), dtype=t.int32), 3)
  assert tuple(got.table.shape) == (0, 4, 256) and tuple(got.bad.shape) == (0,)
  got = M.configuration_histogram(t.zeros((0, 4, 5, 6), dtype=t.bool))
  assert tuple(got.table.shape) == (0, 1, 256)
  b = M.betti_numbers(t.zeros((0, 4, 5, 6), dtype=t.bool))
  assert all(tuple(x.shape) == (0, 1) for x in b)


def test_lookup_tables(M):
  luts = M.lookup_tables()
  assert set(luts) == {"popcount", "axis_mixed", "face_diag_mixed", "body_diag_mixed", "chi26_x8", "chi6_x8"}
  for v in luts.values():
    assert v.dtype == t.int64 and tuple(v.shape) == (256,)
  assert luts["popcount"][255] == 8 and luts["axis_mixed"][1] == 3 and luts["face_diag_mixed"][1] == 3 and luts["body_diag_mixed"][1] == 1
  assert luts["axis_mixed"].max() == 12 and luts["body_diag_mixed"].max() == 4     # the 3-D checkerboard code 0b10010110
  assert luts["axis_mixed"][0b10010110] == 12 and luts["face_diag_mixed"][0b10010110] == 0 and luts["body_diag_mixed"][0b10010110] == 4
  assert luts["chi26_x8"][255] == 0 and luts["chi6_x8"][255] == 0 and luts["chi26_x8"][1] == 1 and luts["chi6_x8"][1] == 1
  # voxel (i, j, k) is bit 4 i + 2 j + k, so bits 0 and 1 are a pair along W: 2 vertices - 1 edge of the centre complex;
  # 1 vertex, 4 edges, 5 faces, 2 cubes of the closed voxels at the cell's centre: 8 - 16 + 10 - 2
  assert luts["chi6_x8"][0b11] == 0 and luts["chi26_x8"][0b11] == 0
  assert luts["axis_mixed"][0b11] == 4 and luts["face_diag_mixed"][0b11] == 6 and luts["body_diag_mixed"][0b11] == 2


@pytest.mark.parametrize("connectivity", [6, 26])
def test_betti_against_scipy(M, connectivity):
  rng = np.random.default_rng(connectivity)
  for density in (0.05, 0.3, 0.5, 0.8):
    grid = rng.random((2, 7, 9, 11)) < density
    got = M.betti_numbers(t.from_numpy(grid), connectivity)
    for n in range(2):
      assert tuple(int(x[n, 0]) for x in got) == TC.betti_of(grid[n], connectivity), (density, n)
  L = 3
  grid = TC.random_labels(rng, (2, 6, 7, 8), L, density=0.6, bad=0.05)
  got = M.betti_numbers(t.from_numpy(grid), connectivity, num_labels=L, _chunk_bytes=1)      # one mask per chunk
  assert t.equal(got.b0, M.betti_numbers(t.from_numpy(grid), connectivity, num_labels=L).b0)
  for n in range(2):
    masks = TC.masks_of(grid[n], L)[0]
    for row in range(L + 1):
      assert tuple(int(x[n, row]) for x in got) == TC.betti_of(masks[row], connectivity), (n, row)


KNOWN = [  # shape, volume, exposed faces, chi, b under 6-connectivity, b under 26-connectivity
    ("torus", 1280, 1200, (0, 0), (1, 1, 0), (1, 1, 0)),
    ("hollow_ball", 3312, 2568, (2, 2), (1, 0, 1), (1, 0, 1)),
    ("corner_pair", 2, 12, (2, 1), (2, 0, 0), (1, 0, 0)),
    ("ring", 8, 32, (0, 0), (1, 1, 0), (1, 1, 0)),
]


@pytest.mark.parametrize("name,vol,faces,chi,b6,b26", KNOWN)
def test_known_shapes(M, name, vol, faces, chi, b6, b26):
  mask = getattr(TC, name)()
  table = M.configuration_histogram(t.from_numpy(mask)[None]).table
  assert int(M.volume(table)) == vol and int(M.exposed_faces(table)) == faces
  assert (int(M.euler_characteristic(table, 6)), int(M.euler_characteristic(table, 26))) == chi
  for connectivity, want in ((6, b6), (26, b26)):
    got = M.betti_numbers(t.from_numpy(mask)[None], connectivity)
    assert tuple(int(x) for x in got[:3]) == want
    assert int(got.chi) == want[0] - want[1] + want[2]


def test_full_and_empty(M):
  for fill, want in ((True, (1, 0, 0)), (False, (0, 0, 0))):
    mask = t.full((1, 4, 5, 6), fill)
    for connectivity in (6, 26):
      assert tuple(int(x) for x in M.betti_numbers(mask, connectivity)[:3]) == want
    table = M.configuration_histogram(mask).table
    assert int(M.volume(table)) == (120 if fill else 0) and int(M.exposed_faces(table)) == (2 * (20 + 24 + 30) if fill else 0)


@pytest.mark.parametrize("shift", [0.0, 0.37])
def test_crofton_area_of_a_ball(M, shift):
  """Measured with numpy: 0.9982 (centred) and 1.0062 (shifted) of 4 pi r^2; the 2 % margin covers the digitisation."""
  r = 12.3
  mask = TC.ball(32, r, shift)
  table = M.configuration_histogram(t.from_numpy(mask)[None]).table
  area = float(M.crofton_area(table))
  print("crofton / sphere", area / (4 * math.pi * r * r))
  assert abs(area / (4 * math.pi * r * r) - 1) < 0.02
  want = TC.crofton_of(TC.table_of(mask[None], 0, True)[0][0, 0])
  assert abs(area - want) <= 1e-12 * want
  assert abs(float(M.crofton_area(table, 0.5)) - 0.25 * want) <= 1e-12 * want
  assert M.crofton_area(table).dtype == t.float64


def test_errors(M):
  cap = M.topology_tiles().max_labels
  z = t.zeros((1, 2, 2, 2), dtype=t.int32)
  with pytest.raises(ValueError, match="rank-4"):
    M.configuration_histogram(t.zeros((2, 2, 2), dtype=t.int32))
  with pytest.raises(ValueError, match="rank-4"):
    M.betti_numbers(t.zeros((2, 2, 2), dtype=t.bool))
  with pytest.raises(ValueError, match="num_labels"):
    M.configuration_histogram(z.float(), num_labels=2)
  with pytest.raises(ValueError, match="num_labels"):
    M.configuration_histogram(z, num_labels=-1)
  with pytest.raises(ValueError, match=str(cap)):
    M.configuration_histogram(z, num_labels=cap + 1)
  with pytest.raises(ValueError, match=str(cap)):
    M.configuration_histogram(z + cap + 1)                                   # num_labels=None: the maximum is over the cap
  with pytest.raises(ValueError, match="connectivity"):
    M.euler_characteristic(t.zeros(256, dtype=t.int64), 18)
  with pytest.raises(ValueError, match="connectivity"):
    M.betti_numbers(z, 18)
  with pytest.raises(ValueError, match="empty"):
    M.configuration_histogram(t.zeros((1, 0, 2, 2), dtype=t.int32))
  with pytest.raises(ValueError, match="too large"):
    M.configuration_histogram(t.zeros((1, 1, 1, 1), dtype=t.uint8).expand(1, 2048, 1024, 1024))
  with pytest.raises(ValueError, match="256"):
    M.volume(t.zeros(255, dtype=t.int64))
