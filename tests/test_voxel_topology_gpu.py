"""Voxel topology on the GPU (csrc/voxel_topology.hip) against the library's host twin: table and bad
are equal exactly.  The twin itself is anchored to numpy in test_voxel_topology_cpu.py.  Shapes come from
topology_tiles() and are the smallest that reach each seam: the brick of a workgroup on every axis, the corner where
eight bricks meet, the implicit border, the 16-byte loads with their element-wise heads and tails, the grids of a launch."""
import numpy as np
import pytest
import torch as t

import voxel_topology_check as TC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
  from corenet_amd import voxel_topology as M
  return M


def _on_device(x):
  """x on the device with the strides it has on the host."""
  return t.empty_strided(x.shape, x.stride(), dtype=x.dtype, device="cuda").copy_(x) if x.numel() else x.cuda()


def _equal_on(M, dev_grid, want, num_labels=None, msg=""):
  got = M.configuration_histogram(dev_grid, num_labels)
  assert got.table.is_cuda and got.bad.is_cuda and got.table.dtype == t.int64 and got.bad.dtype == t.int64
  assert t.equal(got.table.cpu(), want.table), (msg, "table")
  assert t.equal(got.bad.cpu(), want.bad), (msg, "bad")
  return want


def _equal(M, grid, num_labels=None, msg=""):
  """GPU == twin on the CPU tensor grid [N, D, H, W] (any strides: the device copy keeps them)."""
  grid = t.as_tensor(grid)
  return _equal_on(M, _on_device(grid), M.configuration_histogram(grid, num_labels), num_labels, msg)


def _brick(M, dtype):
  tiles = M.topology_tiles()
  return tiles.brick_d, tiles.brick_h_uint8 if dtype == np.uint8 else tiles.brick_h_int32, tiles.brick_w


@pytest.mark.parametrize("dtype", [np.int32, np.uint8])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_brick_seams(M, dtype, axis):
  """Cells and voxels of one axis: the owned extent - 1, the extent, + 1 (a grid of E voxels has E + 1 cells)."""
  rng = np.random.default_rng(axis)
  extent = _brick(M, dtype)[axis]
  for size in (extent - 2, extent - 1, extent, extent + 1):
    shape = [2, 3, 5, 6]
    shape[1 + axis] = size
    grid = TC.random_labels(rng, tuple(shape), 3, density=0.5, dtype=dtype)
    want = _equal(M, grid, 3, msg=size)
    assert int(want.table[0, 0].sum()) == (shape[1] + 1) * (shape[2] + 1) * (shape[3] + 1)
    _equal(M, grid > 0, msg=(size, "mask"))


@pytest.mark.parametrize("dtype", [np.int32, np.uint8])
def test_corner_of_eight_bricks(M, dtype):
  """One voxel whose eight cells belong to eight workgroups, alone and in a filled grid."""
  bd, bh, bw = _brick(M, dtype)
  grid = np.zeros((2, bd + 2, bh + 2, bw + 40), dtype=dtype)
  grid[0, bd - 1, bh - 1, bw - 1] = 2
  grid[1] = 1
  grid[1, bd - 1, bh - 1, bw - 1] = 2
  want = _equal(M, grid, 2)
  assert int(want.table[0, 0, 1:].sum()) == 8 and int(want.table[0, 2, 1:].sum()) == 8 and int(want.table[0, 1, 1:].sum()) == 0
  _equal(M, grid == 2)


@pytest.mark.parametrize("shape", [(5, 6, 7), (3, 4, 256), (1, 1, 1), (2, 2, 16)])
def test_grid_corners(M, shape):
  """The cells around the 8 corner voxels exist only through the implicit border."""
  D, H, W = shape
  for dtype in (np.int32, np.uint8):
    grid = np.zeros((1,) + shape, dtype=dtype)
    for d in (0, D - 1):
      for h in (0, H - 1):
        for w in (0, W - 1):
          grid[0, d, h, w] = 1
    _equal(M, grid, 1, msg=dtype)
    _equal(M, grid > 0, msg=(dtype, "mask"))


@pytest.mark.parametrize("W", [1, 3, 4, 5, 17])
def test_row_heads_and_tails(M, W):
  rng = np.random.default_rng(W)
  base = t.from_numpy(TC.random_labels(rng, (2, 5, 7, W + 4), 6, density=0.6))
  for b in (base, base.to(t.uint8)):
    _equal(M, b[..., :W].contiguous(), 6, msg="one row")
    dev = b.cuda()
    for start in (0, 1, 3):                                                  # rows of W voxels at every alignment
      sl = (Ellipsis, slice(start, start + W))
      _equal_on(M, dev[sl], M.configuration_histogram(b[sl], 6), 6, msg=(start, b.dtype))


def test_views(M):
  rng = np.random.default_rng(1)
  for dtype in (np.int32, np.uint8):
    a = t.from_numpy(TC.random_labels(rng, (3, 6, 9, 261), 5, density=0.5, dtype=dtype))
    dev = a.cuda()
    for sl in ((Ellipsis, slice(1, None)), (slice(None), slice(None, None, 2)), (slice(None), slice(None), slice(1, None, 3)),
               (slice(1, None),), (slice(None, None, 2),)):
      _equal_on(M, dev[sl], M.configuration_histogram(a[sl], 5), 5, msg=sl)
    _equal_on(M, dev[..., ::2], M.configuration_histogram(a[..., ::2], 5), 5, msg="W stride 2")
    _equal_on(M, dev[:1].expand(3, -1, -1, -1), M.configuration_histogram(a[:1].expand(3, -1, -1, -1), 5), 5, msg="N stride 0")


def test_dtypes(M):
  rng = np.random.default_rng(2)
  grid = t.from_numpy(TC.random_labels(rng, (2, 4, 33, 130), 4, density=0.5))
  want = _equal(M, grid, 4)
  for dtype in (t.uint8, t.int64):
    _equal_on(M, grid.cuda().to(dtype), want, 4, msg=dtype)
    _equal_on(M, grid.cuda().to(dtype), want, msg=(dtype, "maximum"))
  mask = M.configuration_histogram(grid > 0)
  assert t.equal(mask.table[:, 0], want.table[:, 0])
  for dtype in (t.bool, t.float32):
    _equal_on(M, (grid > 0).cuda().to(dtype), mask, msg=dtype)


def test_uniform_grids(M):
  """All background: nothing is counted; all one label: every interior cell takes the full-unit path."""
  for dtype in (t.int32, t.uint8):
    for value in (0, 3):
      want = _equal(M, t.full((2, 5, 40, 300), value, dtype=dtype), 3, msg=(dtype, value))
      assert int(want.table[0, 0, 255]) == (4 * 39 * 299 if value else 0)
      assert int(want.table[0, 3, 255]) == int(want.table[0, 0, 255])
  _equal(M, t.ones((1, 5, 40, 300), dtype=t.bool))


def test_label_checkerboard(M):
  """No two neighbours carry the same label: every cell is mixed and ends every run."""
  d, h, w = np.meshgrid(np.arange(6), np.arange(19), np.arange(70), indexing="ij")
  board = (1 + (d + h + w) % 2 + 2 * (h % 2))[None]
  for dtype in (np.int32, np.uint8):
    _equal(M, board.astype(dtype), 4, msg=dtype)
    _equal(M, np.where((d + w) % 3 == 0, 0, board).astype(dtype), 4, msg=(dtype, "holes"))


def test_label_counts(M):
  cap = M.topology_tiles().max_labels
  rng = np.random.default_rng(3)
  for L in (0, 1, cap):
    for dtype in (np.int32, np.uint8):
      grid = TC.random_labels(rng, (2, 7, 12, 70), L, density=0.8, dtype=dtype)
      grid[:, 0, 0, :L] = np.arange(1, L + 1)                                # every label is present
      want = _equal(M, grid, L, msg=(L, dtype))
      if L:
        assert bool((want.table[:, 1:, 1:].sum(-1) > 0).all())


def test_bad_labels(M):
  rng = np.random.default_rng(4)
  grid = TC.random_labels(rng, (3, 6, 11, 37), 4, density=0.6, bad=0.2)
  want = _equal(M, grid, 4)
  assert int(want.bad.min()) > 0
  _equal(M, TC.random_labels(rng, (3, 6, 11, 37), 4, density=0.6, bad=0.2, dtype=np.uint8), 4)
  want = _equal(M, np.full((2, 4, 5, 6), 9, np.int32), 4, msg="all out of range")
  assert want.bad.tolist() == [120, 120] and int(want.table[:, :, 1:].sum()) == 0
  _equal(M, np.full((2, 4, 5, 6), -1, np.int32), 0, msg="all negative")


def test_more_grids_than_a_launch(M):
  batch = M.topology_tiles().batch
  rng = np.random.default_rng(5)
  grid = TC.random_labels(rng, (batch + 2, 2, 2, 3), 2, density=0.6, bad=0.1)
  want = _equal(M, grid, 2)
  assert int(want.table[-1, 0, 1:].sum()) > 0


def test_stream_and_no_grids(M):
  rng = np.random.default_rng(6)
  grid = t.from_numpy(TC.random_labels(rng, (2, 9, 20, 70), 3, density=0.5))
  want = M.configuration_histogram(grid, 3)
  dev = grid.cuda()
  stream = t.cuda.Stream()
  stream.wait_stream(t.cuda.current_stream())
  with t.cuda.stream(stream):
    got = M.configuration_histogram(dev, 3)
  stream.synchronize()
  assert t.equal(got.table.cpu(), want.table) and t.equal(got.bad.cpu(), want.bad)
  got = M.configuration_histogram(t.zeros((0, 4, 5, 6), dtype=t.int32, device="cuda"), 2)
  assert got.table.is_cuda and tuple(got.table.shape) == (0, 3, 256) and tuple(got.bad.shape) == (0,)


def test_betti_numbers(M):
  for name in ("torus", "hollow_ball", "corner_pair", "ring"):
    mask = t.from_numpy(getattr(TC, name)())[None]
    for connectivity in (6, 26):
      want, got = M.betti_numbers(mask, connectivity), M.betti_numbers(mask.cuda(), connectivity)
      for x, y in zip(got, want):
        assert x.is_cuda and t.equal(x.cpu(), y), (name, connectivity)
  rng = np.random.default_rng(7)
  grid = t.from_numpy(TC.random_labels(rng, (1, 9, 10, 21), 2, density=0.6, bad=0.05))
  for connectivity in (6, 26):
    want = M.betti_numbers(grid, connectivity, num_labels=2)
    got = M.betti_numbers(grid.cuda(), connectivity, num_labels=2, _chunk_bytes=1)           # one mask per chunk: three chunks
    for x, y in zip(got, want):
      assert t.equal(x.cpu(), y), connectivity
