"""Voxel connected components on the GPU (csrc/voxel_components.hip) against the library's host twin:
exact equality of labels, counts and every stats field.  Shapes are expressed in the kernel's brick extents, so they
stay the smallest that reach each path: inside one brick, exactly one brick, a seam with a one-voxel-thick far side along
each axis, 2 x 2 x 2 bricks plus one voxel, the word boundaries of the run arithmetic along W, and one grid with more
chunks than one round of the root-count scan takes."""
import numpy as np
import pytest
import torch as t

import voxel_components_check as VC

pytestmark = pytest.mark.gpu

CONNECTIVITIES = (6, 18, 26)


@pytest.fixture(scope="module")
def M():
  from corenet_amd import voxel_components as M
  return M


@pytest.fixture(scope="module")
def bricks(M):
  return M.component_bricks()


def _full(bricks):
  bd, bh, bw = bricks
  return (2 * bd + 1, 2 * bh + 1, 2 * bw + 1)


def _multi_brick_shapes(bricks):
  bd, bh, bw = bricks
  return [(bd + 1, bh, bw), (bd, bh + 1, bw), (bd, bh, bw + 1), _full(bricks)]


def _equal(M, grid, connectivity=6, by_value=True):
  """GPU == twin on grid (a CPU tensor [N, D, H, W], any strides): labels, counts, stats.  Returns the twin's result."""
  want = M.connected_components(grid, connectivity, by_value)
  got = M.connected_components(grid.cuda(), connectivity, by_value)
  assert got.labels.is_cuda and got.labels.dtype == t.int32 and got.labels.is_contiguous() and got.num_components.dtype == t.int64
  assert t.equal(got.num_components.cpu(), want.num_components), (connectivity, by_value)
  assert t.equal(got.labels.cpu(), want.labels), (connectivity, by_value)
  sw, sg = M.component_stats(want, grid), M.component_stats(got, grid.cuda())
  assert t.equal(sg.offsets, sw.offsets) and not sg.offsets.is_cuda
  for name in ("size", "bbox", "first", "value"):
    a, b = getattr(sg, name), getattr(sw, name)
    assert a.is_cuda and a.dtype == b.dtype and t.equal(a.cpu(), b), (name, connectivity, by_value)
  assert M.component_stats(got).value is None and t.equal(M.component_stats(got).size, sg.size)
  return want


def _random_batch(shape, seed, dtype=np.int32):
  rng = np.random.default_rng(seed)
  return t.from_numpy(np.stack([VC.random_grid(rng, shape, density, classes, dtype) for density in (0.2, 0.5, 0.8)
                                for classes in (1, 3)]))


def test_twin_agrees_with_the_oracle_on_a_seam(M, bricks):
  """Anchors the comparisons below: on a grid small enough for the flood fill that still has a seam along W, the twin
  (and so the GPU) gives the oracle's labels."""
  bd, bh, bw = bricks
  g = VC.random_grid(np.random.default_rng(1), (3, 4, bw + 1), 0.6, 2)
  for c in CONNECTIVITIES:
    want, K, _ = VC.oracle_label(g, c, True)
    twin = _equal(M, t.from_numpy(g)[None], c)
    assert np.array_equal(twin.labels[0].numpy(), want) and int(twin.num_components[0]) == K


@pytest.mark.parametrize("which", ["inside", "one_brick"])
def test_single_brick(M, bricks, which):
  shape = (3, 5, 7) if which == "inside" else bricks
  grids = _random_batch(shape, 2)
  for c in CONNECTIVITIES:
    for bv in (True, False):
      _equal(M, grids, c, bv)


@pytest.mark.parametrize("index", range(4))
def test_random_multi_brick(M, bricks, index):
  grids = _random_batch(_multi_brick_shapes(bricks)[index], 10 + index)
  for c in CONNECTIVITIES:
    for bv in (True, False):
      _equal(M, grids, c, bv)


@pytest.mark.parametrize("W", [1, 63, 64, 65, 129])
def test_word_boundaries_along_w(M, W):
  grids = _random_batch((3, 5, W), 20 + W)
  for c in CONNECTIVITIES:
    _equal(M, grids, c, True)
  runs = t.ones((1, 2, 3, W), dtype=t.uint8)                           # runs that end exactly at the row's end
  runs[0, :, :, W // 2] = 0
  _equal(M, runs, 6)


def test_serpentine(M, bricks):
  g = t.from_numpy(VC.serpentine(_full(bricks)))[None]
  for c in CONNECTIVITIES:
    twin = _equal(M, g, c)
    assert twin.num_components.tolist() == [1]


@pytest.mark.parametrize("axis", range(3))
def test_u_across_a_seam(M, bricks, axis):
  g = VC.u_across_seam(_full(bricks), axis, bricks)
  inside = [slice(None)] * 3
  inside[axis] = slice(0, bricks[axis])
  assert int(M.connected_components(t.from_numpy(np.ascontiguousarray(g[tuple(inside)]))[None]).num_components[0]) == 2
  for c in CONNECTIVITIES:
    twin = _equal(M, t.from_numpy(g)[None], c)
    assert twin.num_components.tolist() == [1]
  # the same with the arms' order exchanged: the grid's lowest index is now in the short arm
  flipped = np.ascontiguousarray(np.flip(g, [a for a in range(3) if a != axis][0]))
  assert _equal(M, t.from_numpy(flipped)[None], 6).num_components.tolist() == [1]


def test_contacts_across_a_brick_corner(M, bricks):
  bd, bh, bw = bricks
  g = t.zeros((1,) + _full(bricks), dtype=t.uint8)
  pairs = [((bd - 1, bh - 1, 5), (bd, bh, 5)), ((3, bh - 1, bw - 1), (3, bh, bw)), ((bd - 1, 3, bw - 1), (bd, 3, bw)),
           ((bd - 1, bh, 20), (bd, bh - 1, 20)),                                               # by an edge only
           ((bd - 1, bh - 1, bw - 1), (bd, bh, bw)), ((2 * bd - 1, 2 * bh, bw - 1), (2 * bd, 2 * bh - 1, bw))]   # by a corner only
  for a, b in pairs:
    g[(0,) + a] = g[(0,) + b] = 1
  assert [_equal(M, g, c).num_components.tolist() for c in CONNECTIVITIES] == [[12], [8], [6]]


def test_checkerboard_and_uniform_grids(M, bricks):
  shape = _full(bricks)
  board = t.from_numpy(VC.checkerboard(shape))[None]
  assert _equal(M, board, 6).num_components.tolist() == [int(board.sum())]
  assert _equal(M, board, 26).num_components.tolist() == [1]
  for c in CONNECTIVITIES:
    assert _equal(M, t.full((1,) + shape, 3, dtype=t.int32), c).num_components.tolist() == [1]
    assert _equal(M, t.zeros((1,) + shape, dtype=t.int32), c).num_components.tolist() == [0]


def test_more_chunks_than_one_scan_round(M, bricks):
  shape = (64, 128, 2 * bricks[2] + 1)                                  # 1033 chunks of 1024 voxels
  g = t.from_numpy(VC.random_grid(np.random.default_rng(4), shape, 0.3, 2, np.uint8))[None]
  assert int(_equal(M, g, 6).num_components[0]) > 1024


def test_grids_are_independent(M, bricks):
  shape = _full(bricks)
  rng = np.random.default_rng(6)
  grids = t.from_numpy(np.stack([VC.random_grid(rng, shape, 0.5, 3), np.zeros(shape, np.int32), VC.random_grid(rng, shape, 0.3, 1)]))
  twin = _equal(M, grids, 18)
  assert int(twin.num_components[1]) == 0 and int(twin.labels[2].max()) == int(twin.num_components[2])
  one = M.connected_components(grids[2:].cuda(), 18)
  assert t.equal(one.labels[0].cpu(), twin.labels[2])


def test_strided_view_and_dtypes(M, bricks):
  bd, bh, bw = bricks
  rng = np.random.default_rng(8)
  full = t.from_numpy(VC.random_grid(rng, (2, 2, bd + 1, bh + 1, bw + 1), 0.5, 3))
  view = full[:, 1]
  assert not view.is_contiguous()
  twin = _equal(M, view, 26)
  assert t.equal(twin.labels, M.connected_components(view.contiguous(), 26).labels)
  gview = full.cuda()[:, 1]                                             # the strides reach the kernel: no copy
  assert not gview.is_contiguous()
  got = M.connected_components(gview, 26)
  assert t.equal(got.labels.cpu(), twin.labels)
  assert all(t.equal(x.cpu(), y) for x, y in zip(M.component_stats(got, gview), M.component_stats(twin, view)))
  dense = view.contiguous()
  for dtype in (t.uint8, t.int32, t.float32, t.int64, t.bool):
    x = (dense > 0).to(dtype) if dtype in (t.float32, t.bool) else dense.to(dtype)
    _equal(M, x, 6)
  nan = dense.float()
  nan[dense == 2] = float("nan")
  nan[dense == 3] = -1.0
  _equal(M, nan, 18)


def test_two_calls_give_identical_tensors(M, bricks):
  g = _random_batch(_full(bricks), 9).cuda()
  a = M.connected_components(g, 26)
  sa = M.component_stats(a, g)
  b = M.connected_components(g, 26)
  sb = M.component_stats(b, g)
  assert t.equal(a.labels, b.labels) and t.equal(a.num_components, b.num_components)
  assert all(t.equal(x, y) for x, y in zip(sa, sb))


def test_filter_and_instance_meshes_gpu_against_cpu(M, bricks):
  from corenet_amd.visualization import instance_meshes
  bd, bh, bw = bricks
  g = t.zeros((2, bd + 3, bh + 3, bw + 3), dtype=t.int32)
  g[0, 2:bd + 2, 3:7, 5:bw + 2] = 1                                     # crosses the d and the w seam
  g[0, 1:4, bh - 2:bh + 2, 2:6] = 2                                     # crosses the h seam
  g[0, bd + 1, bh + 1, bw + 1] = 2                                      # a floater
  g[1, :, 1:3, bw - 1:bw + 2] = 3
  g[1, 0, 8, 8] = 1
  for kw in (dict(min_voxels=2), dict(keep_largest=1), dict(keep_largest=1, by_value=False, connectivity=26)):
    want, got = M.filter_components(g, **kw), M.filter_components(g.cuda(), **kw)
    assert got.is_cuda and got.dtype == g.dtype and t.equal(got.cpu(), want)
  assert int((M.filter_components(g, min_voxels=2) != g).sum()) == 2
  f = g.float() * 0.25
  assert t.equal(M.filter_components(f.cuda(), min_voxels=2).cpu(), M.filter_components(f, min_voxels=2))
  mats = t.eye(4).repeat(2, 1, 1)
  mats[1, :3, 3] = t.tensor([1.0, 2.0, 3.0])
  mc, tc = instance_meshes(g, matrices=mats)
  mg, tg = instance_meshes(g.cuda(), matrices=mats.cuda())
  assert tc.size.tolist() == [3 * 4 * 4, bd * 4 * (bw - 3), 1, (bd + 3) * 2 * 3, 1]
  for a, b in zip(tuple(mg) + tuple(tg), tuple(mc) + tuple(tc)):
    assert a.dtype == b.dtype and t.equal(a.cpu(), b)
  assert mg.vertices.is_cuda and not tg.grid_index.is_cuda
