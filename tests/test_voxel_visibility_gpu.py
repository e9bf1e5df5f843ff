"""Voxel visibility on the GPU (csrc/voxel_visibility.hip) against the library's host twin: occluded
and first are equal exactly, with and without first, through the coarse form (brick bits in LDS) and the flat form (fine
words only).  The twin itself is anchored to the definition in test_voxel_visibility_cpu.py.  Shapes are the smallest
that reach each seam: the 64-voxel words of a row, the 4^3 bricks of the coarse map, more than one workgroup."""
import dataclasses
import math

import numpy as np
import pytest
import torch as t

import voxel_visibility_check as VC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
  from corenet_amd import voxel_visibility as M
  return M


def _equal(M, grid, eye, msg=""):
  """GPU == twin on grid (a CPU tensor [N, D, H, W], any strides) for the eye(s), in all four kernel forms."""
  dev = grid.cuda()
  want = M.occlusion(grid, eye, return_first=True)
  for flags in (0, M.FLAT):
    got = M.occlusion(dev, eye, return_first=True, flags=flags)
    assert got.occluded.is_cuda and got.occluded.dtype == t.bool and got.occluded.is_contiguous() and got.first.dtype == t.int32
    assert t.equal(got.occluded.cpu(), want.occluded), (msg, flags)
    assert t.equal(got.first.cpu(), want.first), (msg, flags)
    only = M.occlusion(dev, eye, flags=flags)
    assert only.first is None and t.equal(only.occluded.cpu(), want.occluded), (msg, flags)
  return want


def _batch(rng, shape, densities=(0.003, 0.05, 0.4), dtype=np.uint8):
  return t.from_numpy(np.stack([VC.random_grid(rng, shape, d, dtype) for d in densities]))


def _eyes(shape):
  """Eyes of every kind for a grid [D, H, W]: in front, on the centre lattice, inside, behind (z beyond D), the limits."""
  D, H, W = shape
  return {"front": [W / 2 + 0.3, H / 2 - 0.2, -0.87 * max(shape) - 0.11], "centre lattice": [W + 2.5, -1.5, -3.5],
          "inside": [W / 3 + 0.1, H / 2 + 0.25, D / 2 + 0.4], "behind": [W / 2 + 1.0, H / 2, D + 7.25],
          "limit +": [2048.0, 2048.0, 2048.0], "limit -": [-2048.0, -2048.0, -2048.0], "limit mixed": [2048.0, -2048.0, 2048.0]}


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 9), (7, 1, 1), (3, 5, 7), (24, 40, 72)])
def test_shapes(M, shape):
  grids = _batch(np.random.default_rng(sum(shape)), shape)
  for kind, eye in _eyes(shape).items():
    _equal(M, grids, eye, (shape, kind))


@pytest.mark.parametrize("W", [63, 64, 65, 130])
def test_word_seams(M, W):
  rng = np.random.default_rng(W)
  g = np.zeros((3, 5, W), np.uint8)
  g[1, 2, 0] = g[1, 2, 63 % W] = g[0, 4, W - 1] = g[2, 0, W // 2] = 1
  grids = t.cat([_batch(rng, (3, 5, W)), t.from_numpy(g)[None]])
  for eye in ([-20.5, 2.5, 1.5], [W + 30.0, 2.2, -4.0], [W / 2, 2.5, 40.0]):              # along the rows, both ways, and across
    _equal(M, grids, eye, (W, eye))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_brick_seams(M, axis):
  rng = np.random.default_rng(40 + axis)
  for extent in (3, 4, 5, 9):
    shape = [6, 6, 6]
    shape[axis] = extent
    grids = _batch(rng, tuple(shape), (0.02, 0.2))
    for kind in ("front", "inside", "behind", "centre lattice"):
      _equal(M, grids, _eyes(shape)[kind], (shape, kind))


def test_an_eye_per_grid(M):
  rng = np.random.default_rng(50)
  shape = (9, 10, 70)
  grids = _batch(rng, shape, (0.05,) * 4)
  eyes = t.tensor([_eyes(shape)[k] for k in ("front", "inside", "behind", "limit mixed")], dtype=t.float64)
  want = _equal(M, grids, eyes, "per grid")
  for n in range(4):
    assert t.equal(M.occlusion(grids[n:n + 1], eyes[n]).occluded[0], want.occluded[n])
  got = M.occlusion(grids.cuda(), eyes.cuda(), return_first=True)                         # a CUDA eye: copied to the host
  assert t.equal(got.first.cpu(), want.first)


def test_more_grids_than_one_launch_takes(M):
  """The eyes travel as kernel arguments, 64 grids per launch: 70 grids need two."""
  rng = np.random.default_rng(51)
  grids = _batch(rng, (3, 4, 9), (0.15,) * 70)
  eyes = t.from_numpy(rng.random((70, 3)) * 40 - 15)
  _equal(M, grids, eyes, "70 grids")


def test_sparse_fixture_with_the_documented_camera(M):
  from corenet_amd.geometry import transformations as T
  cam = T.perspective_rh(math.radians(60), 1, 1e-4, 10) @ T.look_at_rh([.5, .5, -.8666666], [.5, .5, .5], [0, -1, 0])
  eye = M.eye_in_voxel_space(cam, T.scale([64.0] * 3))
  assert bool((eye[0] - t.tensor([32.0, 32.0, -55.4667], dtype=t.float64)).abs().max() < 1e-3)
  grids = t.from_numpy(VC.fixture_grids(2, 64, seed=1))
  want = _equal(M, grids, eye[0], "2 x 64^3")
  assert 0 < int(want.occluded.sum()) < want.occluded.numel() // 4


def test_strided_view_no_grids_and_dtypes(M):
  rng = np.random.default_rng(52)
  x = t.from_numpy(np.stack([VC.random_grid(rng, (3, 5, 6, 70), d, np.int32) for d in (0.1, 0.4)]))
  view = x.cuda()[:, 1]
  assert not view.is_contiguous()
  eye = [80.0, 2.0, -9.5]
  want = M.occlusion(x[:, 1], eye, return_first=True)
  for flags in (0, M.FLAT):
    got = M.occlusion(view, eye, return_first=True, flags=flags)
    assert t.equal(got.occluded.cpu(), want.occluded) and t.equal(got.first.cpu(), want.first)
  none = M.occlusion(t.zeros((0, 3, 4, 5), dtype=t.uint8, device="cuda"), eye, return_first=True)
  assert none.occluded.shape == (0, 3, 4, 5) and none.first.is_cuda
  for dtype in (np.bool_, np.float32):
    _equal(M, _batch(rng, (5, 6, 70), (0.1,), dtype), eye, dtype)
  with pytest.raises(ValueError):
    M.occlusion(view, [float("nan"), 0.0, 0.0])
  with pytest.raises(ValueError):
    M.walk_steps(view, eye)


def test_non_default_stream(M):
  grids = _batch(np.random.default_rng(53), (20, 33, 70))
  eye = [35.0, 16.5, -30.25]
  want = M.occlusion(grids, eye, return_first=True)
  s = t.cuda.Stream()
  with t.cuda.stream(s):
    dev = grids.cuda()
    got = M.occlusion(dev, eye, return_first=True)
    flat = M.occlusion(dev, eye, flags=M.FLAT)
  s.synchronize()
  assert t.equal(got.occluded.cpu(), want.occluded) and t.equal(got.first.cpu(), want.first)
  assert t.equal(flat.occluded.cpu(), want.occluded)


def test_iou_and_batch_metrics_equal_the_cpu_results(M):
  import point_triangle_check as TC
  from corenet_amd import evaluation_results as ER
  rng = np.random.default_rng(54)
  shape = (10, 12, 66)
  pred, gt = _batch(rng, shape, (0.3, 0.05, 0.0)), _batch(rng, shape, (0.3, 0.05, 0.0))
  eye = [30.0, 6.0, -12.0]
  for occluder in (None, pred):
    want = M.visibility_iou(pred, gt, eye, occluder=occluder)
    got = M.visibility_iou(pred.cuda(), gt.cuda(), eye, occluder=None if occluder is None else occluder.cuda())
    for name in ("intersection", "union", "region_voxels"):
      assert getattr(got, name).is_cuda and t.equal(getattr(got, name).cpu(), getattr(want, name)), name
    x, y = got.iou.cpu(), want.iou
    assert x.dtype == t.float64 and bool(((x == y) | (t.isnan(x) & t.isnan(y))).all())       # bit for bit
  pmf, ex = TC.fixture_batch_cpu()
  C = pmf.shape[1]
  grid = ((pmf[:, 1:] > 0.5).to(t.int32) * t.arange(1, C, dtype=t.int32)[None, :, None, None, None]).max(1)[0]
  pmf = t.where(t.from_numpy(rng.random(tuple(pmf.shape)) < 0.1), 1.0 - pmf, pmf)
  ex = dataclasses.replace(ex, grid=grid)
  want = ER.visibility_metrics_for_batch(pmf, ex, "semantic")
  ex_dev = dataclasses.replace(ex, grid=grid.cuda(), camera_transform=ex.camera_transform.cuda(),
                               grid_sampling_offset=ex.grid_sampling_offset.cuda())
  got = ER.visibility_metrics_for_batch(pmf.cuda(), ex_dev, "semantic")
  assert t.equal(got.eye, want.eye) and got.scene_id == want.scene_id
  for name in ("intersection", "union", "region_voxels"):
    assert getattr(got.metrics, name).is_cuda and t.equal(getattr(got.metrics, name).cpu(), getattr(want.metrics, name)), name
  x, y = got.metrics.iou.cpu(), want.metrics.iou
  assert bool(((x == y) | (t.isnan(x) & t.isnan(y))).all())
