"""Voxel visibility on the host (csrc/voxel_visibility_cpu.cpp, corenet_amd.voxel_visibility): the
library's twin against the definition itself (voxel_visibility_check.brute, exact rationals over all pairs of voxels)
and against the integer walk in Python integers; the derived functions, the argument rules, the camera helper and the
evaluation hooks.  Everything is exact: no tolerance, no excluded case."""
import dataclasses
import math

import numpy as np
import pytest
import torch as t

import voxel_visibility_check as VC

DENSITIES = (0.05, 0.3, 0.7)


@pytest.fixture(scope="module")
def M():
  from corenet_amd import voxel_visibility as M
  return M


@pytest.fixture(scope="module")
def small_cases():
  """A dozen random grids of extents 1 .. 5 at three densities, each with an eye of every kind, and the definition's
  answer for each -- computed once and shared."""
  rng = np.random.default_rng(19)
  shapes = [(1, 1, 1), (1, 1, 5), (5, 1, 1), (1, 4, 1), (5, 5, 5)] + [tuple(int(v) for v in rng.integers(1, 6, size=3)) for _ in range(7)]
  cases = []
  for i, shape in enumerate(shapes):
    grid = VC.random_grid(rng, shape, DENSITIES[i % 3])
    for kind, eye in VC.eyes_for(shape, rng).items():
      cases.append((shape, kind, grid, eye, VC.brute(grid > 0, VC.quantise(eye))))
  return cases


def test_twin_equals_the_definition(M, small_cases):
  assert len({c[0] for c in small_cases}) >= 10 and len({c[1] for c in small_cases}) == 6
  for shape, kind, grid, eye, (occluded, first) in small_cases:
    got = M.occlusion(t.from_numpy(grid)[None], t.from_numpy(eye), return_first=True)
    assert got.occluded.dtype == t.bool and got.first.dtype == t.int32 and got.occluded.shape == (1,) + shape
    assert np.array_equal(got.occluded[0].numpy(), occluded), (shape, kind)
    assert np.array_equal(got.first[0].numpy(), first), (shape, kind)


def test_python_walk_equals_the_definition(small_cases):
  for shape, kind, grid, eye, (occluded, first) in small_cases:
    o, f = VC.dda(grid > 0, VC.quantise(eye))
    assert np.array_equal(o, occluded) and np.array_equal(f, first), (shape, kind)


def test_twin_equals_python_walk_at_the_range_limit(M):
  """Eyes at +-2^19 sub-units on all three axes: |delta| reaches 2^20 and the 64-bit terms are largest."""
  rng = np.random.default_rng(20)
  grid = VC.random_grid(rng, (3, 5, 70), 0.1)
  for sx in (-1, 1):
    for sy in (-1, 1):
      for sz in (-1, 1):
        eye = np.array([sx, sy, sz], np.float64) * (VC.MAX_EYE / VC.SUB)
        q = VC.quantise(eye)
        assert [abs(v) for v in q] == [VC.MAX_EYE] * 3
        o, f = VC.dda(grid > 0, q)
        got = M.occlusion(t.from_numpy(grid)[None], eye, return_first=True)
        assert np.array_equal(got.occluded[0].numpy(), o) and np.array_equal(got.first[0].numpy(), f), (sx, sy, sz)
        steps = M.walk_steps(t.from_numpy(grid)[None], eye)
        assert np.array_equal(steps[0].numpy(), VC.dda(grid > 0, q, count=True)[1])


def test_one_voxel_on_the_axis_casts_its_column(M):
  g = t.zeros((1, 1, 1, 9), dtype=t.uint8)
  g[0, 0, 0, 3] = 1
  got = M.occlusion(g, [-4.0, 0.5, 0.5], return_first=True)           # the eye on the row's axis, before voxel 0
  assert got.occluded[0, 0, 0].tolist() == [False] * 4 + [True] * 5
  assert got.first[0, 0, 0].tolist() == [-1] * 4 + [3] * 5
  got = M.occlusion(g, [12.0, 0.5, 0.5], return_first=True)           # from the other end
  assert got.occluded[0, 0, 0].tolist() == [True] * 3 + [False] * 6
  assert got.first[0, 0, 0].tolist() == [3] * 3 + [-1] * 6


def test_empty_grid_monotonicity_and_mask_without_first(M):
  rng = np.random.default_rng(21)
  shape = (6, 7, 9)
  eye = t.tensor([[4.3, -6.1, 20.7], [2.5, 3.5, 1.5]])
  empty = M.occlusion(t.zeros((2,) + shape, dtype=t.uint8), eye, return_first=True)
  assert not bool(empty.occluded.any()) and bool((empty.first == -1).all())
  a = t.from_numpy(np.stack([VC.random_grid(rng, shape, 0.1) for _ in range(2)]))
  b = t.maximum(a, t.from_numpy(np.stack([VC.random_grid(rng, shape, 0.1) for _ in range(2)])))
  oa, ob = M.occlusion(a, eye, return_first=True), M.occlusion(b, eye)
  assert bool(oa.occluded.any()) and ob.first is None
  assert bool((ob.occluded | ~oa.occluded).all())                     # adding occupancy never un-occludes
  assert t.equal(M.occlusion(a, eye).occluded, oa.occluded)           # return_first does not change the mask
  assert t.equal(oa.first >= 0, oa.occluded)
  assert t.equal(M.visible(a, eye), ~oa.occluded) and t.equal(M.visible_surface(a, eye), (a > 0) & ~oa.occluded)
  assert t.equal(M.occlusion(a, eye, flags=M.FLAT).occluded, oa.occluded)          # the twin takes the flag and ignores it
  # one eye for all grids == the same eye per grid
  assert t.equal(M.occlusion(a, eye[0]).occluded, M.occlusion(a, eye[:1].expand(2, 3)).occluded)


@pytest.mark.parametrize("dtype", [np.uint8, np.int32, np.bool_, np.float32, np.float64, np.int64])
def test_dtypes(M, dtype):
  rng = np.random.default_rng(22)
  g = np.stack([VC.random_grid(rng, (4, 5, 70), d, dtype) for d in (0.02, 0.3)])
  eye = [80.25, -3.0, 9.5]
  want = [VC.dda(VC.foreground_of(x), VC.quantise(eye)) for x in g]
  got = M.occlusion(t.from_numpy(g), eye, return_first=True)
  for n in range(2):
    assert np.array_equal(got.occluded[n].numpy(), want[n][0]) and np.array_equal(got.first[n].numpy(), want[n][1])


def test_strided_view_and_no_grids(M):
  rng = np.random.default_rng(23)
  x = t.from_numpy(np.stack([VC.random_grid(rng, (3, 4, 5, 66), d, np.int32) for d in (0.1, 0.4)]))
  view = x[:, 1]
  assert not view.is_contiguous()
  eye = t.tensor([[70.0, 2.0, -5.0], [-1.0, 9.0, 9.0]])
  got, want = M.occlusion(view, eye, return_first=True), M.occlusion(view.contiguous(), eye, return_first=True)
  assert t.equal(got.occluded, want.occluded) and t.equal(got.first, want.first)
  wide = t.from_numpy(VC.random_grid(rng, (1, 3, 4, 10), 0.3))[..., ::2]              # W stride 2: copied first
  assert t.equal(M.occlusion(wide, eye[0]).occluded, M.occlusion(wide.contiguous(), eye[0]).occluded)
  none = M.occlusion(t.zeros((0, 3, 4, 5)), t.zeros((0, 3)), return_first=True)
  assert none.occluded.shape == (0, 3, 4, 5) and none.occluded.dtype == t.bool and none.first.dtype == t.int32
  assert M.occlusion(t.zeros((0, 3, 4, 5)), [1.0, 2.0, 3.0]).first is None


def test_argument_errors(M):
  g = t.zeros((2, 3, 4, 5), dtype=t.uint8)
  eye = [1.0, 2.0, -3.0]
  for bad in (t.zeros((3, 4, 5)), t.zeros((1, 2, 3, 4, 5)), t.zeros((2, 0, 4, 5)), t.zeros((2, 3, 4, 0)),
              t.zeros((1, 1, 1, M.MAX_EXTENT + 1), dtype=t.uint8), t.zeros((1, M.MAX_EXTENT + 1, 1, 1), dtype=t.uint8)):
    with pytest.raises(ValueError):
      M.occlusion(bad, eye)
  for bad_eye in ([1.0, 2.0], [[1.0, 2.0, 3.0]] * 3, [[[1.0, 2.0, 3.0]]], [float("nan"), 0.0, 0.0], [0.0, float("inf"), 0.0],
                  [0.0, 0.0, 2048.01], [-2048.01, 0.0, 0.0], 1.0):
    with pytest.raises(ValueError):
      M.occlusion(g, bad_eye)
  M.occlusion(g, [2048.0, -2048.0, 2048.0])                           # the limit itself is inside
  with pytest.raises(ValueError):
    M.occlusion(g, eye, flags=2)
  with pytest.raises(ValueError):
    M.visibility_iou(g, g[:1], eye)
  with pytest.raises(ValueError):
    M.visibility_iou(g, g, eye, occluder=g[:, :2])
  # the library's own checks (the C ABI behind the Python ones)
  import ctypes as C
  from corenet_amd import _lib as L
  lib = L.lib()
  occ = t.empty(g.shape, dtype=t.bool)
  st = (C.c_int64 * 4)(*g.stride())

  def call(N, D, H, W, q, flags=0):
    q = t.tensor(q, dtype=t.int32)
    lib.crn_voxel_visibility_cpu(g.data_ptr(), st, 1, N, D, H, W, q.data_ptr(), flags, occ.data_ptr(), None, 1)
  call(2, 3, 4, 5, [[0, 0, 0], [1 << 19, -(1 << 19), 5]])
  for args in ((2, 3, 4, 5, [[0, 0, 0], [(1 << 19) + 1, 0, 0]]), (2, 3, 4, 5, [[0, -(1 << 19) - 1, 0], [0, 0, 0]]),
               (2, 0, 4, 5, [[0, 0, 0]] * 2), (1, 1, 1, 2049, [[0, 0, 0]]), (2, 3, 4, 5, [[0, 0, 0]] * 2, 8),
               (2, 3, 4, 5, [[0, 0, 0]] * 2, 2)):                      # counting steps needs `first`
    with pytest.raises(L.HipError):
      call(*args)


def test_eye_in_voxel_space(M):
  from corenet_amd.geometry import transformations as T
  cam = T.perspective_rh(math.radians(60), 1, 1e-4, 10) @ T.look_at_rh([.5, .5, -.8666666], [.5, .5, .5], [0, -1, 0])
  eye = M.eye_in_voxel_space(cam, T.scale([128.0] * 3))
  assert eye.dtype == t.float64 and eye.shape == (1, 3)
  # float32 matrices: the eye comes back through a float64 inverse of a float32 product
  assert bool((eye[0] - t.tensor([64.0, 64.0, -0.8666666 * 128], dtype=t.float64)).abs().max() < 1e-4)
  cam64 = (T.perspective_rh(math.radians(60), 1, 1e-4, 10).double() @
           t.tensor([[1, 0, 0, -.5], [0, -1, 0, .5], [0, 0, -1, -.8666666], [0, 0, 0, 1]], dtype=t.float64))    # look_at_rh in float64
  eye64 = M.eye_in_voxel_space(cam64, T.scale([128.0] * 3).double())
  assert bool((eye64[0] - t.tensor([64.0, 64.0, -0.8666666 * 128], dtype=t.float64)).abs().max() < 1e-9)
  both = M.eye_in_voxel_space(t.stack([cam64, cam64]), T.scale([64.0] * 3).double())
  assert both.shape == (2, 3) and bool((both - eye64 / 2).abs().max() < 1e-9)
  with pytest.raises(ValueError):
    M.eye_in_voxel_space(T.ortho_lh(-1, 1, -1, 1, 0.1, 10), T.scale([128.0] * 3))
  with pytest.raises(ValueError):
    M.eye_in_voxel_space(cam64, T.scale([128.0 * 32] * 3).double())     # 3550 voxels in front: beyond the range
  with pytest.raises(ValueError):
    M.eye_in_voxel_space(cam64[:3], T.scale([128.0] * 3))


def test_visibility_iou(M):
  rng = np.random.default_rng(24)
  shape = (6, 7, 8)
  pred = t.from_numpy(np.stack([VC.random_grid(rng, shape, d) for d in (0.3, 0.5, 0.0, 0.2)]))
  gt = t.from_numpy(np.stack([VC.random_grid(rng, shape, d) for d in (0.3, 0.4, 0.0, 0.0)]))
  eye = [3.5, 3.0, -9.0]
  r = M.visibility_iou(pred, gt, eye)
  p, g = (pred > 0).reshape(4, -1), (gt > 0).reshape(4, -1)
  for x in (r.intersection, r.union, r.region_voxels):
    assert x.dtype == t.int64 and x.shape == (4, 2)
  assert t.equal(r.intersection.sum(1), (p & g).sum(1)) and t.equal(r.union.sum(1), (p | g).sum(1))
  assert bool((r.region_voxels.sum(1) == 6 * 7 * 8).all())
  hidden = M.occlusion(gt, eye).occluded.reshape(4, -1)
  assert t.equal(r.region_voxels[:, 1], hidden.sum(1)) and t.equal(r.intersection[:, 1], (p & g & hidden).sum(1))
  assert r.iou.dtype == t.float64 and t.equal(t.isnan(r.iou), r.union == 0)
  assert bool(t.isnan(r.iou[2]).all()) and bool(t.isnan(r.iou[3, 1]))          # an empty gt hides nothing: no hidden region
  ok = r.union > 0
  assert t.equal(r.iou[ok], r.intersection[ok].double() / r.union[ok].double())
  other = M.visibility_iou(pred, gt, eye, occluder=pred)
  assert t.equal(other.region_voxels[:, 1], M.occlusion(pred, eye).occluded.reshape(4, -1).sum(1))
  # right in front, wrong behind: a wall facing the eye and, behind it, a block the prediction puts elsewhere
  gt1 = t.zeros((1, 8, 8, 8), dtype=t.uint8)
  gt1[0, 2] = 1                                                        # the wall z = 2, seen from z < 0
  gt1[0, 5, 1:4, 1:4] = 1
  pr1 = gt1.clone()
  pr1[0, 5] = 0
  pr1[0, 6, 4:7, 4:7] = 1
  one = M.visibility_iou(pr1, gt1, [4.0, 4.0, -30.0])
  assert one.iou[0].tolist() == [1.0, 0.0] and one.intersection[0].tolist() == [64, 0] and one.union[0].tolist() == [64, 18]


@pytest.fixture(scope="module")
def fixture_batch():
  import point_triangle_check as TC
  pmf, ex = TC.fixture_batch_cpu()
  C = pmf.shape[1]
  grid = ((pmf[:, 1:] > 0.5).to(t.int32) * t.arange(1, C, dtype=t.int32)[None, :, None, None, None]).max(1)[0]
  return pmf, dataclasses.replace(ex, grid=grid)


def test_visibility_metrics_for_batch_and_results(M, fixture_batch):
  from corenet_amd import evaluation_results as ER
  from corenet_amd.data.batched_example import view2voxel_matrices
  pmf, ex = fixture_batch
  B, C = pmf.shape[:2]
  K = C - 1
  rng = np.random.default_rng(25)
  pmf = t.where(t.from_numpy(rng.random(tuple(pmf.shape)) < 0.1), 1.0 - pmf, pmf)     # a prediction that is partly wrong
  rows = ER.visibility_metrics_for_batch(pmf, ex, "semantic")
  assert rows.scene_index.tolist() == [b for b in range(B) for _ in range(K)]
  assert rows.class_index.tolist() == [k for _ in range(B) for k in range(1, C)]
  assert rows.scene_id == [ex.scene_id[b] for b in range(B) for _ in range(K)]
  eye = M.eye_in_voxel_space(ex.camera_transform, view2voxel_matrices(ex.grid_sampling_offset, pmf.shape[2:]))
  assert t.equal(rows.eye, eye)
  scene = (ex.grid > 0)
  assert 0 < int(M.occlusion(scene, eye).occluded.sum()) < scene.numel()
  for b in range(B):
    for k in range(1, C):
      want = M.visibility_iou(pmf[b, k][None] > 0.5, (ex.grid[b] == k)[None], eye[b], occluder=scene[b][None])
      r = b * K + k - 1
      for name in ("intersection", "union", "region_voxels"):
        assert t.equal(getattr(rows.metrics, name)[r], getattr(want, name)[0]), (b, k, name)
      x, y = rows.metrics.iou[r], want.iou[0]
      assert bool(((x == y) | (t.isnan(x) & t.isnan(y))).all())
  assert bool((rows.metrics.union > 0).any(0).all())                   # both regions are measured somewhere
  res = ER.VisibilityResults("semantic")
  assert res.rows()[0].numel() == 0 and res.summary()["per_class"] == {}
  res.add_batch(pmf, ex)
  res.add_batch(pmf, ex)
  cls, inter, union, iou = res.rows()
  assert cls.tolist() == rows.class_index.tolist() * 2 and t.equal(inter[:B * K], rows.metrics.intersection)
  s = res.summary()
  assert sorted(s["per_class"]) == list(range(1, C)) and set(s["overall"]) == {"visible", "hidden"}
  for c, region in enumerate(("visible", "hidden")):
    col = rows.metrics.iou[:, c]
    keep = ~t.isnan(col)
    assert s["overall"][region]["num_rows"] == 2 * int(keep.sum())
    assert abs(s["overall"][region]["mean_iou"] - float(col[keep].mean())) < 1e-12
    pooled = float(rows.metrics.intersection[:, c].sum()) / float(rows.metrics.union[:, c].sum())
    assert abs(s["overall"][region]["pooled_iou"] - pooled) < 1e-12
  # argument errors as in voxel_surface_metrics_for_batch
  for bad in (lambda: ER.visibility_metrics_for_batch(pmf[0], ex, "semantic"),
              lambda: ER.visibility_metrics_for_batch(pmf[:1], ex, "semantic"),
              lambda: ER.visibility_metrics_for_batch(pmf, ex, "fg_bg"),
              lambda: ER.visibility_metrics_for_batch(pmf[..., :-1], ex, "semantic")):
    with pytest.raises(ValueError):
      bad()
