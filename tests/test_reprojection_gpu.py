"""Image-space reprojection metrics on the MI355X: the fixture scenes voxelized on the GPU, the rows of the geometry kernel
against those of the host twin (identical) and against the ray caster.  Batches and references:
render_geometry_check.py."""
import math

import pytest
import torch as t

import render_geometry_check as K

pytestmark = pytest.mark.gpu
_gpu = K.gpu_step
SIZE = (48, 64)


@pytest.fixture(scope="module")
def ER():
  from corenet_amd import evaluation_results as ER
  return ER


@pytest.fixture(scope="module")
def R():
  from corenet_amd.visualization import render as R
  return R


@pytest.fixture(scope="module")
def fixture():
  """(one-hot pmf of the ground truth, a pmf near it, the batch): the two fixture scenes voxelized at 32^3."""
  from corenet_amd import pipeline
  from corenet_amd.data import batched_example as B
  ex = _gpu(lambda: pipeline.voxelize_batch(B.batch(K.fixture_elements()), "semantic", resolution=(32, 32, 32)))
  noise = t.randn((2, 4, 32, 32, 32), generator=t.Generator().manual_seed(7)) * 0.8
  exact = K.one_hot_pmf(ex.grid, 4)
  return exact, (noise.cuda() + 2 * exact).softmax(1), ex


def test_prediction_equal_to_ground_truth_is_exact(ER, fixture):
  exact, _, ex = fixture
  rows = _gpu(lambda: ER.reprojection_metrics_for_batch(exact, ex, "semantic", image_size=SIZE))
  assert rows.silhouette.iou.device.type == "cuda"
  K.check_identity_rows(rows, 2)
  K.rows_equal(rows, ER.reprojection_metrics_for_batch(exact.cpu(), ex.cpu(), "semantic", image_size=SIZE))


def test_shifted_prediction_against_ray_caster(ER, R):
  rows = _gpu(lambda: K.check_shifted_example(ER, R, "cuda"))
  pmf, ex, _ = K.shifted_example()
  K.rows_equal(rows, ER.reprojection_metrics_for_batch(pmf, ex, "semantic"))


@pytest.mark.parametrize("gt", ["grid", "mesh"])
def test_rows_and_summary_equal_host(ER, fixture, gt):
  _, near, ex = fixture
  empty = t.zeros_like(near)
  empty[:, 0] = 1.0
  gpu, cpu = ER.ReprojectionResults("semantic", SIZE, gt=gt), ER.ReprojectionResults("semantic", SIZE, gt=gt)
  for pmf in (near, empty):
    rows = _gpu(lambda: gpu.add_batch(pmf, ex))
    K.rows_equal(rows, cpu.add_batch(pmf.cpu(), ex.cpu()))
  r = gpu.rows()
  assert bool((r["iou"][:2] > 0).all()) and bool((r["iou"][:2] < 1).all())     # near the truth, not equal to it
  assert bool((r["depth_count"][:2] > 50).all()) and bool(t.isfinite(r["depth_abs_sum"]).all())
  assert r["iou"][2:].tolist() == [0.0, 0.0] and r["depth_count"][2:].tolist() == [0, 0]
  g, c = gpu.summary(), cpu.summary()
  def same(a, b):
    if isinstance(a, dict):
      return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    return a == b or (math.isnan(a) and math.isnan(b))
  assert same(g, c), (g, c)
  assert g["depth"]["num_pixels"] == int(r["depth_count"].sum()) and 0 < g["depth"]["delta1"] <= 1
