"""Image-space reprojection metrics on the host (corenet_amd.image_metrics, evaluation_results.reprojection_metrics_for_batch
and ReprojectionResults through the renderer's host twin).  Batches and references: render_geometry_check.py."""
import dataclasses
import math

import numpy as np
import pytest
import torch as t

import render_geometry_check as K


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
  ex = K.host_fixture_batch()
  return K.one_hot_pmf(ex.grid, 4), ex


def test_prediction_equal_to_ground_truth_is_exact(ER, fixture):
  pmf, ex = fixture
  rows = ER.reprojection_metrics_for_batch(pmf, ex, "semantic", image_size=(48, 64))
  K.check_identity_rows(rows, 2)
  assert rows.scene_id == ex.scene_id and rows.class_index.tolist() == [1, 2, 3, 1, 2, 3]
  small = ER.reprojection_metrics_for_batch(pmf, ex, "semantic")              # the input image's 24 x 32
  assert int(small.silhouette.union.sum()) < int(rows.silhouette.union.sum())
  # fg_bg: one class per scene, the silhouette under the scene's label
  one = dataclasses.replace(ex, mesh_labels=[t.tensor([3], dtype=t.int32), t.tensor([7], dtype=t.int32)],
                            grid=(ex.grid > 0).to(t.int32))
  fg = ER.reprojection_metrics_for_batch(K.one_hot_pmf(one.grid, 2), one, "fg_bg", image_size=(48, 64))
  K.check_identity_rows(fg, 2)
  assert fg.class_index.tolist() == [1, 1]
  assert t.equal(fg.class_union, fg.silhouette.union) and t.equal(fg.silhouette.union, rows.silhouette.union)


def test_shifted_prediction_against_ray_caster(ER, R):
  K.check_shifted_example(ER, R, "cpu")


def test_mesh_ground_truth_summary_and_empty_prediction(ER, fixture):
  pmf, ex = fixture
  res = ER.ReprojectionResults("semantic", image_size=(48, 64), gt="mesh")
  rows = res.add_batch(pmf, ex)
  s, d = rows.silhouette, rows.depth
  assert bool((s.intersection > 50).all()) and bool((s.intersection <= s.union).all())
  assert bool(((s.iou > 0.2) & (s.iou < 1)).all())                            # boxes around the meshes, not the meshes
  assert bool((d.count == s.intersection).all()) and bool((d.delta1_count <= d.count).all())
  for x in (d.abs_sum, d.sq_sum, d.abs_rel_sum):
    assert bool(t.isfinite(x).all()) and bool((x > 0).all())
  assert bool((d.abs_sum / d.count < 0.5).all())                              # the scene is about one unit deep
  present = rows.class_union > 0
  assert present.tolist() == [True, True, True, True, True, False]            # scene 1 has no mesh of class 3
  assert bool((rows.class_intersection[present] > 0).all())
  # an empty prediction: IoU 0, no pixel covered on both sides
  empty = t.zeros_like(pmf)
  empty[:, 0] = 1.0
  rows0 = res.add_batch(empty, ex)
  assert rows0.silhouette.intersection.tolist() == [0, 0] and rows0.silhouette.iou.tolist() == [0.0, 0.0]
  assert bool((rows0.silhouette.union > 0).all()) and bool((rows0.silhouette.union < s.union).all())
  assert rows0.depth.count.tolist() == [0, 0] and rows0.depth.abs_sum.tolist() == [0.0, 0.0]
  lone = ER.ReprojectionResults("semantic", image_size=(48, 64), gt="mesh")
  lone.add_batch(empty, ex)
  sm0 = lone.summary()
  assert sm0["silhouette"]["mean_iou"] == 0.0 and sm0["depth"]["num_pixels"] == 0
  assert all(math.isnan(sm0["depth"][k]) for k in ("mean_abs", "rmse", "abs_rel", "delta1"))
  # summary() pools as documented, over both batches
  r = res.rows()
  sm = res.summary()
  assert r["iou"].shape == (4,) and r["class_iou"].shape == (12,) and res.scene_id == ex.scene_id * 2
  assert sm["silhouette"]["num_rows"] == 4
  assert abs(sm["silhouette"]["mean_iou"] - float(r["iou"].mean())) < 1e-15
  assert abs(sm["silhouette"]["pooled_iou"] - int(r["intersection"].sum()) / int(r["union"].sum())) < 1e-15
  n = int(r["depth_count"].sum())
  assert sm["depth"]["num_pixels"] == n == int(d.count.sum())
  assert abs(sm["depth"]["mean_abs"] - float(r["depth_abs_sum"].sum()) / n) < 1e-15
  assert abs(sm["depth"]["rmse"] - math.sqrt(float(r["depth_sq_sum"].sum()) / n)) < 1e-15
  assert abs(sm["depth"]["abs_rel"] - float(r["depth_abs_rel_sum"].sum()) / n) < 1e-15
  assert abs(sm["depth"]["delta1"] - int(r["depth_delta1_count"].sum()) / n) < 1e-15
  assert sorted(sm["per_class"]) == [1, 2, 3]
  c3 = r["class_index"] == 3
  assert sm["per_class"][3]["num_rows"] == 2 and int(c3.sum()) == 4            # NaN rows (absent on both sides) drop out
  assert abs(sm["per_class"][3]["pooled_iou"] - int(r["class_intersection"][c3].sum()) / int(r["class_union"][c3].sum())) < 1e-15
  assert math.isnan(ER.ReprojectionResults("semantic").summary()["silhouette"]["mean_iou"])


def test_image_metrics_functions():
  from corenet_amd import image_metrics as IM
  rng = np.random.RandomState(0)
  p, g = t.from_numpy(rng.rand(3, 9, 11) < 0.5), t.from_numpy(rng.rand(3, 9, 11) < 0.4)
  p[2], g[2] = False, False
  s = IM.silhouette_counts(p, g)
  assert s.intersection.tolist() == [int((p[i] & g[i]).sum()) for i in range(3)]
  assert s.union.tolist() == [int((p[i] | g[i]).sum()) for i in range(3)]
  assert s.iou.dtype == t.float64 and math.isnan(float(s.iou[2])) and float(s.iou[0]) == int(s.intersection[0]) / int(s.union[0])
  dp = t.from_numpy(rng.rand(3, 9, 11).astype(np.float32) + 0.5)
  dg = t.from_numpy(rng.rand(3, 9, 11).astype(np.float32) + 0.5)
  dp[~p], dg[~g] = math.inf, math.inf
  d = IM.depth_errors(dp, dg, p & g)
  for i in range(3):
    v = (p[i] & g[i]).numpy()
    a, b = dp[i].numpy().astype(np.float64)[v], dg[i].numpy().astype(np.float64)[v]
    assert int(d.count[i]) == v.sum() and int(d.delta1_count[i]) == (np.maximum(a / b, b / a) < 1.25).sum()
    for got, want in ((d.abs_sum[i], np.abs(a - b).sum()), (d.sq_sum[i], ((a - b) ** 2).sum()),
                      (d.abs_rel_sum[i], (np.abs(a - b) / b).sum())):
      assert abs(float(got) - want) <= 1e-13 * max(want, 1.0)
  lp, lg = t.from_numpy(rng.randint(0, 4, (3, 9, 11))), t.from_numpy(rng.randint(0, 4, (3, 9, 11)).astype(np.int32))
  lp[0, 0, 0] = 9                                                             # outside [0, C): counted nowhere
  table = IM.label_image_overlaps(lp, lg, 4)
  want = np.zeros((3, 4, 4), np.int64)
  ok = lp.numpy() < 4
  np.add.at(want, (np.nonzero(ok)[0], lp.numpy()[ok], lg.numpy()[ok]), 1)
  assert table.dtype == t.int64 and np.array_equal(table.numpy(), want) and int(table.sum()) == 3 * 99 - 1
  for bad in (lambda: IM.silhouette_counts(p, g[:2]), lambda: IM.silhouette_counts(p.int(), g),
              lambda: IM.depth_errors(dp, dg, p.int()), lambda: IM.depth_errors(dp[0], dg[0], p[0]),
              lambda: IM.label_image_overlaps(lp, lg, 0)):
    with pytest.raises(ValueError):
      bad()


def test_errors(ER, fixture):
  pmf, ex = fixture
  for bad in (lambda: ER.reprojection_metrics_for_batch(pmf, ex, "semantic", gt="voxels"),
              lambda: ER.reprojection_metrics_for_batch(pmf[:1], ex, "semantic"),
              lambda: ER.reprojection_metrics_for_batch(pmf[:, :, :16], ex, "semantic"),
              lambda: ER.reprojection_metrics_for_batch(pmf[:, :1], ex, "semantic"),
              lambda: ER.reprojection_metrics_for_batch(pmf, ex, "fg_bg"),
              lambda: ER.reprojection_metrics_for_batch(pmf[:, :2], ex, "fg_bg"),      # scenes of 3 and 2 meshes
              lambda: ER.reprojection_metrics_for_batch(pmf, ex, "semantic", image_size=(0, 4)),
              lambda: ER.reprojection_metrics_for_batch(pmf, ex, "panoptic")):
    with pytest.raises(ValueError):
      bad()
