"""Topology evaluation on the host (evaluation_results.topology_metrics_for_batch / TopologyResults) on
hand-made scenes (voxel_topology_check.semantic_scenes): a torus whose hole the prediction fills, a block the prediction
misses, a hollow ball predicted exactly.  The expected rows and the summary are worked out by hand below."""
import math

import numpy as np
import pytest
import torch as t

import voxel_topology_check as TC


@pytest.fixture(scope="module")
def ER():
  from corenet_amd import evaluation_results as ER
  return ER


SIZE = float(np.float32(1 / 24))                                            # the voxel edge as _voxel_sizes hands it on: float32


def _area(mask, size):
  return TC.crofton_of(TC.table_of(mask[None], 0, True)[0][0, 0], size)


def test_semantic_rows(ER):
  pred, gt = TC.semantic_scenes()
  rows = ER.topology_metrics_for_batch(*TC.batch_of(pred, gt, "cpu"), "semantic")
  # scene 0: any object, class 1 (torus / filled torus), class 2 (block / nothing); scene 1: any object and class 2.
  # Class 1 of scene 1 is empty on both sides and left out; class 2 of scene 0 has no predicted voxel and stays.
  assert rows.scene_index.tolist() == [0, 0, 0, 1, 1] and rows.class_index.tolist() == [0, 1, 2, 0, 2]
  assert rows.scene_id == ["scene0"] * 3 + ["scene1"] * 2
  filled = int(TC.filled_torus().sum())
  assert filled > 1280
  #                 b0 b1 b2 chi volume
  assert rows.gt[:, :5].tolist() == [[2, 1, 0, 1, 1288], [1, 1, 0, 0, 1280], [1, 0, 0, 1, 8], [1, 0, 1, 2, 3312], [1, 0, 1, 2, 3312]]
  assert rows.pred[:, :5].tolist() == [[1, 0, 0, 1, filled], [1, 0, 0, 1, filled], [0, 0, 0, 0, 0], [1, 0, 1, 2, 3312], [1, 0, 1, 2, 3312]]
  assert rows.gt[:, 5].tolist() == [1200 + 24, 1200, 24, 2568, 2568]
  assert int(rows.pred[0, 5]) == TC.exposed_faces_of(TC.filled_torus()) and int(rows.pred[2, 5]) == 0
  assert rows.pred_area.dtype == t.float64
  want = [_area(gt[0] > 0, SIZE), _area(gt[0] == 1, SIZE), _area(gt[0] == 2, SIZE), _area(gt[1] > 0, SIZE), _area(gt[1] == 2, SIZE)]
  assert np.allclose(rows.gt_area.numpy(), want, rtol=1e-12, atol=0)
  assert float(rows.pred_area[2]) == 0.0 and abs(float(rows.pred_area[1]) - _area(TC.filled_torus(), SIZE)) < 1e-12


def test_summary(ER):
  pred, gt = TC.semantic_scenes()
  res = ER.TopologyResults("semantic")
  res.add_batch(*TC.batch_of(pred[:1], gt[:1], "cpu"))
  res.add_batch(*TC.batch_of(pred[1:], gt[1:], "cpu"))
  s = res.summary()
  filled = int(TC.filled_torus().sum())
  assert s["connectivity"] == 26 and sorted(s["per_class"]) == [1, 2]
  c1, c2, overall, any_object = s["per_class"][1], s["per_class"][2], s["overall"], s["any_object"]
  # class 1: one row, the torus with its hole filled
  assert (c1["num_rows"], c1["mean_abs_delta_b0"], c1["mean_abs_delta_b1"], c1["mean_abs_delta_b2"], c1["topology_correct"]) == (1, 0.0, 1.0, 0.0, 0.0)
  assert c1["volume_ratio"] == filled / 1280 and c1["volume_ratio"] > 1
  assert abs(c1["area_ratio"] - _area(TC.filled_torus(), 1.0) / _area(TC.torus(), 1.0)) < 1e-12
  # class 2: the missed block (b0 1 against 0) and the exact hollow ball
  assert (c2["num_rows"], c2["mean_abs_delta_b0"], c2["mean_abs_delta_b1"], c2["mean_abs_delta_b2"], c2["topology_correct"]) == (2, 0.5, 0.0, 0.0, 0.5)
  assert c2["volume_ratio"] == 3312 / 3320
  # overall: the three class rows together
  assert overall["num_rows"] == 3 and overall["mean_abs_delta_b0"] == pytest.approx(1 / 3, abs=1e-15)
  assert overall["mean_abs_delta_b1"] == pytest.approx(1 / 3, abs=1e-15) and overall["mean_abs_delta_b2"] == 0.0
  assert overall["topology_correct"] == pytest.approx(1 / 3, abs=1e-15) and overall["volume_ratio"] == (filled + 3312) / 4600
  # any object: scene 0 has two pieces and a handle against one piece, scene 1 is exact
  assert (any_object["num_rows"], any_object["mean_abs_delta_b0"], any_object["mean_abs_delta_b1"], any_object["topology_correct"]) == (2, 0.5, 0.5, 0.5)
  empty = ER.TopologyResults("semantic").summary()
  assert empty["overall"]["num_rows"] == 0 and math.isnan(empty["overall"]["volume_ratio"]) and empty["per_class"] == {}


def test_exact_prediction(ER):
  _, gt = TC.semantic_scenes()
  res = ER.TopologyResults("semantic", connectivity=6)
  rows = res.add_batch(*TC.batch_of(gt, gt, "cpu"))
  assert t.equal(rows.pred, rows.gt) and t.equal(rows.pred_area, rows.gt_area) and rows.class_index.tolist() == [0, 1, 2, 0, 2]
  for e in [res.summary()["overall"], res.summary()["any_object"]] + list(res.summary()["per_class"].values()):
    assert (e["mean_abs_delta_b0"], e["mean_abs_delta_b1"], e["mean_abs_delta_b2"], e["topology_correct"]) == (0.0, 0.0, 0.0, 1.0)
    assert e["volume_ratio"] == 1.0 and e["area_ratio"] == 1.0


def test_fg_bg_rows_carry_the_mesh_label(ER):
  pred, gt = TC.semantic_scenes()
  pred, gt = (pred > 0).astype(np.int32), (gt > 0).astype(np.int32)
  pmf, ex = TC.batch_of(pred, gt, "cpu", mesh_labels=[t.tensor([5]), t.tensor([3])], num_classes=2)
  rows = ER.topology_metrics_for_batch(pmf, ex, "fg_bg")
  assert rows.scene_index.tolist() == [0, 0, 1, 1] and rows.class_index.tolist() == [0, 5, 0, 3]
  assert t.equal(rows.gt[0], rows.gt[1]) and t.equal(rows.pred[2], rows.pred[3])
  assert rows.gt[:, :3].tolist() == [[2, 1, 0]] * 2 + [[1, 0, 1]] * 2 and rows.pred[:, :3].tolist() == [[1, 0, 0]] * 2 + [[1, 0, 1]] * 2
  s = ER.TopologyResults("fg_bg")
  s.add_batch(pmf, ex)
  assert sorted(s.summary()["per_class"]) == [3, 5] and s.summary()["per_class"][5]["topology_correct"] == 0.0


def test_errors(ER):
  pred, gt = TC.semantic_scenes()
  bad = gt.copy()
  bad[1, 0, 0, 0] = 7
  with pytest.raises(ValueError, match="outside"):
    ER.topology_metrics_for_batch(*TC.batch_of(pred, bad, "cpu"), "semantic")
  pmf, ex = TC.batch_of(pred, gt, "cpu")
  with pytest.raises(ValueError, match="connectivity"):
    ER.topology_metrics_for_batch(pmf, ex, "semantic", connectivity=18)
  with pytest.raises(ValueError, match="pmf"):
    ER.topology_metrics_for_batch(pmf[:, :, 0], ex, "semantic")
  with pytest.raises(ValueError, match="fg_bg"):
    ER.topology_metrics_for_batch(pmf, ex, "fg_bg")
