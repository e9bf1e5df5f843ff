"""Topology evaluation on the GPU (evaluation_results.TopologyResults): CUDA equals CPU exactly in
every integer and within 1e-12 in the areas and ratios on the hand-made scenes of voxel_topology_check, and the fixture
scenes evaluate their own ground truth as topologically correct."""
import math
import types

import numpy as np
import pytest
import torch as t

import voxel_topology_check as TC

pytestmark = pytest.mark.gpu


def _rows_equal(got, want):
  assert got.scene_id == want.scene_id
  for name in ("scene_index", "class_index", "pred", "gt"):
    assert t.equal(getattr(got, name), getattr(want, name)), name
  for name in ("pred_area", "gt_area"):
    assert t.allclose(getattr(got, name), getattr(want, name), rtol=1e-12, atol=0), name


def _summaries_equal(got, want):
  assert got.keys() == want.keys()
  for k, v in want.items():
    if isinstance(v, dict):
      _summaries_equal(got[k], v)
    elif isinstance(v, float) and math.isnan(v):
      assert math.isnan(got[k]), k
    elif isinstance(v, float):
      assert abs(got[k] - v) <= 1e-12 * abs(v), k
    else:
      assert got[k] == v, k


@pytest.mark.parametrize("connectivity", [6, 26])
def test_topology_results_equal_cpu(connectivity):
  from corenet_amd import evaluation_results as ER
  pred, gt = TC.semantic_scenes()
  gpu, cpu = ER.TopologyResults("semantic", connectivity), ER.TopologyResults("semantic", connectivity)
  _rows_equal(gpu.add_batch(*TC.batch_of(pred, gt, "cuda")), cpu.add_batch(*TC.batch_of(pred, gt, "cpu")))
  _rows_equal(gpu.add_batch(*TC.batch_of(gt, gt, "cuda")), cpu.add_batch(*TC.batch_of(gt, gt, "cpu")))
  _summaries_equal(gpu.summary(), cpu.summary())
  assert cpu.summary()["per_class"][1]["num_rows"] == 2
  fg = [(pred > 0).astype(np.int32), (gt > 0).astype(np.int32)]
  labels = [t.tensor([5]), t.tensor([3])]
  _rows_equal(ER.topology_metrics_for_batch(*TC.batch_of(*fg, "cuda", mesh_labels=labels, num_classes=2), "fg_bg", connectivity),
              ER.topology_metrics_for_batch(*TC.batch_of(*fg, "cpu", mesh_labels=labels, num_classes=2), "fg_bg", connectivity))


def test_topology_metrics_on_the_fixture_scenes():
  """The one-hot of the semantic ground truth is topologically correct in every row, and its class-agnostic b0 is the
  number of 26-components of the grid: scenes of 2 and 3 meshes at 32^3."""
  import os
  from corenet_amd import evaluation_results as ER, pipeline
  from corenet_amd.data import batched_example as B, dataset as D
  from corenet_amd.voxel_components import connected_components
  root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "n2_dataset")
  ds = D.CoReNetDatasetImpl(os.path.join(root, "dataset.json"), os.path.join(root, "meshes"))
  ex = pipeline.voxelize_batch(B.batch([ds[0], ds[1]]), "semantic", resolution=(32, 32, 32))
  top = int(ex.grid.amax())
  assert top >= 1
  pmf = t.nn.functional.one_hot(ex.grid.to(t.int64), top + 1).permute(0, 4, 1, 2, 3).float()
  res = ER.TopologyResults("semantic")
  rows = res.add_batch(pmf, ex)
  assert t.equal(rows.pred, rows.gt) and len(rows.scene_id) >= 4
  s = res.summary()
  for e in [s["overall"], s["any_object"]] + list(s["per_class"].values()):
    assert e["topology_correct"] == 1.0 and e["num_rows"] > 0
  any_object = rows.class_index == 0
  assert rows.scene_index[any_object].tolist() == [0, 1]
  assert t.equal(rows.gt[any_object, 0], connected_components(ex.grid > 0, 26, by_value=False).num_components.cpu())
  cpu_ex = types.SimpleNamespace(scene_id=ex.scene_id, mesh_labels=ex.mesh_labels, grid=ex.grid.cpu(), v2x_transform=ex.v2x_transform.cpu())
  _rows_equal(rows, ER.topology_metrics_for_batch(pmf.cpu(), cpu_ex, "semantic"))
