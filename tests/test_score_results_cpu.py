"""Score-level evaluation glue on the host: evaluation_results.ScoreResults on the twin over a two-batch synthetic run,
the shape of its CSV, the streaming hand-over of SuperResolutionInference.predict_score_histogram, and pipeline.run_eval
with and without `scores` (voxel_metrics.csv must not change by a byte).  No GPU."""
import csv
import math
import types

import numpy as np
import pytest
import torch as t

import score_metrics_check as SC


@pytest.fixture(scope="module")
def ER():
  from corenet_amd import evaluation_results as ER
  return ER


def _stand_in_batch(grid, mesh_labels, ids=None):
  B = grid.shape[0]
  return types.SimpleNamespace(grid=grid, mesh_labels=[t.tensor(v, dtype=t.int32) for v in mesh_labels],
                               scene_id=ids or [f"scene/{i}" for i in range(B)])


def _batches(task, K, seed=0):
  g = t.Generator().manual_seed(seed)
  out = []
  for labels in ([[3], [1]], [[4], [3]]):
    if task == "fg_bg":
      pmf = (t.rand((2, 2, 3, 4, 5), generator=g) * 3).softmax(1)
      grid = t.randint(0, 2, (2, 3, 4, 5), generator=g, dtype=t.int32)
    else:
      pmf = (t.rand((2, K, 3, 4, 5), generator=g) * 3).softmax(1)
      grid = t.randint(0, K, (2, 3, 4, 5), generator=g, dtype=t.int32)
    out.append((pmf.clamp(0, 1), _stand_in_batch(grid, labels)))
  return out


@pytest.mark.parametrize("task", ["fg_bg", "semantic"])
def test_score_results_two_batches(ER, task, tmp_path):
  from corenet_amd import score_metrics as SM
  classes = ["__void__", "a", "b", "c", "d"]
  K, nbins = len(classes), 10
  res = ER.ScoreResults(classes, task, nbins=nbins)
  want = [0, 0, 0]
  for pmf, ex in _batches(task, K):
    scene = np.asarray([int(v[0]) for v in ex.mesh_labels], dtype=np.int32) if task == "fg_bg" else None
    assert res.add_batch(pmf, ex) is res.histogram
    want = [a + b for a, b in zip(want, SC.reference_histogram(pmf.numpy(), ex.grid.numpy(), K, nbins, scene))]
  h = res.compute_metrics()
  assert h is res.histogram and h.nbins == nbins
  assert np.array_equal(h.table.numpy(), want[0]) and np.array_equal(h.sq.numpy(), want[1]) and int(h.bad) == 0
  s = res.summary()
  assert list(s) == classes + ["__global__"]
  assert all(tuple(v) == ER.SCORE_SUMMARY_NAMES for v in s.values())
  ece, brier = SM.expected_calibration_error(h), SM.brier_score(h)
  thr, best = SM.best_threshold(h)
  for r, name in enumerate(list(s)):
    for key, val in (("ece", ece[r]), ("brier", brier[r]), ("best_threshold", thr[r]), ("best_iou", best[r]),
                     ("ap", SM.average_precision(h)[r]), ("iou_at_0.5", SM.threshold_curve(h).iou[r, 5])):
      assert s[name][key] == float(val) or (math.isnan(s[name][key]) and math.isnan(float(val)))
  assert 0 <= s["__global__"]["ece"] <= 1 and 0 <= s["__global__"]["ap"] <= 1
  if task == "fg_bg":
    assert math.isnan(s["b"]["ap"]) and not math.isnan(s["c"]["ap"])       # no scene of class 2: a row without positives
    assert math.isnan(s["b"]["brier"])                                       # ... and without voxels
  # one pmf through score_metrics_for_batch gives the first batch's table
  pmf, ex = _batches(task, K)[0]
  one = ER.score_metrics_for_batch(pmf, ex, task, nbins=nbins, num_classes=K)
  scene = np.asarray([int(v[0]) for v in ex.mesh_labels], dtype=np.int32) if task == "fg_bg" else None
  assert np.array_equal(one.table.numpy(), SC.reference_histogram(pmf.numpy(), ex.grid.numpy(), K, nbins, scene)[0])
  plain = ER.score_metrics_for_batch(pmf, ex, task, nbins=nbins)
  assert plain.table.shape == (pmf.shape[1] + 1, nbins, 2, 2)
  # the CSV: a header, nbins + 1 threshold lines and nbins bin lines per column
  path = tmp_path / "out" / "score_metrics.csv"
  res.write_csv(str(path))
  rows = list(csv.reader(open(path, newline="")))
  assert rows[0] == ["class", "kind", "value", "tp", "fp", "fn", "iou", "precision", "recall", "count", "confidence", "frequency"]
  assert len(rows) == 1 + (K + 1) * (2 * nbins + 1) and all(len(r) == 12 for r in rows)
  for r, name in enumerate(classes + ["__global__"]):
    block = rows[1 + r * (2 * nbins + 1):1 + (r + 1) * (2 * nbins + 1)]
    assert [b[0] for b in block] == [name] * (2 * nbins + 1)
    assert [b[1] for b in block] == ["threshold"] * (nbins + 1) + ["bin"] * nbins
    assert [float(b[2]) for b in block[:nbins + 1]] == [j / nbins for j in range(nbins + 1)]
    c = SM.threshold_counts(h)
    assert [int(b[3]) for b in block[:nbins + 1]] == c.tp[r].tolist() and [int(b[5]) for b in block[:nbins + 1]] == c.fn[r].tolist()
    assert sum(int(b[9]) for b in block[nbins + 1:]) == int(h.table[r, :, :, 0].sum())
    assert block[nbins][6] == ""                                             # threshold 1: no true positive, NaN
  # a rejected voxel makes compute_metrics refuse the run
  bad = ER.ScoreResults(classes, task, nbins=nbins)
  pmf2 = pmf.clone()
  pmf2[0, 0, 0, 0, 0] = float("nan")
  bad.add_batch(pmf2, ex)
  assert int(bad.histogram.bad) == 1
  with pytest.raises(ValueError):
    bad.compute_metrics()
  with pytest.raises(ValueError):
    ER.ScoreResults(classes, task).compute_metrics()
  with pytest.raises(ValueError):
    ER.ScoreResults(classes, task, nbins=400)
  with pytest.raises(ValueError):
    ER.ScoreResults(["c%d" % i for i in range(64)], task, nbins=32)


def test_streaming_hand_over(ER):
  from corenet_amd import super_resolution as SR

  class PmfOnly(SR.MultiOffsetInferenceFn):
    pass
  args = (t.zeros(1, 3, 8, 8), t.eye(4)[None], (t.eye(4) * t.tensor([8.0, 8.0, 8.0, 1.0]))[None], t.full((1, 3), 0.5), (8, 8, 8))
  gt = t.zeros((1, 8, 8, 8), dtype=t.int32)
  with pytest.raises(TypeError):
    SR.SuperResolutionInference(PmfOnly(), (4, 4, 4)).predict_score_histogram(*args, gt)
  seen = {}

  class Streams(SR.MultiOffsetInferenceFn):
    def score_histogram(self, image, camera, v2x_native, offsets, m, gt, **kw):
      seen.update(m=m, offsets=offsets, v2x=v2x_native, gt=gt, kw=kw)
      return "histogram"
  sr = SR.SuperResolutionInference(Streams(), (4, 4, 4))
  assert sr.predict_score_histogram(*args, gt, num_classes=3, nbins=7) == "histogram"
  assert seen["m"] == 2 and t.equal(seen["offsets"], sr.get_native_offsets((8, 8, 8), t.full((1, 3), 0.5))) and seen["gt"] is gt
  assert t.allclose(seen["v2x"][0].diagonal(), t.tensor([4.0, 4.0, 4.0, 1.0]))
  assert seen["kw"] == dict(num_classes=3, scene_classes=None, nbins=7, out=None)
  # ScoreResults.add_batch_streaming hands the run's tables and the scene classes over
  res = ER.ScoreResults(["__void__", "a", "b"], "fg_bg", nbins=7)
  ex = types.SimpleNamespace(grid=gt, mesh_labels=[t.tensor([2], dtype=t.int32)], scene_id=["s/0"], input_image=args[0],
                             camera_transform=args[1], v2x_transform=args[2], grid_sampling_offset=args[3])
  assert res.add_batch_streaming(sr, ex) == "histogram"
  assert seen["kw"]["out"] is res.histogram and seen["kw"]["scene_classes"].tolist() == [2] and seen["kw"]["num_classes"] == 3


def _run_eval(monkeypatch, tmp_path, name, inference, batches, classes, **kw):
  from corenet_amd import pipeline
  monkeypatch.setattr(pipeline, "create_distributed_loader", lambda *a, **k: [ex for _, ex in batches])
  monkeypatch.setattr(pipeline, "batched_example", types.SimpleNamespace(batch=lambda b, device: b))
  monkeypatch.setattr(pipeline, "voxelize_batch", lambda ex, task, resolution, **k: ex)
  dataset = types.SimpleNamespace(classes=classes)
  out = tmp_path / name
  miou = pipeline.run_eval(inference, dataset, str(out), "semantic", 2, resolution=(3, 4, 5), device="cpu", **kw)
  return miou, out


def test_run_eval_scores_argument(ER, monkeypatch, tmp_path):
  """voxel_metrics.csv is the same bytes without `scores`, with scores=None and with a ScoreResults; the ScoreResults
  ends up with the tables of its own add_batch calls, from the pmf path and from a streaming inference."""
  classes = ["__void__", "a", "b", "c"]
  K = len(classes)
  batches = _batches("semantic", K, seed=3)
  for i, (pmf, ex) in enumerate(batches):
    ex.input_image, ex.camera_transform, ex.v2x_transform, ex.grid_sampling_offset = i, None, None, None
  calls = {"pmf": 0, "hist": 0}

  def pmf_only(image, camera, v2x, offsets, resolution):
    calls["pmf"] += 1
    return batches[image][0]
  miou0, out0 = _run_eval(monkeypatch, tmp_path, "plain", pmf_only, batches, classes)
  miou1, out1 = _run_eval(monkeypatch, tmp_path, "none", pmf_only, batches, classes, scores=None)
  res = ER.ScoreResults(classes, "semantic", nbins=10)
  miou2, out2 = _run_eval(monkeypatch, tmp_path, "scores", pmf_only, batches, classes, scores=res)
  assert calls["pmf"] == 6                                                   # one inference per batch, with scores too
  csv0 = (out0 / "voxel_metrics.csv").read_bytes()
  assert csv0 == (out1 / "voxel_metrics.csv").read_bytes() == (out2 / "voxel_metrics.csv").read_bytes() and len(csv0) > 0
  assert miou0 == miou1 == miou2
  assert not (out0 / "score_metrics.csv").exists() and not (out1 / "score_metrics.csv").exists()
  assert (out2 / "score_metrics.csv").exists() and res.reduced
  want = ER.ScoreResults(classes, "semantic", nbins=10)
  for pmf, ex in batches:
    want.add_batch(pmf, ex)
  assert t.equal(res.histogram.table, want.histogram.table) and t.equal(res.histogram.sq, want.histogram.sq)

  # a streaming inference: labels and scores both pass by pass, no pmf asked for
  from corenet_amd import score_metrics as SM, voxel_metrics as VM

  class Streaming:
    def __call__(self, *a):
      raise AssertionError("no pmf is needed")

    def predict_labels(self, image, camera, v2x, offsets, resolution, gt=None, num_classes=None, scene_classes=None, cm=None,
                       bad=None):
      return VM.label_confusion(batches[image][0], gt, num_classes, scene_classes, cm=cm, bad=bad)[0]

    def predict_score_histogram(self, image, camera, v2x, offsets, resolution, gt, num_classes=None, scene_classes=None,
                                nbins=20, out=None):
      calls["hist"] += 1
      return SM.score_histogram(batches[image][0], gt, num_classes, scene_classes, nbins=nbins, out=out)
  res3 = ER.ScoreResults(classes, "semantic", nbins=10)
  miou3, out3 = _run_eval(monkeypatch, tmp_path, "streaming", Streaming(), batches, classes, scores=res3)
  assert calls["hist"] == 2 and t.equal(res3.histogram.table, want.histogram.table)
  assert (out3 / "voxel_metrics.csv").read_bytes() == csv0 and miou3 == miou0
