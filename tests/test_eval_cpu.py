"""Dataset evaluation on the host: the reference's voxel metrics and its table / CSV against recorded goldens, the host
twin of crn_eval_labels (csrc/eval_labels_cpu.cpp) against the numpy restatement in eval_check.py with exact equality,
and QuantitativeResults on CPU tensors with stand-in batches.  No GPU."""
import math
import os
import types

import numpy as np
import pytest
import torch as t

import eval_check as EC


@pytest.fixture(scope="module")
def VM():
  from corenet_amd import voxel_metrics as VM
  return VM


@pytest.fixture(scope="module")
def ER():
  from corenet_amd import evaluation_results as ER
  return ER


@pytest.fixture(scope="module")
def golden(golden_dir):
  return np.load(os.path.join(golden_dir, "metrics.npz")), np.load(os.path.join(golden_dir, "voxel_metrics_table.npz"))


def _t(x):
  return None if x is None else t.from_numpy(np.ascontiguousarray(x))


# ---------------- known answers of the reference's own test ----------------
def test_known_confusion_matrix(VM):
  cm = VM.confusion_matrix(_t(EC.KNOWN_PRED), _t(EC.KNOWN_GT), 5)
  assert cm.dtype in (t.int32, t.int64)
  assert np.array_equal(cm.numpy(), EC.KNOWN_CM)
  assert np.array_equal(VM.confusion_matrix(_t(EC.KNOWN_PRED).long(), _t(EC.KNOWN_GT), 5).numpy(), EC.KNOWN_CM)
  with pytest.raises(ValueError):
    VM.confusion_matrix(_t(EC.KNOWN_PRED), _t(EC.KNOWN_GT), 4)            # label 4 >= num_classes
  with pytest.raises(AssertionError):
    VM.confusion_matrix(_t(EC.KNOWN_PRED).float(), _t(EC.KNOWN_GT), 5)
  with pytest.raises(AssertionError):
    VM.confusion_matrix(_t(EC.KNOWN_PRED)[:1], _t(EC.KNOWN_GT), 5)


def test_known_tfpn(VM):
  tfpn = VM.compute_tfpn(t.tensor(EC.KNOWN_CM, dtype=t.int32))
  for k, want in EC.KNOWN_TFPN.items():
    assert getattr(tfpn, k).tolist() == want, k


def test_known_metrics(VM):
  tfpn = VM.TfpnValues(**{k: t.tensor(v, dtype=t.int32) for k, v in EC.KNOWN_TFPN.items()})
  mm = VM.compute_voxel_metrics(tfpn)
  hit = np.array(EC.KNOWN_TFPN["tp"]) != 0
  for k, want in EC.KNOWN_METRICS.items():
    got = getattr(mm, k)
    assert got.dtype == t.float64
    np.testing.assert_allclose(got.numpy()[hit], np.array(want)[hit], rtol=1e-7)
    assert np.isnan(got.numpy()[~hit]).all()
  assert math.isnan(float(VM.nan_tp_div(t.tensor(0.0), t.tensor(3.0)))) and float(VM.nan_tp_div(t.tensor(1.0), t.tensor(4.0))) == 0.25


# ---------------- the table and its CSV against the reference's ----------------
@pytest.mark.parametrize("i", range(5))
def test_golden_table_and_csv(VM, ER, golden, golden_dir, i, tmp_path):
  metrics, tables = golden
  cm = t.from_numpy(metrics[f"cm_{i}"])
  classes = [str(c) for c in tables[f"classes_{i}"]]
  tfpn, tfg = VM.compute_tfpn(cm), VM.compute_tfpn_fg(cm)
  assert np.array_equal(np.stack([getattr(tfpn, k).numpy() for k in ("tp", "tn", "fp", "fn")]), tables[f"tfpn_{i}"])
  assert [int(getattr(tfg, k)) for k in ("tp", "tn", "fp", "fn")] == tables[f"tfpn_fg_{i}"].tolist()
  table = ER.compute_voxel_metrics(cm, classes)
  want = tables[f"table_{i}"]
  assert table.rows == ("iou", "precision", "recall") and table.columns == tuple(classes) + ("__global__",)
  got = table.values.numpy()
  assert got.dtype == np.float64 and got.shape == want.shape
  assert np.array_equal(np.isnan(got), np.isnan(want))
  assert np.nanmax(np.abs(got - want), initial=0.0) <= 1e-12
  with open(os.path.join(golden_dir, f"voxel_metrics_table_{i}.csv"), "rb") as f:
    want_csv = f.read()
  assert table.to_csv().encode() == want_csv
  q = ER.QuantitativeResults(classes, "semantic")
  q.confusion_matrix, q.bad = cm.clone(), t.zeros(1, dtype=t.int32)
  q.compute_metrics()
  miou, want_miou = q.get_mean_iou(), float(metrics[f"miou_{i}"])
  # a float64 mean of at most 13 values in [0, 1]: summation order may move it by a few 2^-53
  assert (math.isnan(miou) and math.isnan(want_miou)) or abs(miou - want_miou) <= 1e-12
  assert (math.isnan(miou) and math.isnan(VM.mean_iou(cm))) or abs(miou - VM.mean_iou(cm)) <= 1e-12
  q.write_csv(str(tmp_path / "sub" / "voxel_metrics.csv"))
  assert (tmp_path / "sub" / "voxel_metrics.csv").read_bytes() == want_csv


# ---------------- the host twin against the numpy restatement ----------------
def _run_twin(VM, scores, gt, scene, K, m, n, labels, cm, bad):
  VM.label_confusion(_t(scores), _t(gt), K, _t(scene), m, n, _t(labels), _t(cm), _t(bad))      # (_t shares memory)


@pytest.mark.parametrize("m", EC.MULTIPLIERS)
@pytest.mark.parametrize("shape", EC.SHAPES)
def test_host_twin_equals_numpy(VM, shape, m):
  D, H, W = shape
  rejecting = {False: 0, True: 0}
  for C, K, B, scene, seed in EC.kernel_cases(shape, m):
    scores, gt, sc = EC.make_case(shape, m, C, K, B, scene, seed)
    fine = (B, m * D, m * H, m * W)
    prefill = np.random.RandomState(seed).randint(0, 1 << 40, size=(K, K)).astype(np.int64)      # cm accumulates
    got_l, want_l = np.full(fine, EC.SENTINEL, np.int32), np.full(fine, EC.SENTINEL, np.int32)
    got_cm, want_cm = prefill.copy(), prefill.copy()
    got_bad, want_bad = np.array([5], np.int32), np.array([5], np.int32)
    for n in range(m ** 3):
      EC.eval_labels_ref(scores, gt, sc, K, m, n, want_l, want_cm, want_bad)
      _run_twin(VM, scores, gt, sc, K, m, n, got_l, got_cm, got_bad)
      if n == 0 and m > 1:                                   # one pass alone: the other sub-lattices keep the sentinel
        untouched = np.ones(fine, bool)
        untouched[:, 0::m, 0::m, 0::m] = False
        assert (got_l[untouched] == EC.SENTINEL).all() and (got_l[~untouched] != EC.SENTINEL).all()
    case = (shape, m, C, K, B, scene)
    assert np.array_equal(got_l, want_l), case
    assert np.array_equal(got_cm, want_cm), case
    assert got_bad[0] == want_bad[0], case
    assert (want_cm - prefill).sum() + want_bad[0] - 5 == np.prod(fine), case       # every voxel counted exactly once
    rejecting[scene] += int(want_bad[0] > 5)
  assert rejecting[False] > 0 and rejecting[True] > 0      # the cases do exercise the rejection, with and without scenes


def test_host_twin_optional_outputs_ties_and_nan(VM):
  shape, m, C, K, B = (3, 5, 7), 2, 5, 7, 3
  scores, gt, sc = EC.make_case(shape, m, C, K, B, True, 3)
  fine = gt.shape
  for n in (0, 5):
    # labels = NULL: counts alone
    cm, bad, wcm, wbad = (np.zeros((K, K), np.int64), np.zeros(1, np.int32), np.zeros((K, K), np.int64), np.zeros(1, np.int32))
    from corenet_amd import _lib
    p = _lib.ptr
    _lib.lib().crn_eval_labels_cpu(p(_t(scores)), p(_t(gt)), p(_t(sc)), B, C, K, *shape, m, n, None, p(_t(cm)), p(_t(bad)), 2)
    EC.eval_labels_ref(scores, gt, sc, K, m, n, None, wcm, wbad)
    assert np.array_equal(cm, wcm) and bad[0] == wbad[0]
    # gt = NULL: labels alone, cm / bad not needed
    got_l, want_l = np.full(fine, EC.SENTINEL, np.int32), np.full(fine, EC.SENTINEL, np.int32)
    _lib.lib().crn_eval_labels_cpu(p(_t(scores)), None, p(_t(sc)), B, C, K, *shape, m, n, p(_t(got_l)), None, None, 2)
    EC.eval_labels_ref(scores, None, sc, K, m, n, want_l, None, None)
    assert np.array_equal(got_l, want_l)
  # the first of equal maxima wins; a NaN never replaces the best and a NaN at class 0 stays
  s = np.zeros((1, 4, 1, 1, 6), np.float32)
  s[0, :, 0, 0, 0] = [1, 2, 2, 0]            # tie of classes 1 and 2 -> 1
  s[0, :, 0, 0, 1] = [3, 3, 3, 3]            # all equal -> 0
  s[0, :, 0, 0, 2] = [np.nan, 9, 9, 9]       # NaN at class 0 stays
  s[0, :, 0, 0, 3] = [0, np.nan, 1, np.nan]  # NaN skipped -> 2
  s[0, :, 0, 0, 4] = [-np.inf, -np.inf, 0, 0]
  s[0, :, 0, 0, 5] = [0, 0, 0, np.inf]
  labels, _, _ = VM.label_confusion(_t(s))
  assert labels.dtype == t.int32 and labels.reshape(-1).tolist() == [1, 0, 0, 2, 2, 3]


def test_host_twin_threads(VM):
  """Large enough for the twin to split the work over threads: the sums are integers, so the result does not move."""
  shape, m, C, K, B = (16, 64, 65), 2, 2, 5, 2
  scores, gt, sc = EC.make_case(shape, m, C, K, B, True, 11)
  fine = gt.shape
  got_l, want_l = np.full(fine, EC.SENTINEL, np.int32), np.full(fine, EC.SENTINEL, np.int32)
  got_cm, want_cm, got_bad, want_bad = np.zeros((K, K), np.int64), np.zeros((K, K), np.int64), np.zeros(1, np.int32), np.zeros(1, np.int32)
  old = t.get_num_threads()
  try:
    t.set_num_threads(4)
    for n in (0, 7):
      EC.eval_labels_ref(scores, gt, sc, K, m, n, want_l, want_cm, want_bad)
      _run_twin(VM, scores, gt, sc, K, m, n, got_l, got_cm, got_bad)
  finally:
    t.set_num_threads(old)
  assert np.array_equal(got_l, want_l) and np.array_equal(got_cm, want_cm) and got_bad[0] == want_bad[0]


def test_m1_equals_torch_argmax_confusion(VM):
  """m = 1, K = C, no scene class: the contract of crn_argmax_confusion, restated with torch."""
  g = t.Generator().manual_seed(4)
  scores = t.randn((2, 14, 4, 6, 9), generator=g)
  gt = t.randint(0, 14, (2, 4, 6, 9), generator=g, dtype=t.int32)
  labels, cm, bad = VM.label_confusion(scores, gt)
  assert t.equal(labels, scores.argmax(1).to(t.int32)) and int(bad) == 0
  assert t.equal(cm, VM.confusion_matrix(labels, gt, 14))


@pytest.mark.parametrize("m", [2, 3])
def test_all_passes_equal_argmax_of_interleaved_softmax(VM, m):
  """After all m^3 passes labels is the argmax of what crn_softmax_superres defines: the softmax over classes of pass
  n = (iz*m + iy)*m + ix at fine voxel (z*m+iz, y*m+iy, x*m+ix), here in float64 from the same scores.  The scores are
  multiples of 1/8, so the softmax keeps every strict order and ties stay exact ties (first index on both sides)."""
  B, C, D, H, W = 2, 5, 3, 4, 5
  r = np.random.RandomState(m)
  passes = (r.randint(-16, 17, size=(m ** 3, B, C, D, H, W)) / 8.0).astype(np.float32)
  e = np.exp(passes.astype(np.float64) - passes.astype(np.float64).max(2, keepdims=True))
  pmf = e / e.sum(2, keepdims=True)
  fine = pmf.reshape(m, m, m, B, C, D, H, W).transpose(3, 4, 5, 0, 6, 1, 7, 2).reshape(B, C, m * D, m * H, m * W)
  labels = t.full((B, m * D, m * H, m * W), EC.SENTINEL, dtype=t.int32)
  for n in range(m ** 3):
    VM.label_confusion(_t(passes[n]), m=m, offset_index=n, labels=labels)
  assert np.array_equal(labels.numpy(), fine.argmax(1).astype(np.int32))


# ---------------- rejections ----------------
def test_rejected_calls_touch_nothing(VM):
  from corenet_amd import _lib
  lib = _lib.lib()
  B, C, K, D, H, W, m = 2, 3, 4, 2, 3, 4, 2
  scores = t.zeros((B, C, D, H, W))
  gt = t.zeros((B, m * D, m * H, m * W), dtype=t.int32)
  sc = t.ones(B, dtype=t.int32)
  labels = t.full(gt.shape, EC.SENTINEL, dtype=t.int32)
  cm = t.full((K, K), 11, dtype=t.int64)
  bad = t.full((1,), 13, dtype=t.int32)
  p = _lib.ptr
  good = dict(scores=p(scores), gt=p(gt), sc=p(sc), B=B, C=C, K=K, D=D, H=H, W=W, m=m, n=3, labels=p(labels), cm=p(cm), bad=p(bad))
  wrong = [dict(scores=None), dict(C=0), dict(C=33), dict(K=0), dict(K=65), dict(m=0), dict(n=-1), dict(n=m ** 3), dict(B=0),
           dict(D=0), dict(H=0), dict(W=0), dict(cm=None), dict(bad=None), dict(gt=None, labels=None),
           dict(m=2 ** 20, n=0), dict(m=2 ** 31 - 1, n=0)]       # 4 * B * D * H * W * m^3 beyond int64: offsets would wrap
  fn = lib.cdll.crn_eval_labels_cpu
  for change in wrong:
    a = dict(good, **change)
    rc = fn(a["scores"], a["gt"], a["sc"], a["B"], a["C"], a["K"], a["D"], a["H"], a["W"], a["m"], a["n"], a["labels"], a["cm"],
            a["bad"], 1)
    assert rc == -1, change
    assert bool((labels == EC.SENTINEL).all()) and bool((cm == 11).all()) and int(bad) == 13, change
  a = good
  assert fn(a["scores"], a["gt"], a["sc"], B, C, K, D, H, W, m, 3, a["labels"], a["cm"], a["bad"], 1) == 0     # the good call is good
  assert int(cm.sum()) - 11 * K * K + int(bad) - 13 == B * D * H * W
  # the Python surface raises ValueError before it reaches the library
  for kw in (dict(scores=scores.double()), dict(scores=scores[0]), dict(gt=gt.long()), dict(gt=gt[:, :1]), dict(m=0),
             dict(offset_index=8), dict(num_classes=65), dict(scene_classes=sc.long()), dict(labels=labels[:1]),
             dict(cm=cm.to(t.int32)), dict(bad=bad.long()), dict(scores=t.zeros((B, 33, D, H, W)))):
    args = dict(scores=scores, gt=gt, num_classes=K, scene_classes=sc, m=m, offset_index=3, labels=labels, cm=cm, bad=bad)
    args.update(kw)
    with pytest.raises(ValueError):
      VM.label_confusion(**args)


# ---------------- QuantitativeResults on CPU tensors ----------------
def _stand_in_batch(grid, mesh_labels, ids=None):
  B = grid.shape[0]
  return types.SimpleNamespace(grid=grid, mesh_labels=[t.tensor(v, dtype=t.int32) for v in mesh_labels],
                               scene_id=ids or [f"scene/{i}" for i in range(B)])


def _reference_style(ER, VM, pmf, ex, task, K):
  pred, gt = ER.extract_labels(pmf, ex, task)
  return VM.confusion_matrix(pred, gt, K)


def test_quantitative_results_semantic(ER, VM):
  g = t.Generator().manual_seed(0)
  K = 4
  classes = ["__void__", "a", "b", "c"]
  q = ER.QuantitativeResults(classes, "semantic")
  want = t.zeros((K, K), dtype=t.int64)
  for _ in range(2):
    pmf = t.rand((2, K, 3, 4, 5), generator=g).softmax(1)
    ex = _stand_in_batch(t.randint(0, K, (2, 3, 4, 5), generator=g, dtype=t.int32), [[1, 2], [3]])
    labels = q.add_batch(pmf, ex)
    assert t.equal(labels, pmf.argmax(1).to(t.int32))
    want += _reference_style(ER, VM, pmf, ex, "semantic", K)
  table = q.compute_metrics()
  assert t.equal(q.confusion_matrix, want)
  ref = ER.compute_voxel_metrics(want, classes)
  assert table.columns == ("__void__", "a", "b", "c", "__global__") and t.equal(table.values, ref.values)
  assert abs(q.get_mean_iou() - VM.mean_iou(want)) <= 1e-12


def test_quantitative_results_fg_bg(ER, VM):
  """K = 5 dataset classes, C = 2 logits: the class of a voxel is argmax x the scene's class."""
  g = t.Generator().manual_seed(1)
  K = 5
  classes = ["__void__", "a", "b", "c", "d"]
  q = ER.QuantitativeResults(classes, "fg_bg")
  pmf = t.rand((3, 2, 3, 4, 5), generator=g).softmax(1)
  ex = _stand_in_batch(t.randint(0, 2, (3, 3, 4, 5), generator=g, dtype=t.int32), [[3], [1], [4]])
  labels = q.add_batch(pmf, ex)
  want_pred, want_gt = ER.extract_labels(pmf, ex, "fg_bg")
  assert t.equal(labels, want_pred)
  q.compute_metrics()
  want = VM.confusion_matrix(want_pred, want_gt, K)
  assert t.equal(q.confusion_matrix, want)
  assert int(want[2].sum()) == 0 and int(want[:, 2].sum()) == 0 and int(want[3, 3]) > 0        # class 2 has no scene
  assert math.isnan(float(q.metrics.row("iou")[2]))
  # a scene with two meshes has no single class
  with pytest.raises(ValueError):
    q.add_batch(pmf, _stand_in_batch(ex.grid, [[3], [1, 2], [4]]))
  # a label beyond the dataset's classes is counted as bad, and compute_metrics refuses the run
  q2 = ER.QuantitativeResults(classes, "fg_bg")
  q2.add_batch(pmf, _stand_in_batch(ex.grid, [[3], [1], [5]]))
  assert int(q2.bad) > 0
  with pytest.raises(ValueError):
    q2.compute_metrics()


def test_streaming_needs_labels_and_qualitative_wants(ER):
  from corenet_amd import super_resolution as SR

  class PmfOnly(SR.MultiOffsetInferenceFn):
    pass
  sr = SR.SuperResolutionInference(PmfOnly(), (4, 4, 4))
  with pytest.raises(TypeError):
    sr.predict_labels(t.zeros(1, 3, 8, 8), t.eye(4)[None], t.eye(4)[None], t.zeros(1, 3), (8, 8, 8))
  seen = {}

  class Streams(SR.MultiOffsetInferenceFn):
    def labels(self, image, camera, v2x_native, offsets, m, **kw):
      seen.update(m=m, offsets=offsets, v2x=v2x_native, kw=kw)
      return "labels"
  sr = SR.SuperResolutionInference(Streams(), (4, 4, 4))
  v2x = (t.eye(4) * t.tensor([8.0, 8.0, 8.0, 1.0]))[None]
  assert sr.predict_labels(t.zeros(1, 3, 8, 8), t.eye(4)[None], v2x, t.full((1, 3), 0.5), (8, 8, 8), num_classes=3) == "labels"
  assert seen["m"] == 2 and t.equal(seen["offsets"], sr.get_native_offsets((8, 8, 8), t.full((1, 3), 0.5)))
  assert t.allclose(seen["v2x"][0].diagonal(), t.tensor([4.0, 4.0, 4.0, 1.0])) and seen["kw"]["num_classes"] == 3
  assert set(seen["kw"]) == {"gt", "num_classes", "scene_classes", "cm", "bad"}
  with pytest.raises(ValueError):
    sr.predict_labels(t.zeros(1, 3, 8, 8), t.eye(4)[None], v2x, t.zeros(1, 3), (6, 6, 6))
  dataset = [types.SimpleNamespace(scene_id="s/0"), types.SimpleNamespace(scene_id="s/1")]
  qual = ER.QualitativeResults(dataset, "unused", "semantic", num_qualitative_results=1)
  assert qual.wants(types.SimpleNamespace(scene_id=["s/1", "s/0"])) and not qual.wants(types.SimpleNamespace(scene_id=["s/1"]))
