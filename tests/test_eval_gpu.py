"""Dataset evaluation on the MI355X: crn_eval_labels against the library's host twin (exact), the streaming x2 labels of
a model against its ordinary forwards and against the pmf path, their memory, and pipeline.run_eval end to end on the
fixture dataset."""
import dataclasses
import os

import numpy as np
import pytest
import torch as t

import eval_check as EC
from oracle import corenet_oracle as O

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
MATHS = ["bf16x3", "fp32"]


def _model(nc, sd, decoder_math):
  from corenet_amd.model.core_net import CoreNet, CoreNetConfig, DecoderConfig
  m = CoreNet(CoreNetConfig(DecoderConfig((128, 128, 128), nc, 2, 64, 0.75)), device="cuda", decoder_math=decoder_math)
  missing = m.load_state_dict(sd)
  assert not missing.missing_keys and not missing.unexpected_keys
  return m


def _gpu_equals_twin(shape, m, C, K, B, scene, seed):
  from corenet_amd import voxel_metrics as VM
  D, H, W = shape
  scores, gt, sc = EC.make_case(shape, m, C, K, B, scene, seed)
  fine = (B, m * D, m * H, m * W)
  prefill = t.from_numpy(np.random.RandomState(seed).randint(0, 1 << 40, size=(K, K)).astype(np.int64))
  host = [t.from_numpy(scores), t.from_numpy(gt), None if sc is None else t.from_numpy(sc),
          t.full(fine, EC.SENTINEL, dtype=t.int32), prefill.clone(), t.full((1,), 5, dtype=t.int32)]
  dev = [None if x is None else x.cuda() for x in host]
  for n in range(m ** 3):
    for s, g, c, l, cm, bad in (host, dev):
      VM.label_confusion(s, g, K, c, m, n, l, cm, bad)
  case = (shape, m, C, K, B, scene)
  assert t.equal(dev[3].cpu(), host[3]), case
  assert t.equal(dev[4].cpu(), host[4]), case
  assert int(dev[5]) == int(host[5]), case
  assert int((host[4] - prefill).sum()) + int(host[5]) - 5 == int(np.prod(fine)), case


@pytest.mark.parametrize("m", EC.MULTIPLIERS)
@pytest.mark.parametrize("shape", EC.SHAPES)
def test_kernel_equals_host_twin(shape, m):
  for C, K, B, scene, seed in EC.kernel_cases(shape, m):
    _gpu_equals_twin(shape, m, C, K, B, scene, seed)


def test_kernel_many_workgroups_and_optional_outputs():
  """31200 voxels per sample: 16 workgroups per sample, eight rounds of the grid-stride loop each, the last one ragged;
  then labels = NULL and gt = NULL."""
  from corenet_amd import voxel_metrics as VM
  from corenet_amd.backend import default_backend
  shape = (6, 40, 130)
  for C, K, scene in ((2, 5, True), (14, 14, False), (32, 64, False)):
    _gpu_equals_twin(shape, 2, C, K, 2, scene, 77 + C)
  be = default_backend()
  C, K, B, m, n = 5, 7, 3, 2, 5
  scores, gt, sc = EC.make_case((3, 5, 7), m, C, K, B, True, 3)
  want_l, want_cm, want_bad = np.full(gt.shape, EC.SENTINEL, np.int32), np.zeros((K, K), np.int64), np.zeros(1, np.int32)
  EC.eval_labels_ref(scores, gt, sc, K, m, n, want_l, want_cm, want_bad)
  s, g, c = t.from_numpy(scores).cuda(), t.from_numpy(gt).cuda(), t.from_numpy(sc).cuda()
  cm, bad = t.zeros((K, K), dtype=t.int64, device="cuda"), t.zeros(1, dtype=t.int32, device="cuda")
  be.eval_labels(s, g, c, B, C, K, 3, 5, 7, m, n, None, cm, bad)
  assert np.array_equal(cm.cpu().numpy(), want_cm) and int(bad) == int(want_bad[0])
  labels = t.full(gt.shape, EC.SENTINEL, dtype=t.int32, device="cuda")
  be.eval_labels(s, None, c, B, C, K, 3, 5, 7, m, n, labels, None, None)
  assert np.array_equal(labels.cpu().numpy(), want_l)
  # rejected calls launch nothing
  from corenet_amd import _lib
  for bad_args in (dict(C=33), dict(K=65), dict(n=8), dict(m=0)):
    a = {**dict(C=C, K=K, n=n, m=m), **bad_args}
    with pytest.raises(_lib.HipError):
      be.eval_labels(s, g, c, B, a["C"], a["K"], 3, 5, 7, a["m"], a["n"], labels, cm, bad)
  with pytest.raises(_lib.HipError):
    be.eval_labels(s, g, c, B, C, K, 3, 5, 7, m, n, labels, None, bad)
  t.cuda.synchronize()
  assert np.array_equal(labels.cpu().numpy(), want_l) and np.array_equal(cm.cpu().numpy(), want_cm)


def test_kernel_unaligned_buffers():
  """W a multiple of 4 with buffers that start 4 bytes past a 16-byte boundary: the four-voxel reads of the scores, and at
  m = 1 those of the ground truth and the labels, need aligned addresses, so the kernel has to notice and take its
  one-voxel form.  Every combination of (scores, gt, labels) aligned or not, m = 1 and 2, against the host twin."""
  from corenet_amd import voxel_metrics as VM
  shape, C, K, B = (3, 5, 8), 5, 7, 2

  def shifted(x, on):
    if not on:
      return x.cuda()
    buf = t.empty(x.numel() + 1, dtype=x.dtype, device="cuda")
    out = buf[1:].view(x.shape)
    out.copy_(x)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out
  for m in (1, 2):
    scores, gt, sc = EC.make_case(shape, m, C, K, B, True, 40 + m)
    want_l, want_cm, want_bad = np.full(gt.shape, EC.SENTINEL, np.int32), np.zeros((K, K), np.int64), np.zeros(1, np.int32)
    n = m ** 3 - 1
    EC.eval_labels_ref(scores, gt, sc, K, m, n, want_l, want_cm, want_bad)
    for mask in range(8):
      s = shifted(t.from_numpy(scores), mask & 1)
      g = shifted(t.from_numpy(gt), mask & 2)
      l = shifted(t.full(gt.shape, EC.SENTINEL, dtype=t.int32), mask & 4)
      _, cm, bad = VM.label_confusion(s, g, K, t.from_numpy(sc).cuda(), m, n, l)
      assert np.array_equal(l.cpu().numpy(), want_l), (m, mask)
      assert np.array_equal(cm.cpu().numpy(), want_cm) and int(bad) == int(want_bad[0]), (m, mask)


def _sr_inputs():
  image, _, _, _ = O.synthetic_batch(1, 0, 2)
  camera = O.canonical_camera()[None].cuda()
  v2v = O.scale([128.0] * 3)[None].cuda()
  go = t.full((1, 3), 0.5).cuda()
  return image.cuda(), camera, v2v, go


@pytest.mark.parametrize("math", MATHS)
def test_streaming_labels_x2_model(math):
  """h7 at x2, B = 1 (the setting of test_super_resolution_x2_golden_and_encoder_reuse).
  Deterministic mode: predict_labels equals the interleaved argmax of the logits of eight ordinary eval forwards exactly,
  and its confusion matrix against a random ground truth equals the host twin's on those logits.
  Default mode: labels equal the argmax of the pmf path wherever the two largest probabilities are at least 2e-4 apart
  (twice the 1e-4 run-to-run pmf bound of the test named above); at most 1 % of the voxels may be that close.
  Memory: after a warm-up call, one predict_labels call raises the peak by less than one stash of the m^3 passes
  (m^3 B C D H W 4 bytes; the label grid is half of that at C = 2)."""
  from corenet_amd import super_resolution as SR, voxel_metrics as VM
  from corenet_amd.backend import default_backend
  m = _model(2, O.make_state(0, 2, nbt=100, logit_scale=2e-4), math).eval()
  image, camera, v2v, go = _sr_inputs()

  class State: pass
  st = State(); st.model = m
  sr = SR.super_resolution_from_state(st)
  res = (256, 256, 256)
  gt = t.randint(0, 2, (1,) + res, generator=t.Generator().manual_seed(9), dtype=t.int32)
  native = sr.get_native_offsets(res, go)
  vs = camera @ (v2v @ O.scale([0.5] * 3).cuda()).inverse()
  be = default_backend()
  prev = bool(getattr(be, "_deterministic", False))
  try:
    be.set_deterministic(True)
    cm, bad = t.zeros((2, 2), dtype=t.int64, device="cuda"), t.zeros(1, dtype=t.int32, device="cuda")
    labels = sr.predict_labels(image, camera, v2v, go, res, gt=gt.cuda(), cm=cm, bad=bad)
    assert labels.shape == (1,) + res and labels.dtype == t.int32
    want = t.empty((1,) + res, dtype=t.int32)
    want_cm, want_bad = t.zeros((2, 2), dtype=t.int64), t.zeros(1, dtype=t.int32)
    with t.no_grad():
      for n in range(8):
        logits = m(image, vs, native[n]).cpu()
        want[:, n // 4::2, (n // 2) % 2::2, n % 2::2] = logits.argmax(1).to(t.int32)
        VM.label_confusion(logits, gt, m=2, offset_index=n, labels=t.empty_like(want), cm=want_cm, bad=want_bad)
    print("deterministic mode: voxels that differ", int((labels.cpu() != want).sum()), "foreground share",
          float((want == 1).float().mean()))
    assert t.equal(labels.cpu(), want)
    assert t.equal(cm.cpu(), want_cm) and int(bad) == 0 and int(cm.sum()) == 256 ** 3
    assert t.equal(cm.cpu(), VM.confusion_matrix(want, gt, 2))
  finally:
    be.set_deterministic(prev)
  # default mode against the pmf path
  pmf = sr(image, camera, v2v, go, res)
  labels = sr.predict_labels(image, camera, v2v, go, res)
  top = pmf.topk(2, dim=1).values
  clear = (top[:, 0] - top[:, 1]) >= 2e-4
  excluded = 1.0 - float(clear.float().mean())
  print("default mode: share of voxels under the 2e-4 gap", excluded, "disagreeing among the clear ones",
        int((labels != pmf.argmax(1))[clear].sum()))
  assert excluded <= 0.01
  assert t.equal(labels[clear], pmf.argmax(1).to(t.int32)[clear])
  del pmf, top, clear, labels
  # memory of one streaming call
  t.cuda.synchronize()
  t.cuda.empty_cache()
  base = t.cuda.memory_allocated()
  t.cuda.reset_peak_memory_stats()
  labels = sr.predict_labels(image, camera, v2v, go, res)
  t.cuda.synchronize()
  rise = t.cuda.max_memory_allocated() - base
  stash = 8 * 1 * 2 * 128 ** 3 * 4
  print("peak rise of one x2 predict_labels call", rise, "bytes; one stash", stash)
  assert labels.numel() * 4 <= rise < stash
  m.train()
  with pytest.raises(AssertionError):
    sr.predict_labels(image, camera, v2v, go, res)


@pytest.fixture(scope="module")
def fixture_dataset():
  from corenet_amd.data import dataset as D
  root = os.path.join(G, "n2_dataset")
  g = t.Generator().manual_seed(5)

  def big_image(scene, el):
    return dataclasses.replace(el, input_image=t.randint(0, 256, (3, 256, 256), generator=g, dtype=t.uint8))
  ds = D.CoReNetDatasetImpl(os.path.join(root, "dataset.json"), os.path.join(root, "meshes"), data_transforms=[big_image])
  # the images are drawn once, so that every pass over the dataset sees the same elements
  els = [ds[0], ds[1]]

  class Fixed(t.utils.data.Dataset):
    classes = ds.classes

    def __len__(self):
      return len(els)

    def __getitem__(self, i):
      return els[int(i)]
  return Fixed()


@pytest.fixture(scope="module")
def semantic_model():
  return _model(4, O.make_state(0, 4, nbt=100, logit_scale=2e-4), "bf16x3").eval()


def test_run_eval_end_to_end(fixture_dataset, semantic_model, tmp_path):
  """pipeline.run_eval on the two fixture scenes, task semantic (4 classes), batch 2, deterministic mode: the streaming
  inference and a pmf-only inference function on the same model write identical voxel_metrics.csv files, the returned mean
  IoU is voxel_metrics.mean_iou of the matrix argmax_confusion gives on the same logits, and a QualitativeResults for one
  scene draws exactly that scene."""
  from corenet_amd import evaluation_results as ER, pipeline, super_resolution as SR, voxel_metrics as VM
  from corenet_amd.backend import default_backend
  from corenet_amd.data import batched_example as B
  model, ds = semantic_model, fixture_dataset
  assert len(ds.classes) == 4

  class State: pass
  st = State(); st.model = model
  sr = SR.super_resolution_from_state(st)
  calls = {"pmf": 0}

  def pmf_only(image, camera, v2x, offsets, resolution):
    calls["pmf"] += 1
    with t.no_grad():
      return model(image, camera @ v2x.inverse(), offsets).softmax(1)
  be = default_backend()
  prev = bool(getattr(be, "_deterministic", False))
  try:
    be.set_deterministic(True)
    qual = ER.QualitativeResults(ds, str(tmp_path / "img"), "semantic", num_qualitative_results=1)
    miou_s = pipeline.run_eval(sr, ds, str(tmp_path / "streaming"), "semantic", 2, qualitative=qual)
    miou_p = pipeline.run_eval(pmf_only, ds, str(tmp_path / "pmf"), "semantic", 2)
    assert calls["pmf"] == 1
    # the same logits, counted by the kernel this project had before
    ex = pipeline.voxelize_batch(B.batch([ds[0], ds[1]]), "semantic")
    with t.no_grad():
      logits = model(ex.input_image, ex.camera_transform @ ex.v2x_transform.inverse(), ex.grid_sampling_offset)
    _, cm = VM.argmax_confusion(logits, ex.grid, 4)
  finally:
    be.set_deterministic(prev)
  csv_s = (tmp_path / "streaming" / "voxel_metrics.csv").read_bytes()
  csv_p = (tmp_path / "pmf" / "voxel_metrics.csv").read_bytes()
  print(csv_s.decode(), "mean IoU", miou_s, miou_p, VM.mean_iou(cm))
  assert csv_s == csv_p and csv_s == ER.compute_voxel_metrics(cm, ds.classes).to_csv().encode()
  assert int(cm.sum()) == 2 * 128 ** 3
  want = VM.mean_iou(cm)
  assert miou_s == miou_p and (miou_s == want or (np.isnan(miou_s) and np.isnan(want)) or abs(miou_s - want) <= 1e-12)
  assert sorted(os.listdir(tmp_path / "img")) == ["img_%s.png" % ds[0].scene_id.replace("/", "_")]


def test_run_eval_x2_resolution(fixture_dataset, semantic_model, tmp_path):
  """resolution = 256^3: the ground truth is voxelized at 256^3 and the model streams x2 labels against it."""
  from corenet_amd import pipeline, super_resolution as SR

  class State: pass
  st = State(); st.model = semantic_model
  sr = SR.super_resolution_from_state(st)
  seen = {}
  inner = sr.inference_fn.labels

  def spy(*a, **kw):
    seen["m"], seen["cm"] = a[4], kw["cm"]
    return inner(*a, **kw)
  sr.inference_fn.labels = spy
  miou = pipeline.run_eval(sr, fixture_dataset, str(tmp_path), "semantic", 2, resolution=(256,) * 3)
  assert seen["m"] == 2 and int(seen["cm"].sum()) == 2 * 256 ** 3
  lines = (tmp_path / "voxel_metrics.csv").read_text().split("\n")
  assert lines[0].split(",") == [""] + [str(c) for c in fixture_dataset.classes] + ["__global__"] and len(lines[0].split(",")) == 6
  assert [ln.split(",")[0] for ln in lines[1:4]] == ["iou", "precision", "recall"] and lines[4:] == [""]
  assert isinstance(miou, float)
