"""Score-level evaluation on the MI355X: crn_eval_scores against the library's host twin, exact on table, sq and bad, at
the smallest shapes that reach each seam of the kernel (shapes from score_tiles()); softmax_scores bit for bit; and the
streaming x2 histogram of a model against the twin on the logits of its ordinary forwards."""
import numpy as np
import pytest
import torch as t

import score_metrics_check as SC
from oracle import corenet_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def SM():
  from corenet_amd import score_metrics as SM
  return SM


def _t(x):
  return None if x is None else (x if isinstance(x, t.Tensor) else t.from_numpy(np.ascontiguousarray(x)))


def _both(SM, scores, gt, K=None, scene=None, nbins=20, from_logits=False, m=1, case=None, cuda_scores=None, cuda_gt=None):
  """Every pass of m accumulated into one used table, on the twin and on the GPU; all three tensors must be equal."""
  scores, gt, scene = _t(scores), _t(gt), _t(scene)
  Kk = scores.shape[1] if K is None else K
  pre = t.from_numpy(np.random.default_rng(1).integers(0, 1 << 40, size=(Kk + 1, nbins, 2, 2)))
  host = SM.ScoreHistogram(pre.clone(), pre[:, 0, :, 0].clone(), t.full((1,), 5, dtype=t.int64), nbins)
  dev = SM.ScoreHistogram(pre.cuda(), pre[:, 0, :, 0].cuda(), t.full((1,), 5, dtype=t.int64, device="cuda"), nbins)
  ds = scores.cuda() if cuda_scores is None else cuda_scores
  dg = gt.cuda() if cuda_gt is None else cuda_gt
  dsc = None if scene is None else scene.cuda()
  for n in range(m ** 3):
    SM.score_histogram(scores, gt, K, scene, nbins=nbins, from_logits=from_logits, m=m, offset_index=n, out=host)
    SM.score_histogram(ds, dg, K, dsc, nbins=nbins, from_logits=from_logits, m=m, offset_index=n, out=dev)
  assert t.equal(dev.table.cpu(), host.table), case
  assert t.equal(dev.sq.cpu(), host.sq), case
  assert int(dev.bad) == int(host.bad), case
  B, C = scores.shape[:2]
  counted = int((host.table[..., 0] - pre[..., 0]).sum())
  assert counted == (C + 1) * (gt.numel() - (int(host.bad) - 5)), case
  return host


def _case(seed, B, C, shape, m=1, K=None, scene=None, logits=False):
  rng = np.random.default_rng(seed)
  D, H, W = shape
  K = C if K is None else K
  sc = None if scene is None else np.asarray(scene, dtype=np.int32)
  x = (rng.standard_normal((B, C, D, H, W)) * 4).astype(np.float32) if logits else SC.random_pmf(rng, (B, C, D, H, W))
  return x, SC.random_gt(rng, B, D, H, W, m, K, sc), sc


def test_chunk_seams(SM):
  """chunk - 1, chunk and chunk + 1 voxels in one row (the last workgroup ragged, full, and one voxel long), and chunk + 4
  with four-voxel loads; pmf and logits."""
  chunk = SM.score_tiles()[0]
  for W in (chunk - 1, chunk, chunk + 1, chunk + 4):
    for logits in (False, True):
      x, gt, _ = _case(W, 1, 2, (1, 1, W), logits=logits)
      _both(SM, x, gt, from_logits=logits, case=(W, logits))
  x, gt, _ = _case(7, 2, 3, (2, 3, chunk // 4 + 4))                   # more than one workgroup per sample, B = 2, rows inside
  _both(SM, x, gt, case="rows")


@pytest.mark.parametrize("W", [1, 3, 4, 5, 17])
def test_widths_and_alignment(SM, W):
  """W in {1, 3, 4, 5, 17}; at W = 4 also buffers that start 4 bytes past a 16-byte boundary, which must take the
  one-voxel form (scores) or the strided label read (gt)."""
  x, gt, _ = _case(W, 2, 3, (3, 5, W))
  _both(SM, x, gt, case=W)
  if W % 4 == 0:
    def shifted(a):
      buf = t.empty(a.numel() + 1, dtype=a.dtype, device="cuda")
      out = buf[1:].view(a.shape)
      out.copy_(a)
      assert out.data_ptr() % 16 == 4 and out.is_contiguous()
      return out
    for mask in (1, 2, 3):
      _both(SM, x, gt, case=(W, mask), cuda_scores=shifted(_t(x)) if mask & 1 else None,
            cuda_gt=shifted(_t(gt)) if mask & 2 else None)


@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 8, 9, 16, 17, 32])
def test_every_channel_instantiation(SM, C):
  """Both ends of each CT instantiation, four-voxel and one-voxel loads, pmf and logits."""
  for W in (8, 7):
    for logits in (False, True):
      x, gt, _ = _case(C + W, 2, C, (2, 5, W), logits=logits)
      _both(SM, x, gt, nbins=10, from_logits=logits, case=(C, W, logits))


@pytest.mark.parametrize("m", [1, 2, 3])
def test_multipliers_every_offset(SM, m):
  for W in (4, 5):
    x, gt, sc = _case(m + W, 2, 2, (3, 2, W), m=m, K=14, scene=(3, 13), logits=True)
    _both(SM, x, gt, K=14, scene=sc, from_logits=True, m=m, case=(m, W))


def test_entry_limit(SM):
  """(K + 1) * nbins at the limit of the LDS table."""
  limit = SM.score_tiles()[1]
  x, gt, _ = _case(1, 1, 7, (2, 4, 40))
  assert 8 * 256 == limit
  _both(SM, x, gt, nbins=256, case="K 7 nbins 256")
  x, gt, sc = _case(2, 2, 2, (2, 4, 40), K=31, scene=(30, 7))
  assert 32 * 64 == limit
  _both(SM, x, gt, K=31, scene=sc, nbins=64, case="K 31 nbins 64")


def test_one_key_and_changing_keys(SM):
  """One key throughout except the last voxel (the register run and the contended address), and a key that changes at
  every voxel (a flush each time)."""
  chunk = SM.score_tiles()[0]
  W = chunk + 8
  for C in (2, 14):
    p = np.zeros((1, C, 1, 1, W), dtype=np.float32)
    p[0, 0] = 1.0
    gt = np.zeros((1, 1, 1, W), dtype=np.int32)
    p[0, 0, 0, 0, -1], p[0, 1, 0, 0, -1], gt[0, 0, 0, -1] = 0.25, 0.75, 1
    _both(SM, p, gt, case=("one key", C))
    # bins cycle with the voxel index in every row, labels alternate
    idx = np.arange(W)
    p = np.zeros((1, C, 1, 1, W), dtype=np.float32)
    p[0, 1, 0, 0] = ((idx % 16) / 16.0).astype(np.float32)
    p[0, 0, 0, 0] = 1 - p[0, 1, 0, 0]
    gt = (idx % 2).astype(np.int32).reshape(1, 1, 1, W)
    _both(SM, p, gt, nbins=16, case=("changing", C))


def test_bad_voxels_head_body_tail(SM):
  """Bad voxels in the first, a middle and the last four-voxel item of a sample, in each position of the item, by every
  rule; W a multiple of four and not."""
  for W in (16, 15):
    x, gt, sc = _case(W, 3, 3, (2, 3, W), K=7, scene=(1, 2, 1))
    S = 2 * 3 * W
    flat, g = x.reshape(3, 3, S), gt.reshape(3, S)
    for k, v in enumerate((0, 1, 2, 3, S // 2 + 1, S // 2 + 2, S - 4, S - 3, S - 2, S - 1)):
      if k % 5 == 0: flat[0, k % 3, v] = np.nan
      elif k % 5 == 1: flat[0, k % 3, v] = -1e-6
      elif k % 5 == 2: flat[0, k % 3, v] = 1.0000001
      elif k % 5 == 3: g[0, v] = -1
      else: g[0, v] = 7
    g[1, 5] = 4                                                    # g = 8 at scene class 2
    h = _both(SM, x, gt, K=7, scene=sc, case=("bad", W))
    assert int(h.bad) - 5 == 11


def test_scene_class_per_sample(SM):
  """B = 3 with a different scene class per sample, one of them without a row for its foreground."""
  x, gt, sc = _case(3, 3, 2, (3, 4, 8), K=14, scene=(5, 13, 1))
  _both(SM, x, gt, K=14, scene=sc, case="scenes")
  sc2 = np.asarray([5, 14, 0], dtype=np.int32)                     # sample 1: (C - 1) * s >= K; sample 2: s < 1
  h = _both(SM, x, gt, K=14, scene=sc2, case="bad scenes")
  assert int(h.bad) - 5 == 2 * 3 * 4 * 8


def test_two_calls_accumulate(SM):
  x, gt, _ = _case(11, 2, 3, (2, 3, 8))
  one = SM.score_histogram(_t(x).cuda(), _t(gt).cuda())
  two = SM.score_histogram(_t(x).cuda(), _t(gt).cuda(), out=SM.score_histogram(_t(x).cuda(), _t(gt).cuda()))
  assert t.equal(two.table, 2 * one.table) and t.equal(two.sq, 2 * one.sq) and int(two.bad) == 0
  want = SC.reference_histogram(x, gt, 3, 20)
  assert np.array_equal(one.table.cpu().numpy(), want[0]) and np.array_equal(one.sq.cpu().numpy(), want[1])


@pytest.mark.parametrize("C", [1, 2, 3, 14, 32])
def test_softmax_scores_bit_equal(SM, C):
  x = _t(SC.softmax_test_logits(np.random.default_rng(C), C, rows=1031))
  host, dev = SM.softmax_scores(x), SM.softmax_scores(x.cuda()).cpu()
  assert t.equal(host.view(t.int32), dev.view(t.int32))
  x = x.reshape(1031, C).t().contiguous()[None]                    # [1, C, 1031]: the voxels along the lanes
  x[0, 0, 5] = float("nan")
  host, dev = SM.softmax_scores(x), SM.softmax_scores(x.cuda()).cpu()
  assert t.equal(host.view(t.int32), dev.view(t.int32)) and bool(t.isnan(host[0, :, 5]).all())


def test_rejected_calls_launch_nothing(SM):
  from corenet_amd import _lib
  from corenet_amd.backend import default_backend
  be = default_backend()
  x, gt, _ = _case(1, 2, 3, (2, 3, 4))
  s, g = _t(x).cuda(), _t(gt).cuda()
  h = SM.empty_histogram(3, 20, "cuda")
  for kw in (dict(C=33), dict(K=65), dict(n=1), dict(m=0), dict(nbins=0), dict(nbins=257), dict(K=8, nbins=256)):
    a = {**dict(C=3, K=3, n=0, m=1, nbins=20), **kw}
    with pytest.raises(_lib.HipError):
      be.eval_scores(s, False, g, None, 2, a["C"], a["K"], 2, 3, 4, a["m"], a["n"], a["nbins"], h.table, h.sq, h.bad)
  with pytest.raises(_lib.HipError):
    be.eval_scores(s, False, None, None, 2, 3, 3, 2, 3, 4, 1, 0, 20, h.table, h.sq, h.bad)
  t.cuda.synchronize()
  assert int(h.table.sum()) == 0 and int(h.sq.sum()) == 0 and int(h.bad) == 0


def test_streaming_histogram_x2_model(SM):
  """h7 at x2, B = 1, deterministic mode: predict_score_histogram equals the sum over the eight passes of the host twin's
  score_histogram(from_logits, m = 2, offset_index = n) on the logits of eight ordinary eval forwards, exactly; and
  nothing of the size of a pmf is allocated on the way."""
  from corenet_amd import super_resolution as SR
  from corenet_amd.backend import default_backend
  from corenet_amd.model.core_net import CoreNet, CoreNetConfig, DecoderConfig
  model = CoreNet(CoreNetConfig(DecoderConfig((128, 128, 128), 2, 2, 64, 0.75)), device="cuda", decoder_math="bf16x3")
  model.load_state_dict(O.make_state(0, 2, nbt=100, logit_scale=2e-4))
  model.eval()
  image, _, _, _ = O.synthetic_batch(1, 0, 2)
  image, camera = image.cuda(), O.canonical_camera()[None].cuda()
  v2v, go = O.scale([128.0] * 3)[None].cuda(), t.full((1, 3), 0.5).cuda()

  class State: pass
  st = State(); st.model = model
  sr = SR.super_resolution_from_state(st)
  res = (256, 256, 256)
  gt = t.randint(0, 2, (1,) + res, generator=t.Generator().manual_seed(9), dtype=t.int32)
  native = sr.get_native_offsets(res, go)
  vs = camera @ (v2v @ O.scale([0.5] * 3).cuda()).inverse()
  be = default_backend()
  prev = bool(getattr(be, "_deterministic", False))
  try:
    be.set_deterministic(True)
    g = gt.cuda()
    got = sr.predict_score_histogram(image, camera, v2v, go, res, g, nbins=20)
    want = SM.empty_histogram(2, 20, "cpu")
    with t.no_grad():
      for n in range(8):
        SM.score_histogram(model(image, vs, native[n]).cpu(), gt, nbins=20, from_logits=True, m=2, offset_index=n, out=want)
    t.cuda.synchronize()
    t.cuda.empty_cache()
    base = t.cuda.memory_allocated()
    t.cuda.reset_peak_memory_stats()
    again = sr.predict_score_histogram(image, camera, v2v, go, res, g, nbins=20, out=got)
    t.cuda.synchronize()
    rise = t.cuda.max_memory_allocated() - base
  finally:
    be.set_deterministic(prev)
  assert again is got
  assert int(want.bad) == 0 and int(want.table[..., 0].sum()) == 3 * 256 ** 3
  assert t.equal(got.table.cpu(), 2 * want.table) and t.equal(got.sq.cpu(), 2 * want.sq) and int(got.bad) == 0
  pmf_bytes = 2 * 256 ** 3 * 4
  print("peak rise of one x2 predict_score_histogram call", rise, "bytes; gt on the device", gt.numel() * 4, "one pmf", pmf_bytes)
  assert rise < pmf_bytes
  model.train()
  with pytest.raises(AssertionError):
    sr.predict_score_histogram(image, camera, v2v, go, res, g)
