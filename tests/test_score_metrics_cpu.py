"""Score-level evaluation on the host: the twin of crn_eval_scores (csrc/eval_scores_cpu.cpp) against the exact numpy
reference in score_metrics_check.py on every element of table, sq and bad; the shared softmax against a float64 softmax;
the derived quantities on cases with closed-form answers; every ValueError and CRN_EINVAL rule.  No GPU.

Softmax bound: the largest absolute error of softmax_scores against the float64 softmax over score_metrics_check's
logits (spanning +-30, C in {1, 2, 3, 14, 32}) was measured on the host at 3.2e-7 (C = 32, where the float32 sum of 32
terms dominates; 8.4e-8 at C = 2).  The bound is four times that, capped at 1e-6: 1e-6."""
import math

import numpy as np
import pytest
import torch as t

import score_metrics_check as SC

SOFTMAX_MEASURED = 3.2e-7
SOFTMAX_BOUND = min(4 * SOFTMAX_MEASURED, 1e-6)


@pytest.fixture(scope="module")
def SM():
  from corenet_amd import score_metrics as SM
  return SM


def _t(x):
  return None if x is None else t.from_numpy(np.ascontiguousarray(x))


def _assert_equal(h, want, case):
  table, sq, bad = want
  assert np.array_equal(h.table.numpy(), table), case
  assert np.array_equal(h.sq.numpy(), sq), case
  assert int(h.bad) == bad, case


# (C, K, scene classes or None): K = C, and fg_bg with mixed scene classes
CLASS_CASES = [(1, 1, None), (2, 2, None), (3, 3, None), (14, 14, None), (32, 32, None), (2, 14, (3, 13, 1))]
NBINS_OF = {1: 256, 2: 10, 3: 1, 14: 64, 32: 2}


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("C,K,scene", CLASS_CASES)
def test_twin_equals_reference(SM, C, K, scene, m):
  """Every offset of m, each pass on its own and all of them accumulated into one table."""
  rng = np.random.default_rng(100 * C + m)
  B = 3 if scene else 2
  D, H, W = 2, 3, 5
  nbins = 20 if scene else NBINS_OF[C]
  sc = None if scene is None else np.asarray(scene, dtype=np.int32)
  pmf = SC.random_pmf(rng, (B, C, D, H, W))
  gt = SC.random_gt(rng, B, D, H, W, m, K, sc)
  total = SM.empty_histogram(K, nbins, "cpu")
  want_total = [0, 0, 0]
  for n in range(m ** 3):
    want = SC.reference_histogram(pmf, gt, K, nbins, sc, m, n)
    h = SM.score_histogram(_t(pmf), _t(gt), K, _t(sc), nbins=nbins, m=m, offset_index=n)
    _assert_equal(h, want, (C, K, m, n))
    assert int(h.table[..., 0].sum()) == (C + 1) * B * D * H * W and want[2] == 0
    assert SM.score_histogram(_t(pmf), _t(gt), K, _t(sc), nbins=nbins, m=m, offset_index=n, out=total) is total
    want_total = [a + b for a, b in zip(want_total, want)]
  _assert_equal(total, want_total, (C, K, m, "accumulated"))


@pytest.mark.parametrize("C,nbins", [(2, 1), (2, 2), (2, 10), (2, 64), (2, 256), (7, 256), (31, 64), (14, 136)])
def test_twin_nbins_and_entry_limit(SM, C, nbins):
  """(7, 256), (31, 64) and (14, 136) sit on the limit or just under it: (K + 1) * nbins = 2048, 2048 and 2040."""
  rng = np.random.default_rng(nbins + C)
  pmf = SC.random_pmf(rng, (1, C, 2, 3, 7), sharp=1.0)
  gt = SC.random_gt(rng, 1, 2, 3, 7, 1, C)
  _assert_equal(SM.score_histogram(_t(pmf), _t(gt), nbins=nbins), SC.reference_histogram(pmf, gt, C, nbins), (C, nbins))


@pytest.mark.parametrize("nbins", [1, 2, 16, 64, 256])
def test_twin_bin_edges(SM, nbins):
  """Scores exactly on the edges j / nbins (exact in float32: nbins is a power of two), one float32 step below and above
  them, 0 and 1: the edge belongs to the upper bin, 1 to the last."""
  edges = np.arange(nbins + 1, dtype=np.float64) / nbins
  p1 = np.concatenate([edges, np.nextafter(edges[1:].astype(np.float32), np.float32(0)),
                       np.nextafter(edges[:-1].astype(np.float32), np.float32(1))]).astype(np.float32)
  pmf = np.stack([(1 - p1.astype(np.float64)).astype(np.float32), p1])[None, :, None, None, :]
  gt = (np.arange(p1.size) % 2).astype(np.int32)[None, None, None, :]
  h = SM.score_histogram(_t(pmf), _t(gt), nbins=nbins)
  _assert_equal(h, SC.reference_histogram(pmf, gt, 2, nbins), nbins)
  # the edges alone: edge j opens bin j, and 1 joins the last bin
  e = SM.score_histogram(_t(pmf[..., :nbins + 1]), _t(gt[..., :nbins + 1]), nbins=nbins)
  want = np.ones(nbins, dtype=np.int64)
  want[-1] += 1
  assert np.array_equal(e.table[1, :, :, 0].sum(1).numpy(), want)


def test_twin_bad_voxels_and_accumulation(SM):
  """Every kind of bad voxel, counted in bad and nowhere else, on top of a table that is already in use."""
  rng = np.random.default_rng(5)
  B, C, K, D, H, W, nbins = 5, 3, 7, 2, 3, 5, 10
  pmf = SC.random_pmf(rng, (B, C, D, H, W))
  gt = rng.integers(0, 3, size=(B, D, H, W)).astype(np.int32)
  sc = np.asarray([1, 2, 0, -3, 4], dtype=np.int32)        # sample 2, 3: s < 1; sample 4: (C - 1) * s = 8 >= K
  pmf[0, 1, 0, 0, 0] = np.nan
  pmf[0, 0, 0, 0, 1] = -1e-9
  pmf[0, 2, 0, 0, 2] = np.nextafter(np.float32(1), np.float32(2))
  pmf[0, 1, 0, 0, 3] = np.inf
  pmf[0, 0, 1, 2, 4] = -np.inf
  gt[0, 1, 0, 0] = -1
  gt[0, 1, 0, 1] = K                                       # g = 7 outside [0, 7)
  gt[1, 0, 0, 0] = 4                                       # g = 8 at scene class 2
  gt[1, 0, 0, 1] = 3                                       # g = 6: inside
  want = SC.reference_histogram(pmf, gt, K, nbins, sc)
  assert want[2] == 5 + 2 + 1 + 3 * D * H * W
  h = SM.score_histogram(_t(pmf), _t(gt), K, _t(sc), nbins=nbins)
  _assert_equal(h, want, "bad")
  assert int(h.table[..., 0].sum()) == (C + 1) * (B * D * H * W - want[2])
  # accumulation into a used out
  used = SM.ScoreHistogram(t.full_like(h.table, 7), t.full_like(h.sq, 1 << 40), t.full_like(h.bad, 3), nbins)
  SM.score_histogram(_t(pmf), _t(gt), K, _t(sc), nbins=nbins, out=used)
  _assert_equal(used, (want[0] + 7, want[1] + (1 << 40), want[2] + 3), "accumulated")


def test_twin_threads(SM):
  """65536 voxels: the twin splits them over threads; one thread and many give the same tables."""
  from corenet_amd import _lib
  rng = np.random.default_rng(9)
  B, C, D, H, W, nbins = 2, 3, 32, 32, 32, 20
  pmf, gt = _t(SC.random_pmf(rng, (B, C, D, H, W))), _t(SC.random_gt(rng, B, D, H, W, 1, C))
  hs = []
  for threads in (1, 7):
    h = SM.empty_histogram(C, nbins, "cpu")
    _lib.lib().crn_eval_scores_cpu(pmf.data_ptr(), 0, gt.data_ptr(), None, B, C, C, D, H, W, 1, 0, nbins, h.table.data_ptr(),
                                   h.sq.data_ptr(), h.bad.data_ptr(), threads)
    hs.append(h)
  assert t.equal(hs[0].table, hs[1].table) and t.equal(hs[0].sq, hs[1].sq) and int(hs[0].bad) == int(hs[1].bad) == 0
  assert int(hs[0].table[..., 0].sum()) == (C + 1) * B * D * H * W


@pytest.mark.parametrize("C", [1, 2, 3, 14, 32])
def test_from_logits_equals_histogram_of_softmax_scores(SM, C):
  rng = np.random.default_rng(C)
  x = _t(SC.softmax_test_logits(rng, C, rows=512).reshape(2, 256, C).transpose(0, 2, 1).reshape(2, C, 4, 8, 8).copy())
  x[1, 0, 0, 0, 0] = math.nan                               # a NaN logit makes the voxel bad on both paths
  gt = _t(SC.random_gt(rng, 2, 4, 8, 8, 1, C))
  a = SM.score_histogram(x, gt, nbins=20, from_logits=True)
  b = SM.score_histogram(SM.softmax_scores(x), gt, nbins=20)
  assert t.equal(a.table, b.table) and t.equal(a.sq, b.sq) and int(a.bad) == int(b.bad) == 1


@pytest.mark.parametrize("C", [1, 2, 3, 14, 32])
def test_softmax_scores_against_float64(SM, C):
  x = SC.softmax_test_logits(np.random.default_rng(C), C)
  p = SM.softmax_scores(_t(x)).numpy()
  assert p.dtype == np.float32 and p.shape == x.shape
  err = float(np.abs(p.astype(np.float64) - SC.softmax64(x)).max())
  print("softmax_scores C", C, "largest absolute error", err, "bound", SOFTMAX_BOUND)
  assert err <= SOFTMAX_BOUND
  assert p.min() >= 0 and p.max() <= 1
  assert not ((p != 0) & (np.abs(p) < np.finfo(np.float32).tiny)).any()          # no denormal is produced
  assert np.array_equal(p[0], np.full_like(p[0], np.float32(1) / np.float32(C)))  # equal logits: exactly 1 / C
  if C > 1:
    assert p[4, 0, 0] == 1 and not p[4, 1:].any()           # a gap below -87: exact zeros
    assert p[3, 1:].all()                                   # a gap of exactly -87 is still positive


def test_known_answers(SM):
  # perfectly calibrated: ECE and MCE 0 in every row
  pmf, gt = SC.calibrated_pmf(nbins=4, per_bin=8)
  h = SM.score_histogram(_t(pmf), _t(gt), nbins=4)
  assert t.equal(SM.expected_calibration_error(h), t.zeros(3, dtype=t.float64))
  assert t.equal(SM.maximum_calibration_error(h), t.zeros(3, dtype=t.float64))
  r = SM.reliability(h)
  assert t.equal(r.count[1], t.full((4,), 8.0, dtype=t.float64))
  assert t.equal(r.confidence[1], t.tensor([0.125, 0.375, 0.625, 0.875], dtype=t.float64)) and t.equal(r.frequency, r.confidence)
  # all-0.5 predictor: Brier 0.25 exactly, whatever the labels
  gt = _t(np.random.default_rng(0).integers(0, 2, size=(1, 2, 3, 5)).astype(np.int32))
  h = SM.score_histogram(t.full((1, 2, 2, 3, 5), 0.5), gt, nbins=10)
  assert t.equal(SM.brier_score(h), t.full((3,), 0.25, dtype=t.float64))
  # separable: AP 1, best IoU 1 at the first threshold that separates 0.25 from 0.75
  pmf, gt = SC.separable_pmf()
  h = SM.score_histogram(_t(pmf), _t(gt), nbins=4)
  assert t.equal(SM.average_precision(h), t.ones(3, dtype=t.float64))
  thr, iou = SM.best_threshold(h)
  assert t.equal(thr, t.full((3,), 0.5, dtype=t.float64)) and t.equal(iou, t.ones(3, dtype=t.float64))
  c = SM.threshold_counts(h)
  assert c.tp[1].tolist() == [3, 3, 3, 3, 0] and c.fp[1].tolist() == [5, 5, 0, 0, 0] and c.fn[1].tolist() == [0, 0, 0, 0, 3]
  curve = SM.threshold_curve(h)
  assert curve.iou[1, :4].tolist() == [3 / 8, 3 / 8, 1.0, 1.0] and math.isnan(float(curve.iou[1, 4]))
  assert curve.recall[1, :4].tolist() == [1.0] * 4 and curve.precision[1, :2].tolist() == [3 / 8, 3 / 8]
  # a class that never occurs: no positives -> NaN AP and best threshold; a table without voxels -> NaN everywhere
  h = SM.score_histogram(_t(SC.random_pmf(np.random.default_rng(1), (1, 3, 1, 2, 3))), t.zeros((1, 1, 2, 3), dtype=t.int32))
  assert math.isnan(float(SM.average_precision(h)[1])) and math.isnan(float(SM.best_threshold(h)[0][2]))
  assert not math.isnan(float(SM.brier_score(h)[1])) and not math.isnan(float(SM.expected_calibration_error(h)[1]))
  empty = SM.empty_histogram(2, 5, "cpu")
  for f in (SM.expected_calibration_error, SM.maximum_calibration_error, SM.brier_score, SM.average_precision):
    assert bool(t.isnan(f(empty)).all())


def test_derived_quantities_against_direct_formulas(SM):
  """ECE, MCE, Brier, the threshold counts and AP of a random case, restated directly on the voxels in float64."""
  rng = np.random.default_rng(3)
  C, nbins = 3, 10
  pmf = SC.random_pmf(rng, (2, C, 3, 4, 5), sharp=1.5)
  gt = SC.random_gt(rng, 2, 3, 4, 5, 1, C)
  h = SM.score_histogram(_t(pmf), _t(gt), nbins=nbins)
  q = np.rint(pmf.astype(np.float64) * SC.Q_ONE).astype(np.int64)
  for r in range(C + 1):
    qr = (q[:, r] if r < C else SC.Q_ONE - q[:, 0]).reshape(-1)
    y = ((gt == r) if r < C else (gt != 0)).reshape(-1)
    bins = np.minimum(nbins - 1, (qr * nbins) >> 24)
    ece, mce = 0.0, 0.0
    for b in range(nbins):
      sel = bins == b
      if sel.any():
        gap = abs(qr[sel].mean() / SC.Q_ONE - y[sel].mean())
        ece += sel.mean() * gap
        mce = max(mce, gap)
    assert abs(float(SM.expected_calibration_error(h)[r]) - ece) <= 1e-12
    assert abs(float(SM.maximum_calibration_error(h)[r]) - mce) <= 1e-12
    brier = float(((qr / SC.Q_ONE - y) ** 2).mean())
    # e is rounded to 16 bits before it is squared: at most 2^-17 off, so e^2 at most 2^-16 off, plus 2^-25 for the shift
    assert abs(float(SM.brier_score(h)[r]) - brier) <= 2.0 ** -16 + 2.0 ** -25
    c = SM.threshold_counts(h)
    ap, prev_recall = 0.0, 0.0
    for j in range(nbins, -1, -1):
      pred = qr * nbins >= j * SC.Q_ONE if j < nbins else np.zeros_like(y)
      tp, fp, fn = int((pred & y).sum()), int((pred & ~y).sum()), int((~pred & y).sum())
      assert (int(c.tp[r, j]), int(c.fp[r, j]), int(c.fn[r, j])) == (tp, fp, fn)
      recall = tp / y.sum()
      ap += (recall - prev_recall) * (tp / (tp + fp) if tp else 0.0)
      prev_recall = recall
    assert abs(float(SM.average_precision(h)[r]) - ap) <= 1e-12


def test_value_errors(SM):
  f32 = lambda *s: t.zeros(s)
  i32 = lambda *s: t.zeros(s, dtype=t.int32)
  ok = dict(scores=f32(2, 3, 2, 3, 4), gt=i32(2, 2, 3, 4))
  SM.score_histogram(**ok)
  h = SM.empty_histogram(3, 20, "cpu")
  bad_calls = [
      dict(ok, scores=ok["scores"].double()), dict(ok, scores=f32(2, 3, 2, 3)), dict(ok, scores=f32(2, 33, 2, 3, 4)),
      dict(ok, scores=t.zeros((2, 3, 2, 3, 4), device="meta")), dict(ok, scores=f32(2, 3, 0, 3, 4), gt=i32(2, 0, 3, 4)),
      dict(ok, num_classes=65), dict(ok, num_classes=0), dict(ok, gt=None), dict(ok, gt=ok["gt"].long()),
      dict(ok, gt=i32(2, 2, 3, 5)), dict(ok, gt=i32(2, 4, 6, 8)[:, ::2, ::2, ::2]), dict(ok, m=0), dict(ok, m=2),
      dict(ok, scene_classes=i32(3)), dict(ok, scene_classes=t.zeros(2, dtype=t.int64)),
      dict(ok, nbins=0), dict(ok, nbins=257), dict(ok, num_classes=8, nbins=256), dict(ok, num_classes=64, nbins=32),
      dict(ok, offset_index=1), dict(ok, offset_index=-1), dict(ok, gt=i32(2, 4, 6, 8), m=2, offset_index=8),
      dict(ok, out=SM.empty_histogram(3, 10, "cpu")), dict(ok, out=SM.empty_histogram(4, 20, "cpu")),
      dict(ok, out=SM.ScoreHistogram(h.table.int(), h.sq, h.bad, 20)), dict(ok, out=SM.ScoreHistogram(h.table, h.sq[:, :1], h.bad, 20)),
      dict(ok, out=SM.ScoreHistogram(h.table, h.sq, t.zeros(1, dtype=t.int32), 20)),
  ]
  for kw in bad_calls:
    with pytest.raises(ValueError):
      SM.score_histogram(**kw)
  SM.score_histogram(**dict(ok, num_classes=7, nbins=256))
  SM.score_histogram(**dict(ok, gt=i32(2, 4, 6, 8), m=2, offset_index=7, out=h))
  for x in (f32(2, 3, 4).double(), f32(3), f32(2, 33, 4), f32(2, 0, 4), f32(2, 3, 0)):
    with pytest.raises(ValueError):
      SM.softmax_scores(x)
  assert SM.softmax_scores(f32(2, 3)).shape == (2, 3)
  assert SM.score_tiles()[1:] == (SM.MAX_ENTRIES, SM.MAX_NBINS) and SM.score_tiles()[0] >= 256


def test_rejected_calls_touch_nothing(SM):
  """CRN_EINVAL for every rule of the native entry point; the outputs keep their contents."""
  from corenet_amd import _lib
  L = _lib.lib()
  B, C, K, D, H, W, nbins = 2, 3, 3, 2, 3, 4, 20
  s, g, sc = t.rand(B, C, D, H, W), t.zeros((B, D, H, W), dtype=t.int32), t.ones(B, dtype=t.int32)
  h = SM.ScoreHistogram(t.full((K + 1, nbins, 2, 2), 5, dtype=t.int64), t.full((K + 1, 2), 6, dtype=t.int64),
                        t.full((1,), 7, dtype=t.int64), nbins)
  p = _lib.ptr

  def call(**kw):
    a = dict(scores=p(s), gt=p(g), B=B, C=C, K=K, D=D, H=H, W=W, m=1, n=0, nbins=nbins, table=p(h.table), sq=p(h.sq), bad=p(h.bad))
    a.update(kw)
    L.crn_eval_scores_cpu(a["scores"], 0, a["gt"], p(sc), a["B"], a["C"], a["K"], a["D"], a["H"], a["W"], a["m"], a["n"],
                          a["nbins"], a["table"], a["sq"], a["bad"], 1)
  for kw in (dict(scores=None), dict(gt=None), dict(table=None), dict(sq=None), dict(bad=None), dict(B=0), dict(C=0), dict(C=33),
             dict(K=0), dict(K=65), dict(D=0), dict(H=0), dict(W=0), dict(m=0), dict(n=-1), dict(n=1), dict(m=2, n=8),
             dict(nbins=0), dict(nbins=257), dict(K=8, nbins=256), dict(K=64, nbins=32), dict(D=1 << 30, H=1 << 30, W=1 << 30)):
    with pytest.raises(_lib.HipError):
      call(**kw)
  assert bool((h.table == 5).all()) and bool((h.sq == 6).all()) and int(h.bad) == 7
  out = t.full((B, C, 4), 9.0)
  for a in ((None, B, C, 4, p(out)), (p(s), B, C, 4, None), (p(s), 0, C, 4, p(out)), (p(s), B, 0, 4, p(out)),
            (p(s), B, 33, 4, p(out)), (p(s), B, C, 0, p(out)), (p(s), B, C, 1 << 62, p(out))):
    with pytest.raises(_lib.HipError):
      L.crn_score_softmax_cpu(*a, 1)
  assert bool((out == 9).all())
  call()
  assert int(h.table[..., 0].sum()) == 5 * h.table[..., 0].numel() + (C + 1) * B * D * H * W
