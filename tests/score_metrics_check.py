"""An independent reference for corenet_amd.score_metrics, exact by construction: from a float32 pmf it forms q by
round-half-even in float64 (p * 2^24 is exact there) and the bins and sums in Python / int64 integers.  Also a float64
softmax, the input generators and the known-answer cases the score tests share."""
import numpy as np

Q_ONE = 1 << 24


def offsets_of(n, m):
  return n % m, (n // m) % m, n // (m * m)           # ix, iy, iz


def reference_histogram(pmf, gt, K, nbins, scene=None, m=1, n=0):
  """(table int64 [K+1, nbins, 2, 2], sq int64 [K+1, 2], bad int) of a float32 pmf [B, C, D, H, W] against gt
  [B, mD, mH, mW], by the issue's rules, one voxel at a time."""
  pmf = np.asarray(pmf, dtype=np.float32)
  B, C, D, H, W = pmf.shape
  ix, iy, iz = offsets_of(n, m)
  table = np.zeros((K + 1, nbins, 2, 2), dtype=np.int64)
  sq = np.zeros((K + 1, 2), dtype=np.int64)
  bad = 0
  p64 = pmf.astype(np.float64)
  with np.errstate(invalid="ignore"):
    fine = (p64 >= 0) & (p64 <= 1)                   # False for a NaN
    q_all = np.where(fine, np.rint(np.where(fine, p64, 0.0) * Q_ONE), 0).astype(np.int64)
  ok_all = fine.all(axis=1)
  sub = gt[:, iz::m, iy::m, ix::m]
  assert sub.shape == (B, D, H, W)

  def entry(row, q, y):
    b = min(nbins - 1, (q * nbins) >> 24)
    table[row, b, y, 0] += 1
    table[row, b, y, 1] += q
    e = Q_ONE - q if y else q
    e16 = (e + 128) >> 8
    sq[row, y] += (e16 * e16 + 128) >> 8

  for b in range(B):
    s = 1 if scene is None else int(scene[b])
    if s < 1 or (C - 1) * s >= K:
      bad += D * H * W
      continue
    for z, y, x in np.ndindex(D, H, W):
      g = int(sub[b, z, y, x]) * s
      if not 0 <= g < K or not ok_all[b, z, y, x]:
        bad += 1
        continue
      qs = [int(v) for v in q_all[b, :, z, y, x]]
      for c in range(C):
        entry(c * s, qs[c], int(g == c * s))
      entry(K, Q_ONE - qs[0], int(g != 0))
  return table, sq, bad


def softmax64(logits):
  """float64 softmax over axis 1."""
  x = np.asarray(logits, dtype=np.float64)
  e = np.exp(x - x.max(axis=1, keepdims=True))
  return e / e.sum(axis=1, keepdims=True)


def random_pmf(rng, shape, sharp=3.0):
  """A float32 pmf [B, C, D, H, W] whose every score is inside [0, 1] (each is a float32 quotient e / sum <= 1)."""
  x = rng.standard_normal(shape) * sharp
  p = softmax64(x).astype(np.float32)
  return np.clip(p, 0.0, 1.0)


def random_gt(rng, B, D, H, W, m, K, scene=None):
  """int32 [B, mD, mH, mW] labels: with scene classes, 0 or 1 (scaled by the scene class by the code under test)."""
  hi = 2 if scene is not None else K
  return rng.integers(0, hi, size=(B, m * D, m * H, m * W)).astype(np.int32)


def softmax_test_logits(rng, C, rows=4096):
  """[rows, C, 1] float32 logits spanning +-30, with rows of equal logits and rows with a gap of 87 or more."""
  x = (rng.random((rows, C, 1)) * 60 - 30).astype(np.float32)
  x[0] = 0.0
  x[1] = 30.0
  x[2] = -30.0
  if C > 1:
    x[3, 0] = 30.0; x[3, 1:] = -57.0                 # a gap of exactly 87
    x[4, 0] = 30.0; x[4, 1:] = -57.5                 # below -87: exact zeros
    x[5, -1] = 29.0; x[5, :-1] = -60.0
    x[6] = -30.0; x[6, C // 2] = 30.0
    x[7:40, 0] = 0.0                                  # small gaps around 0
    x[7:40, 1:] = (rng.random((33, C - 1, 1)) * 2e-3 - 1e-3).astype(np.float32)
  return x


def calibrated_pmf(nbins=4, per_bin=8):
  """A two-class case whose table is perfectly calibrated: in bin j of class 1 all scores are (2j+1) / (2 nbins)
  (exact in float32 for nbins a power of two) and exactly that fraction of the voxels is positive.  Returns
  (pmf [1, 2, 1, 1, W], gt [1, 1, 1, W]); needs per_bin divisible by 2 * nbins."""
  assert per_bin % (2 * nbins) == 0
  p1, g = [], []
  for j in range(nbins):
    conf = (2 * j + 1) / (2 * nbins)
    npos = per_bin * (2 * j + 1) // (2 * nbins)
    p1 += [conf] * per_bin
    g += [1] * npos + [0] * (per_bin - npos)
  p1 = np.asarray(p1, dtype=np.float32)
  pmf = np.stack([1 - p1, p1])[None, :, None, None, :]
  return pmf.astype(np.float32), np.asarray(g, dtype=np.int32)[None, None, None, :]


def separable_pmf():
  """Class 1 positives all score 0.75, negatives all 0.25: AP 1, best IoU 1 at the first threshold that separates
  them.  Returns (pmf [1, 2, 1, 1, 8], gt [1, 1, 1, 8])."""
  g = np.asarray([0, 0, 0, 0, 0, 1, 1, 1], dtype=np.int32)
  p1 = np.where(g == 1, 0.75, 0.25).astype(np.float32)
  pmf = np.stack([1 - p1, p1])[None, :, None, None, :]
  return pmf.astype(np.float32), g[None, None, None, :]
