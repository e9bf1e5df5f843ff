"""Independent oracles and case builders for the label-overlap tests (numpy and plain Python, not shared with the
product).

  oracle_overlaps   the sparse overlap table of N grid pairs with np.unique over the stacked (a, b) columns, per grid.
  oracle_sizes      label histograms of one grid (np.bincount).
  oracle_match_pq   matching and panoptic counts of one grid pair with explicit loops over segment pairs.
  instance_arrays   a hand-made batch of multi-object scenes for the per-object evaluation.
  random_labels     random label grids with a given number of labels, in runs along W like real label grids or i.i.d.
"""
import numpy as np


def oracle_overlaps(a, b, num_a=None, num_b=None):
  """a, b: integer arrays [N, D, H, W].  -> (offsets [N + 1], a [P], b [P], count [P], num_a [N], num_b [N], bad [N]),
  pairs sorted by (grid, a, b); num_* default to the per-grid maximum clamped at 0."""
  a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
  N = a.shape[0]
  num_a = [max(int(a[n].max()), 0) for n in range(N)] if num_a is None else [int(v) for v in num_a]
  num_b = [max(int(b[n].max()), 0) for n in range(N)] if num_b is None else [int(v) for v in num_b]
  offsets, ia, ib, cnt, bad = [0], [], [], [], []
  for n in range(N):
    pairs = np.stack([a[n].reshape(-1), b[n].reshape(-1)])
    ok = (pairs[0] >= 0) & (pairs[0] <= num_a[n]) & (pairs[1] >= 0) & (pairs[1] <= num_b[n])
    bad.append(int((~ok).sum()))
    if ok.any():
      u, c = np.unique(pairs[:, ok], axis=1, return_counts=True)            # columns in lexicographic order
    else:
      u, c = np.zeros((2, 0), np.int64), np.zeros(0, np.int64)
    ia.append(u[0]), ib.append(u[1]), cnt.append(c)
    offsets.append(offsets[-1] + len(c))
  return (np.asarray(offsets, np.int64), np.concatenate(ia), np.concatenate(ib), np.concatenate(cnt).astype(np.int64),
          np.asarray(num_a, np.int64), np.asarray(num_b, np.int64), np.asarray(bad, np.int64))


def oracle_sizes(g, num):
  """Voxels per label 0 .. num of one grid; labels outside are dropped."""
  g = np.asarray(g).astype(np.int64).reshape(-1)
  return np.bincount(g[(g >= 0) & (g <= num)], minlength=num + 1)


def oracle_match_pq(a, b, num_a, num_b, class_a=None, class_b=None, thr=0.5, num_classes=1, min_voxels_a=0):
  """One grid pair [D, H, W] (every label within range).  class_a / class_b: sequences indexed by label (entry 0 unused)
  or None (all class 0).  -> dict with partner_a, iou_a, partner_b, iou_b, best_iou_b (lists indexed by label), size_a,
  size_b and tp, fp, fn, sum_iou (lists per class)."""
  a, b = np.asarray(a).astype(np.int64).copy(), np.asarray(b).astype(np.int64)
  size_a = [int((a == i).sum()) for i in range(num_a + 1)]
  if min_voxels_a > 0:
    for i in range(1, num_a + 1):
      if size_a[i] < min_voxels_a:
        a[a == i] = 0
    size_a = [int((a == i).sum()) for i in range(num_a + 1)]
  size_b = [int((b == j).sum()) for j in range(num_b + 1)]
  ca = [0] * (num_a + 1) if class_a is None else [int(v) for v in class_a]
  cb = [0] * (num_b + 1) if class_b is None else [int(v) for v in class_b]
  partner_a, iou_a = [0] * (num_a + 1), [0.0] * (num_a + 1)
  partner_b, iou_b, best_b = [0] * (num_b + 1), [0.0] * (num_b + 1), [0.0] * (num_b + 1)
  tp, fp, fn, sum_iou = [0] * num_classes, [0] * num_classes, [0] * num_classes, [0.0] * num_classes
  for j in range(1, num_b + 1):
    for i in range(1, num_a + 1):
      if size_a[i] == 0 or ca[i] != cb[j]:
        continue
      c = int(((a == i) & (b == j)).sum())
      if c == 0:
        continue
      iou = c / (size_a[i] + size_b[j] - c)
      best_b[j] = max(best_b[j], iou)
      if iou > thr:
        assert partner_b[j] == 0 and partner_a[i] == 0
        partner_a[i], iou_a[i], partner_b[j], iou_b[j] = j, iou, i, iou
  for j in range(1, num_b + 1):
    if partner_b[j]:
      tp[cb[j]] += 1
      sum_iou[cb[j]] += iou_b[j]
    else:
      fn[cb[j]] += 1
  for i in range(1, num_a + 1):
    if size_a[i] > 0 and not partner_a[i]:
      fp[ca[i]] += 1
  return dict(partner_a=partner_a, iou_a=iou_a, partner_b=partner_b, iou_b=iou_b, best_iou_b=best_b, size_a=size_a,
              size_b=size_b, tp=tp, fp=fp, fn=fn, sum_iou=sum_iou)


def random_labels(rng, shape, num_labels, dtype=np.int32, runs=True, background=0.0):
  """A grid `shape` (any rank) with labels 0 .. num_labels.  runs: constant pieces of random length along the last
  axis (what a lane of the kernel merges), else i.i.d. voxels.  background: the fraction set to 0 afterwards."""
  size = int(np.prod(shape))
  if runs:
    lengths = rng.integers(1, 9, size=size)
    values = rng.integers(0, num_labels + 1, size=size)
    g = np.repeat(values, lengths)[:size]
  else:
    g = rng.integers(0, num_labels + 1, size=size)
  if background > 0:
    g = np.where(rng.random(size) < background, 0, g)
  return g.reshape(shape).astype(dtype)


def blobs(rng, shape, count, radius, dtype=np.int32):
  """A grid [D, H, W] with `count` axis-aligned boxes of half extent <= radius, box k labelled k + 1 (later boxes
  overwrite earlier ones): objects for the matching tests."""
  D, H, W = shape
  g = np.zeros(shape, dtype)
  for k in range(count):
    c = [int(rng.integers(0, s)) for s in shape]
    r = [int(rng.integers(1, radius + 1)) for _ in shape]
    g[max(c[0] - r[0], 0):c[0] + r[0], max(c[1] - r[1], 0):c[1] + r[1], max(c[2] - r[2], 0):c[2] + r[2]] = k + 1
  return g


def instance_arrays(seed, B=2, shape=(10, 12, 14), C=4):
  """A hand-made multi-object batch: (semantic grid [B, D, H, W], per scene the classes of its meshes in 1 .. C - 1,
  instance grid = mesh index + 1).  The last mesh of every scene leaves no voxel."""
  rng = np.random.default_rng(seed)
  meshes = [int(rng.integers(3, 6)) for _ in range(B)]
  inst = np.stack([blobs(rng, shape, m - 1, 4) for m in meshes])
  labels = [rng.integers(1, C, m).astype(np.int32) for m in meshes]
  sem = np.zeros_like(inst)
  for b in range(B):
    sem[b] = np.concatenate([[0], labels[b]])[inst[b]]
  return sem, labels, inst
