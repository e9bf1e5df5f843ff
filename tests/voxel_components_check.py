"""Independent oracle and case builders for the voxel-component tests (not shared with the product).

oracle_label is a plain numpy / Python flood fill that visits the foreground voxels in raster order, so its numbering is
raster-first by construction; it also recomputes size / bbox / first / value.  Used only on grids of at most 24^3.
"""
import itertools

import numpy as np

ORACLE_MAX_VOXELS = 24 ** 3


def offsets(connectivity):
  level = {6: 1, 18: 2, 26: 3}[connectivity]
  return [o for o in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(c != 0 for c in o) <= level]


def foreground_keys(grid, by_value):
  """int64 keys: 0 on background (value <= 0 or NaN), else the value (by_value) or 1.  bool and floating grids have the
  single value 1 (the wrapper's conversion)."""
  g = np.asarray(grid)
  if g.dtype == np.bool_ or np.issubdtype(g.dtype, np.floating):
    with np.errstate(invalid="ignore"):
      return (g > 0).astype(np.int64)
  g = g.astype(np.int64)
  return np.where(g > 0, g if by_value else 1, 0)


def oracle_label(grid, connectivity=6, by_value=True):
  """grid [D, H, W] -> (labels int32 [D, H, W], K, stats dict of arrays size / bbox / first / value)."""
  key = foreground_keys(grid, by_value)
  D, H, W = key.shape
  assert D * H * W <= ORACLE_MAX_VOXELS
  offs = offsets(connectivity)
  labels = np.zeros((D, H, W), np.int32)
  size, bbox, first, value = [], [], [], []
  K = 0
  for d in range(D):
    for h in range(H):
      for w in range(W):
        k = key[d, h, w]
        if k == 0 or labels[d, h, w]:
          continue
        K += 1
        labels[d, h, w] = K
        stack = [(d, h, w)]
        members = []
        while stack:
          a, b, c = stack.pop()
          members.append((a, b, c))
          for da, db, dc in offs:
            e, f, g = a + da, b + db, c + dc
            if 0 <= e < D and 0 <= f < H and 0 <= g < W and key[e, f, g] == k and not labels[e, f, g]:
              labels[e, f, g] = K
              stack.append((e, f, g))
        m = np.array(members)
        size.append(len(members))
        bbox.append(list(m.min(0)) + list(m.max(0) + 1))
        first.append((d * H + h) * W + w)
        value.append(k)
  stats = dict(size=np.array(size, np.int64), bbox=np.array(bbox, np.int32).reshape(-1, 6), first=np.array(first, np.int64),
               value=np.array(value, np.int32))
  return labels, K, stats


def random_grid(rng, shape, density, classes, dtype=np.int32):
  g = (rng.random(shape) < density) * rng.integers(1, classes + 1, shape)
  return g.astype(dtype)


def checkerboard(shape, dtype=np.uint8):
  d, h, w = np.indices(shape)
  return ((d + h + w) % 2 == 0).astype(dtype)


def serpentine(shape, dtype=np.uint8):
  """One 1-voxel-wide path through the whole grid: every other row of every other plane is filled, consecutive rows are
  joined at alternating ends, consecutive planes at alternating corners.  One component at every connectivity."""
  D, H, W = shape
  plane = np.zeros((H, W), dtype)
  rows = list(range(0, H, 2))
  for i, h in enumerate(rows):
    plane[h, :] = 1
    if i + 1 < len(rows):
      plane[h + 1, W - 1 if i % 2 == 0 else 0] = 1
  start, end = (0, 0), (rows[-1], W - 1 if (len(rows) - 1) % 2 == 0 else 0)
  g = np.zeros(shape, dtype)
  for d in range(0, D, 2):                                             # the same path in every other plane, walked
    g[d] = plane                                                       # forwards and backwards in turn
    if d + 2 < D:
      g[(d + 1,) + (end if (d // 2) % 2 == 0 else start)] = 1
  return g


def u_across_seam(shape, axis, brick):
  """A "U": two arms along `axis` inside brick A (indices below brick[axis]), two voxels apart, joined only by a bar in
  brick B just behind the seam.  The grid's lowest index is at the far end of the first arm, so the second arm learns
  its final root only through two seam crossings: a brick-local labelling followed by a one-step seam fix gets this
  wrong.  One component at every connectivity."""
  g = np.zeros(shape, np.uint8)
  b = brick[axis]
  side = [a for a in range(3) if a != axis][0]                         # the arms sit at 0 and 2 along this axis
  assert shape[axis] > b and shape[side] > 2

  def put(along, across):
    sl = [0, 0, 0]
    sl[axis], sl[side] = along, across
    g[tuple(sl)] = 1

  put(slice(0, b), 0)                                                  # the first arm: from index 0 to the seam
  put(slice(b - 3, b), 2)                                              # the second arm: short
  put(b, slice(0, 3))                                                  # the bar, in brick B
  return g
