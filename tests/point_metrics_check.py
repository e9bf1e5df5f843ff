"""Independent restatements and shared inputs for the surface-metric tests (test_point_metrics_cpu.py / _gpu.py): plain
numpy, float32 elementwise in the order the contract states (corenet_amd/mesh_metrics.py), so equality is exact."""
import functools

import numpy as np

# (queries, candidates) per object: below / at / above the wave (64) and tile sizes, an empty object between two
# non-empty ones, and one object larger than one query tile of the kernel would be with fewer queries per lane
NEAREST_SIZES = [(1, 1), (63, 65), (64, 64), (0, 0), (65, 257), (1000, 777)]


def offsets(counts):
  return np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))]).astype(np.int64)


def np_nearest(a, a_off, b, b_off):
  """(dist2 f32 [Na], index i32 [Na]): float32 d2 = (dx*dx + dy*dy) + dz*dz, the first minimum among the candidates
  whose d2 is not NaN; none: +inf and -1."""
  a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
  dist2 = np.full(a.shape[0], np.inf, np.float32)
  index = np.full(a.shape[0], -1, np.int32)
  for n in range(len(a_off) - 1):
    qa, cb = a[a_off[n]:a_off[n + 1]], b[b_off[n]:b_off[n + 1]]
    if not len(qa) or not len(cb):
      continue
    with np.errstate(invalid="ignore", over="ignore"):
      dx = qa[:, None, 0] - cb[None, :, 0]
      dy = qa[:, None, 1] - cb[None, :, 1]
      dz = qa[:, None, 2] - cb[None, :, 2]
      d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    ok = ~np.isnan(d2)
    key = np.where(ok, d2, np.inf)
    first = np.argmin(key, axis=1)                       # argmin: the first minimum, the contract's tie rule
    m = key[np.arange(len(qa)), first]
    hit = ok & (key == m[:, None])                       # where the row minimum is +inf only real candidates count
    any_hit = hit.any(1)
    idx = np.where(any_hit, hit.argmax(1), -1)
    dist2[a_off[n]:a_off[n + 1]] = np.where(any_hit, m, np.inf)
    index[a_off[n]:a_off[n + 1]] = idx
  return dist2, index


@functools.lru_cache(maxsize=None)
def nearest_case(kind):
  """(a, a_off, b, b_off, dist2, index) as numpy arrays, the reference computed once.  kind: 'sizes' (random
  coordinates), 'ties' (coordinates on a grid of 1/8 in [-1, 1] with duplicated candidates), 'nan' (a NaN candidate and a
  NaN query among valid ones)."""
  rng = np.random.RandomState({"sizes": 1, "ties": 2, "nan": 3}[kind])
  na, nb = [s[0] for s in NEAREST_SIZES], [s[1] for s in NEAREST_SIZES]
  a_off, b_off = offsets(na), offsets(nb)
  if kind == "ties":
    a = (rng.randint(-8, 9, (a_off[-1], 3)) / 8.0).astype(np.float32)
    b = (rng.randint(-8, 9, (b_off[-1], 3)) / 8.0).astype(np.float32)
    for n in range(len(na)):                             # the second half of every object's candidates repeats the first
      h = nb[n] // 2
      b[b_off[n] + h:b_off[n] + 2 * h] = b[b_off[n]:b_off[n] + h]
  else:
    a = (rng.rand(a_off[-1], 3).astype(np.float32) * 2 - 1)
    b = (rng.rand(b_off[-1], 3).astype(np.float32) * 2 - 1)
  if kind == "nan":
    for n in (1, 4, 5):
      b[b_off[n] + 3, 1] = np.nan
      b[b_off[n + 1] - 1, 0] = np.nan
      a[a_off[n] + 5, 2] = np.nan
    b[b_off[0], 0] = np.nan                              # the only candidate of object 0: its query finds nothing
  d2, idx = np_nearest(a, a_off, b, b_off)
  for x in (a, a_off, b, b_off, d2, idx):
    x.setflags(write=False)
  return a, a_off, b, b_off, d2, idx


def decade_mesh(seed=0, T=50):
  """T right triangles f32 [T, 3, 3] whose areas span three decades, shuffled, each at its own place and orientation."""
  rng = np.random.RandomState(seed)
  side = 10.0 ** (-1.5 * np.arange(T) / (T - 1))         # area = side^2 / 2: 1 ... 1e-3 of the largest
  rng.shuffle(side)
  tri = np.zeros((T, 3, 3), np.float64)
  for k in range(T):
    q, _ = np.linalg.qr(rng.randn(3, 3))
    p = rng.rand(3) * 2 - 1
    tri[k] = [p, p + side[k] * q[0], p + side[k] * q[1]]
  return tri.astype(np.float32)


def areas64(tri):
  t = np.asarray(tri, np.float64)
  return 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)


def sampling_soup():
  """(triangles f32 [T, 3, 3], counts): five objects -- a random mesh, the decade mesh with zero-area and NaN triangles
  mixed in, an empty object, an all-degenerate object, a single triangle."""
  rng = np.random.RandomState(5)
  rand = (rng.rand(200, 3, 3) * 2 - 1).astype(np.float32)
  dec = decade_mesh(1)
  bad = np.zeros((4, 3, 3), np.float32)
  bad[0] = 0.25                                          # a point
  bad[1] = [[0, 0, 0], [1, 1, 1], [2, 2, 2]]             # collinear
  bad[2] = [[0, 0, 0], [1, 0, 0], [np.nan, 1, 0]]        # NaN
  bad[3] = [[0, 0, 0], [3e38, 0, 0], [0, 3e38, 0]]       # infinite area
  mixed = np.concatenate([dec[:20], bad[:2], dec[20:], bad[2:]])
  one = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)
  tri = np.concatenate([rand, mixed, bad, one]).astype(np.float32)
  return tri, [len(rand), len(mixed), 0, len(bad), 1]


def unit_square(z):
  return np.array([[[0, 0, z], [1, 0, z], [1, 1, z]], [[0, 0, z], [1, 1, z], [0, 1, z]]], np.float32)
