"""Independent oracles and case builders for the voxel-visibility tests (not shared with the product).

  brute             the definition itself: for every pair (v, u) the open t-interval in which the segment from the centre
                    of v to the eye lies inside the open cube of u, intersected with (0, 1), in exact rationals (integer
                    numerators and denominators, compared by cross-multiplication).  No walk, no tie rule.
  dda               the three-axis integer walk in Python integers (unbounded, so no term can overflow).
  eyes_for          eyes of every kind for a grid shape, in float voxel coordinates.
Random grids and the sparse label fixture come from voxel_distance_check.
"""
from fractions import Fraction

import numpy as np

from voxel_distance_check import fixture_grids, foreground_of, random_grid   # noqa: F401  (re-exported for the tests)

SUB = 256
MAX_EYE = 1 << 19


def quantise(eye):
  """int [3]: round(eye * 256) in float64, half to even (numpy's rint)."""
  return [int(v) for v in np.rint(np.asarray(eye, np.float64) * SUB)]


def brute(occupied, eye_q):
  """(occluded bool [D, H, W], first int64 [D, H, W]) of one grid straight from the definition."""
  D, H, W = occupied.shape
  zz, yy, xx = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
  u = np.stack([xx, yy, zz], -1).reshape(-1, 3).astype(np.int64)          # raster order: row i is linear index i
  occ = occupied.reshape(-1)
  e = np.asarray(eye_q, np.int64)
  occluded = np.zeros(len(u), bool)
  first = np.full(len(u), -1, np.int64)
  for i, v in enumerate(u):
    c = v * SUB + SUB // 2
    delta = e - c
    lo_n, lo_d = np.zeros(len(u), np.int64), np.ones(len(u), np.int64)    # the running max of the lower bounds: 0
    hi_n, hi_d = np.ones(len(u), np.int64), np.ones(len(u), np.int64)     # the running min of the upper bounds: 1
    ok = np.ones(len(u), bool)
    for a in range(3):
      lo, hi = u[:, a] * SUB - c[a], u[:, a] * SUB + SUB - c[a]           # the cube's faces relative to the centre of v
      if delta[a] == 0:
        ok &= (lo < 0) & (hi > 0)
        continue
      d = abs(int(delta[a]))
      n0, n1 = (lo, hi) if delta[a] > 0 else (-hi, -lo)                   # t in (n0 / d, n1 / d)
      up = n0 * lo_d > lo_n * d
      lo_n, lo_d = np.where(up, n0, lo_n), np.where(up, d, lo_d)
      down = n1 * hi_d < hi_n * d
      hi_n, hi_d = np.where(down, n1, hi_n), np.where(down, d, hi_d)
    ok &= lo_n * hi_d < hi_n * lo_d                                       # a non-empty open interval
    ok[i] = False                                                         # u != v
    hits = np.nonzero(ok & occ)[0]
    if len(hits):
      occluded[i] = True
      first[i] = max(hits, key=lambda j: Fraction(int(lo_n[j]), int(lo_d[j])))   # entered last: nearest the eye
  return occluded.reshape(D, H, W), first.reshape(D, H, W)


def dda(occupied, eye_q, count=False):
  """The same two arrays by the integer walk, in Python integers; with count the trip counts instead of first."""
  D, H, W = occupied.shape
  ext = (W, H, D)
  occluded = np.zeros((D, H, W), bool)
  first = np.full((D, H, W), -1, np.int64)
  for z in range(D):
    for y in range(H):
      for x in range(W):
        pos = [x, y, z]
        delta = [int(eye_q[a]) - (pos[a] * SUB + SUB // 2) for a in range(3)]
        act = [a for a in range(3) if delta[a]]
        t_end = 1
        for a in act:
          t_end *= abs(delta[a])
        T, inc = {}, {}
        for a in act:
          others = t_end // abs(delta[a])
          T[a], inc[a] = (SUB // 2) * others, SUB * others
        last, steps = -1, 0
        while act:
          m = min(T.values())
          if m >= t_end:
            break
          for a in act:
            if T[a] == m:
              pos[a] += 1 if delta[a] > 0 else -1
              T[a] += inc[a]
          if any(not 0 <= pos[a] < ext[a] for a in range(3)):
            break
          steps += 1
          if occupied[pos[2], pos[1], pos[0]]:
            last = (pos[2] * H + pos[1]) * W + pos[0]
        occluded[z, y, x] = last >= 0
        first[z, y, x] = steps if count else last
  return occluded, first


def eyes_for(shape, rng):
  """{kind: eye (x, y, z) in float voxel coordinates} for a grid [D, H, W]: on the centre lattice (segments through
  edges and corners), on the corner lattice, generic, inside the grid, and equal to a voxel centre."""
  D, H, W = shape
  ext = np.array([W, H, D], np.float64)
  out = {
      "centre lattice": np.array([W + 1.5, -2.5, D + 0.5]),
      "centre lattice, one axis shared": np.array([0.5, H + 2.5, -1.5]),
      "corner lattice": np.array([-2.0, H + 1.0, -3.0]),
      "generic": ext / 2 + (rng.random(3) - 0.5) * 4 * ext + np.array([0.0, 0.0, -3.0 * D]),
      "inside": rng.random(3) * ext,
      "voxel centre": np.floor(rng.random(3) * ext) + 0.5,
  }
  return out
