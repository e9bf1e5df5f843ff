"""Independent oracle and case builders for the voxel-distance tests (not shared with the product), numpy int64.

  targets_of        the three target rules.
  brute_d2          min over the LIST of target voxels of |v - u|^2, no separability assumed.
  recurrence        the separable recurrence that defines the index, each pass a brute force over the whole line with
                    argmin's first-minimum rule (ties to the lower w / j).
"""
import numpy as np

NO_TARGET = (1 << 31) - 1
BIG = 1 << 40                     # "no target" inside the oracle: above every real value, never added up to overflow
MODES = ("foreground", "background", "surface")


def foreground_of(grid):
  g = np.asarray(grid)
  with np.errstate(invalid="ignore"):
    return g > 0                  # NaN > 0 is False


def targets_of(grid, mode):
  """bool [D, H, W]: the target set of a grid [D, H, W]."""
  fg = foreground_of(grid)
  if mode == "foreground":
    return fg
  if mode == "background":
    return ~fg
  assert mode == "surface"
  p = np.pad(fg, 1, constant_values=False)          # outside the grid is not foreground
  inner = (p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] &
           p[1:-1, 1:-1, 2:])
  return fg & ~inner


def brute_d2(target, chunk=1 << 22):
  """int64 [D, H, W]: the squared distance to the nearest target voxel, NO_TARGET when there is none."""
  D, H, W = target.shape
  u = np.argwhere(target).astype(np.int64)          # [T, 3]
  if len(u) == 0:
    return np.full((D, H, W), NO_TARGET, np.int64)
  v = np.stack(np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
  out = np.empty(len(v), np.int64)
  step = max(1, chunk // len(u))
  for s in range(0, len(v), step):
    diff = v[s:s + step, None, :] - u[None, :, :]
    out[s:s + step] = (diff * diff).sum(-1).min(1)
  return out.reshape(D, H, W)


def _line_pass(g, idx, axis, scale):
  """out[i] = min_j g[j] + (i - j)^2 along axis, the first minimum wins; idx: j * scale + idx[j]."""
  L = g.shape[axis]
  g = np.moveaxis(g, axis, -1)
  idx = np.moveaxis(idx, axis, -1)
  i = np.arange(L, dtype=np.int64)
  cand = g[..., None, :] + (i[:, None] - i[None, :]) ** 2            # [..., i, j]
  j = cand.argmin(-1)                                                # first minimum: the lower j
  val = np.take_along_axis(cand, j[..., None], -1)[..., 0]
  win = np.take_along_axis(idx, j, -1) + j * scale
  none = val >= BIG
  val = np.where(none, BIG, val)
  win = np.where(none, -1, win)
  return np.moveaxis(val, -1, axis), np.moveaxis(win, -1, axis)


def recurrence(target):
  """(d2 int64 [D, H, W], index int64 [D, H, W]) by the separable recurrence; NO_TARGET / -1 without a target."""
  D, H, W = target.shape
  w = np.arange(W, dtype=np.int64)
  cand = np.where(target[..., None, :], (w[:, None] - w[None, :]) ** 2, BIG)          # [D, H, w, u]
  j = cand.argmin(-1)
  g = np.take_along_axis(cand, j[..., None], -1)[..., 0]
  idx = np.where(g >= BIG, -1, j)
  g, idx = _line_pass(g, idx, 1, W)
  g, idx = _line_pass(g, idx, 0, H * W)
  return np.where(g >= BIG, NO_TARGET, g), idx


def check_index(target, d2, index):
  """index points at a target voxel at exactly d2 (or is -1 where d2 is NO_TARGET)."""
  D, H, W = target.shape
  d2, index = np.asarray(d2, np.int64), np.asarray(index, np.int64)
  if not target.any():
    assert (d2 == NO_TARGET).all() and (index == -1).all()
    return
  assert index.min() >= 0 and index.max() < D * H * W
  ud, uh, uw = np.unravel_index(index, (D, H, W))
  assert target[ud, uh, uw].all()
  vd, vh, vw = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
  assert np.array_equal((vd - ud) ** 2 + (vh - uh) ** 2 + (vw - uw) ** 2, d2)


def random_grid(rng, shape, density, dtype=np.uint8):
  """A grid [D, H, W] with about `density` foreground: uint8 / int32 carry values 1 .. 3 (int32 also negative
  background), bool is a mask, floating grids carry NaN and negative values on the background."""
  fg = rng.random(shape) < density
  if dtype == np.bool_:
    return fg
  if np.issubdtype(dtype, np.floating):
    bg = rng.choice(np.array([0.0, -1.5, np.nan], dtype), size=shape)
    return np.where(fg, rng.random(shape).astype(dtype) + dtype(0.25), bg).astype(dtype)
  val = rng.integers(1, 4, size=shape)
  bg = rng.integers(-2, 1, size=shape) if dtype == np.int32 else 0
  return np.where(fg, val, bg).astype(dtype)


def ball(shape, centre, radius):
  d, h, w = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
  return ((d - centre[0]) ** 2 + (h - centre[1]) ** 2 + (w - centre[2]) ** 2 <= radius * radius).astype(np.uint8)


def fixture_grids(n, side, seed):
  """n sparse label grids of side^3 in the style of the components benchmark: a few boxes and balls plus specks."""
  rng = np.random.default_rng(seed)
  out = np.zeros((n, side, side, side), np.int32)
  for g in out:
    for k in range(6):
      c = rng.integers(side // 8, side - side // 8, size=3)
      r = int(rng.integers(2, max(3, side // 16)))
      sl = tuple(slice(max(0, int(x) - r), int(x) + r) for x in c)
      if k % 2:
        g[sl] = k + 1
      else:
        sub = ball(tuple(s.stop - s.start for s in sl), (r, r, r), r - 0.5)
        g[sl] = np.where(sub > 0, k + 1, g[sl])
    speck = rng.random(g.shape) < 2e-4
    g[speck] = 7
  return out
