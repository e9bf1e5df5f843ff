"""Independent numpy references for corenet_amd.voxel_topology; none of them uses the configuration
histogram's look-up tables:
  * the table by eight shifted slices of the zero-padded mask plus np.bincount,
  * the Euler characteristic under 26- and 6-connectivity by counting the cells of the two complexes directly,
  * Betti numbers with scipy.ndimage.label on the padded mask and its complement,
  * the shapes with known topology and random label grids."""
import numpy as np

CROFTON = (2 * 0.04577789120476, 2 * 0.03698062787608, 2 * 0.03519563978232)


def masks_of(grid, num_labels, mask_grid=False):
  """(bool [L + 1, D, H, W], bad count) of one grid: row 0 any valid label, row l the label l."""
  grid = np.asarray(grid)
  if mask_grid:
    return (grid > 0)[None], 0
  g = grid.astype(np.int64)
  bad = (g < 0) | (g > num_labels)
  g = np.where(bad, 0, g)
  return np.stack([g != 0] + [g == l for l in range(1, num_labels + 1)]), int(bad.sum())


def code_volume(mask):
  """int64 [D + 1, H + 1, W + 1]: the code of every cell of a bool mask."""
  p = np.pad(np.asarray(mask, dtype=bool), 1).astype(np.int64)
  D, H, W = mask.shape
  code = np.zeros((D + 1, H + 1, W + 1), dtype=np.int64)
  for i in (0, 1):
    for j in (0, 1):
      for k in (0, 1):
        code |= p[i:i + D + 1, j:j + H + 1, k:k + W + 1] << (4 * i + 2 * j + k)
  return code


def table_of(grids, num_labels, mask_grid=False):
  """(table int64 [N, L + 1, 256], bad int64 [N]) of grids [N, D, H, W]."""
  tables, bads = [], []
  for g in grids:
    masks, bad = masks_of(g, num_labels, mask_grid)
    tables.append(np.stack([np.bincount(code_volume(m).reshape(-1), minlength=256) for m in masks]))
    bads.append(bad)
  L1 = 1 if mask_grid else num_labels + 1
  return (np.stack(tables).astype(np.int64) if tables else np.zeros((0, L1, 256), np.int64)), np.asarray(bads, dtype=np.int64)


def volume_of(mask):
  return int(np.asarray(mask, dtype=bool).sum())


def exposed_faces_of(mask):
  p = np.pad(np.asarray(mask, dtype=bool), 1)
  return int(sum((np.diff(p.astype(np.int8), axis=a) != 0).sum() for a in range(3)))


def chi26_of(mask):
  """V - E + F - C of the union of closed unit cubes."""
  p = np.pad(np.asarray(mask, dtype=bool), 1)
  def closure(axes):                                                         # the cells of lower dimension a voxel touches along `axes`
    q = p
    for a in axes:
      s = [slice(None)] * 3
      lo, hi = list(s), list(s)
      lo[a], hi[a] = slice(0, -1), slice(1, None)
      q = q[tuple(lo)] | q[tuple(hi)]
    return int(q.sum())
  cubes = closure(())
  faces = sum(closure((a,)) for a in range(3))
  edges = sum(closure(ax) for ax in ((0, 1), (0, 2), (1, 2)))
  verts = closure((0, 1, 2))
  return verts - edges + faces - cubes


def chi6_of(mask):
  """V - E + F - C of the complex of voxel centres, 6-adjacent pairs, full 2x2 squares and full 2x2x2 blocks."""
  p = np.asarray(mask, dtype=bool)
  def full(axes):
    q = p
    for a in axes:
      s = [slice(None)] * 3
      lo, hi = list(s), list(s)
      lo[a], hi[a] = slice(0, -1), slice(1, None)
      q = q[tuple(lo)] & q[tuple(hi)]
    return int(q.sum())
  return full(()) - sum(full((a,)) for a in range(3)) + sum(full(ax) for ax in ((0, 1), (0, 2), (1, 2))) - full((0, 1, 2))


def betti_of(mask, connectivity):
  """(b0, b1, b2, chi) with scipy.ndimage.label; the complement is labelled with the dual connectivity."""
  from scipy import ndimage
  s6, s26 = ndimage.generate_binary_structure(3, 1), ndimage.generate_binary_structure(3, 3)
  fg, bg = (s26, s6) if connectivity == 26 else (s6, s26)
  p = np.pad(np.asarray(mask, dtype=bool), 1)
  b0 = ndimage.label(p, structure=fg)[1]
  b2 = ndimage.label(~p, structure=bg)[1] - 1
  chi = chi26_of(mask) if connectivity == 26 else chi6_of(mask)
  return b0, b0 + b2 - chi, b2, chi


def crofton_of(table_row, voxel_size=1.0):
  """The area formula on one row of a reference table, with pair counts taken from the codes directly."""
  c1, c2, c3 = CROFTON
  n = [0, 0, 0]
  for code in range(1, 255):
    if not table_row[code]:
      continue
    b = [(code >> q) & 1 for q in range(8)]
    for x in range(8):
      for y in range(x + 1, 8):
        kind = bin(x ^ y).count("1")                                         # 1 axis, 2 face diagonal, 3 body diagonal
        n[kind - 1] += int(table_row[code]) * (b[x] != b[y])
  nA, nF, nB = n[0] / 4, n[1] / 2, n[2]
  return voxel_size ** 2 * 2 * (c1 * nA + c2 * nF / np.sqrt(2) + c3 * nB / np.sqrt(3))


def _coords(n, shift=0.0):
  c = np.arange(n) - (n - 1) / 2 - shift
  return np.meshgrid(c, c, c, indexing="ij")


def torus():
  z, y, x = _coords(24)
  return (np.sqrt(x * x + y * y) - 7) ** 2 + z * z <= 9


def filled_torus():
  z, y, x = _coords(24)
  return torus() | ((x * x + y * y <= 49) & (z * z <= 9))


def hollow_ball():
  z, y, x = _coords(24)
  r2 = x * x + y * y + z * z
  return (r2 >= 36) & (r2 <= 100)


def ball(n=32, r=12.3, shift=0.0):
  z, y, x = _coords(n, shift)
  return x * x + y * y + z * z <= r * r


def corner_pair():
  m = np.zeros((4, 4, 4), dtype=bool)
  m[1, 1, 1] = m[2, 2, 2] = True
  return m


def ring():
  m = np.zeros((3, 5, 5), dtype=bool)
  m[1, 1:4, 1:4] = True
  m[1, 2, 2] = False
  return m


def semantic_scenes():
  """(pred, gt) int32 [2, 24, 24, 24] with labels 0 .. 2.  Scene 0: the ground truth is a torus of class 1 and a 2^3 block
  of class 2, the prediction the torus with its hole filled and no block.  Scene 1: a hollow ball of class 2 on both
  sides; class 1 is empty there."""
  gt, pred = np.zeros((2, 24, 24, 24), np.int32), np.zeros((2, 24, 24, 24), np.int32)
  gt[0][torus()] = 1
  gt[0, :2, :2, :2] = 2
  pred[0][filled_torus()] = 1
  gt[1][hollow_ball()] = 2
  pred[1] = gt[1]
  return pred, gt


def batch_of(pred, gt, dev, task="semantic", mesh_labels=None, num_classes=3):
  """(pmf, ex) as the evaluation takes them: the one-hot of pred and a batch with gt as its grid, voxels of edge 1/24."""
  import types
  import torch as t
  pred, gt = t.as_tensor(pred), t.as_tensor(gt)
  B = pred.shape[0]
  pmf = t.nn.functional.one_hot(pred.to(t.int64), num_classes).permute(0, 4, 1, 2, 3).float()
  if mesh_labels is None:
    mesh_labels = [t.tensor([1, 2])] * B
  ex = types.SimpleNamespace(scene_id=[f"scene{b}" for b in range(B)], mesh_labels=mesh_labels, grid=gt.to(dev),
                             v2x_transform=t.diag(t.tensor([24.0, 24.0, 24.0, 1.0])).expand(B, 4, 4).clone())
  return pmf.to(dev), ex


def random_labels(rng, shape, num_labels, density=0.4, bad=0.0, dtype=np.int32):
  g = rng.integers(1, num_labels + 1, size=shape) if num_labels else np.ones(shape, dtype=np.int64)
  g = np.where(rng.random(shape) < density, g, 0)
  if bad:
    lo = -3 if np.issubdtype(dtype, np.signedinteger) else num_labels + 1
    g = np.where(rng.random(shape) < bad, rng.integers(lo, num_labels + 4, size=shape), g)
  return g.astype(dtype)
