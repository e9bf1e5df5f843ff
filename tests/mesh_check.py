"""numpy checks of marching-cubes output, independent of the triangle table: topology of indexed meshes and the vertex
set the contract pins (one vertex per straddling edge, float32 position formula, float64 normal formula)."""
import numpy as np


def split(m):
  """Meshes -> list of per-object (vertices f32 [v, 3], normals, faces i64 [f, 3]) on the host."""
  V, Nn, F = m.vertices.cpu().numpy(), m.normals.cpu().numpy(), m.faces.cpu().numpy().astype(np.int64)
  nv, nf = m.num_vertices.cpu().numpy(), m.num_faces.cpu().numpy()
  out, v0, f0 = [], 0, 0
  for a, b in zip(nv, nf):
    out.append((V[v0:v0 + a], Nn[v0:v0 + a], F[f0:f0 + b]))
    v0 += a
    f0 += b
  assert v0 == len(V) and f0 == len(F)
  return out


def check_closed_oriented(faces, nv):
  """Every undirected edge in exactly two faces, used once in each direction; no repeated index in a face; every
  vertex used."""
  f = np.asarray(faces, dtype=np.int64)
  assert (f >= 0).all() and (f < nv).all()
  assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all(), "degenerate face"
  d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
  key = d[:, 0] * nv + d[:, 1]
  assert len(np.unique(key)) == len(key), "directed edge used twice (inconsistent orientation / non-manifold)"
  rev = d[:, 1] * nv + d[:, 0]
  assert np.isin(rev, key).all(), "open edge"
  assert len(np.unique(f)) == nv, "unreferenced vertex"


def signed_volume(v, f):
  v = np.asarray(v, dtype=np.float64)
  a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
  return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def areas(v, f):
  v = np.asarray(v, dtype=np.float64)
  return 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)


def euler(nv, f):
  d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
  e = len(np.unique(np.sort(d, 1)[:, 0] * nv + np.sort(d, 1)[:, 1]))
  return nv - e + len(f)


def padded(grid):
  g = np.asarray(grid, dtype=np.float32)
  g = np.where(np.isnan(g), np.float32(0), g)
  return np.pad(g, 1)


def expected_vertices(grid, level=0.5, with_cond=False):
  """One object [D, H, W] -> (positions f32 [V, 3], normals f64 [V, 3]) in the contract's order.  with_cond: also the
  condition number of each normal in float32, max(|g0|, |g1|) / |g0 + t (g1 - g0)| (>= 1 where they nearly cancel)."""
  P = padded(grid)
  L = np.float32(level)
  Z, Y, X = P.shape
  grads = np.gradient(P.astype(np.float64))         # d/dz, d/dy, d/dx: central inside, one-sided on the border
  gx, gy, gz = grads[2], grads[1], grads[0]
  masks, f1s = [], []
  for a in range(3):                                 # x, y, z
    f1 = np.zeros_like(P)
    if a == 0:
      f1[:, :, :-1] = P[:, :, 1:]
    elif a == 1:
      f1[:, :-1, :] = P[:, 1:, :]
    else:
      f1[:-1, :, :] = P[1:, :, :]
    masks.append((P > L) != (f1 > L))
    f1s.append(f1)
  M = np.stack(masks, -1)
  z, y, x, a = np.nonzero(M)                         # raster order (z, y, x), then axis
  f0 = P[z, y, x]
  f1 = np.stack(f1s, -1)[z, y, x, a]
  t = (L - f0) / (f1 - f0)
  pos = np.stack([x, y, z], 1).astype(np.float32)
  pos[np.arange(len(a)), a] = pos[np.arange(len(a)), a] + t
  d = np.stack([a == 0, a == 1, a == 2], 1).astype(np.int64)
  z1, y1, x1 = z + d[:, 2], y + d[:, 1], x + d[:, 0]
  G0 = np.stack([gx[z, y, x], gy[z, y, x], gz[z, y, x]], 1)
  G1 = np.stack([gx[z1, y1, x1], gy[z1, y1, x1], gz[z1, y1, x1]], 1)
  n = -(G0 + t.astype(np.float64)[:, None] * (G1 - G0))
  ln = np.linalg.norm(n, axis=1, keepdims=True)
  cond = np.maximum(np.linalg.norm(G0, axis=1), np.linalg.norm(G1, axis=1)) / np.maximum(ln[:, 0], 1e-30)
  n = np.where(ln > 0, n / np.where(ln > 0, ln, 1), 0)
  return (pos, n, np.maximum(cond, 1.0)) if with_cond else (pos, n)


def case_field(case, rng, level=0.5):
  """2x2x2 object whose corner c = dx + 2 dy + 4 dz is inside iff bit c of `case` is set; values strictly off the level."""
  g = np.empty((2, 2, 2), np.float32)
  for c in range(8):
    dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
    g[dz, dy, dx] = level + rng.uniform(0.05, 1.0) if (case >> c) & 1 else level - rng.uniform(0.05, 0.45)
  return g


def ellipsoid_fields(n, size, seed, blobs=3):
  """Near-binary synthetic objects: a clipped signed distance of a few random ellipsoids, values in [0, 1]."""
  rng = np.random.RandomState(seed)
  ax = np.arange(size, dtype=np.float32)
  Z, Y, X = np.meshgrid(ax, ax, ax, indexing="ij")
  out = np.zeros((n, size, size, size), np.float32)
  for i in range(n):
    f = np.full((size, size, size), -1e9, np.float32)
    for _ in range(blobs):
      c = rng.uniform(0.3, 0.7, 3) * size
      r = rng.uniform(0.08, 0.25, 3) * size
      q = np.sqrt(((X - c[2]) / r[2]) ** 2 + ((Y - c[1]) / r[1]) ** 2 + ((Z - c[0]) / r[0]) ** 2)
      f = np.maximum(f, (1 - q) * r.min())
    out[i] = np.clip(0.5 + 0.5 * f, 0, 1)
  return out
