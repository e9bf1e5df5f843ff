"""numpy restatement of corenet_amd.mesh_ops (the same float32 operations in the same order, so equality is exact) and
the small meshes its tests run on.  Nothing here calls the library under test except the marching-cubes generators."""
import functools

import numpy as np
import torch as t

F32 = np.float32


# ---- comparing ---------------------------------------------------------------------------------------------------------
def bits(x):
  x = t.as_tensor(x).cpu().contiguous()
  return x.view(t.int32) if x.dtype == t.float32 else (x.view(t.int64) if x.dtype == t.float64 else x)


def same(a, b, what=""):
  """Exact equality: integers by value, floats on their bit patterns (so NaN patterns count)."""
  a, b = t.as_tensor(a), t.as_tensor(b)
  assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype} {tuple(a.shape)} against {b.dtype} {tuple(b.shape)}"
  assert t.equal(bits(a), bits(b)), f"{what}: differ"


# ---- batches -----------------------------------------------------------------------------------------------------------
def batch(objects):
  """[(vertices [v, 3], faces [f, 3] local ids)] -> (vertices f32, faces i32, num_vertices i64, num_faces i64) tensors."""
  vs = [np.asarray(v, F32).reshape(-1, 3) for v, _ in objects]
  fs = [np.asarray(f, np.int32).reshape(-1, 3) for _, f in objects]
  V = np.concatenate(vs) if vs else np.zeros((0, 3), F32)
  Fa = np.concatenate(fs) if fs else np.zeros((0, 3), np.int32)
  return (t.from_numpy(V.copy()), t.from_numpy(Fa.copy()), t.tensor([len(v) for v in vs], dtype=t.int64),
          t.tensor([len(f) for f in fs], dtype=t.int64))


def fan(k, rng):
  """A hub (vertex 0) with k rim vertices and the k faces (hub, r_i, r_i+1) around it: the hub has valence k."""
  a = np.arange(k) * (2 * np.pi / k)
  v = np.concatenate([[[0, 0, 1]], np.stack([np.cos(a), np.sin(a), 0 * a], 1)]) + rng.uniform(-0.01, 0.01, (k + 1, 3))
  i = np.arange(k)
  return v.astype(F32), np.stack([0 * i, 1 + i, 1 + (i + 1) % k], 1)


TETRA = [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]]


def small_objects(rng):
  """The irregular and degenerate cases, one object each, with what is_closed must say."""
  p = lambda n: rng.uniform(-1, 1, (n, 3)).astype(F32)
  flipped = [list(f) for f in TETRA]
  flipped[2] = flipped[2][::-1]
  return [
      ("tetrahedron", p(4), TETRA, True),
      ("no_faces", p(3), [], True),
      ("open_square", p(4), [[0, 1, 2], [0, 2, 3]], False),
      ("no_vertices", p(0), [], True),
      ("three_faces_on_an_edge", p(5), [[0, 1, 2], [1, 0, 3], [0, 1, 4]], False),
      ("flipped_face", p(4), flipped, False),
      ("degenerate_face", p(5), TETRA + [[0, 0, 4]], False),
      ("repeated_face", p(4), TETRA + [TETRA[0]], False),
      ("unused_vertex", p(6), TETRA, True),
      ("two_sided_triangle", p(3), [[0, 1, 2], [0, 2, 1]], True),
  ]


def fan_valences(tiles):
  T, C = tiles.sort_lane, tiles.sort_tile
  # the corner list of a hub has `valence` keys, its candidate list twice as many
  return sorted({T // 2 - 1, T // 2, T // 2 + 1, T - 1, T, T + 1, 4 * T + 3, C // 2, C // 2 + 1, C, C + 1, 2 * C + 5})


@functools.lru_cache(maxsize=None)
def ball_mesh(size=24, radius=9.3):
  """(Meshes on the host, centre) of marching cubes on the 0/1 mask of a ball."""
  from corenet_amd.visualization import marching_cubes
  ax = np.arange(size, dtype=np.float64)
  Z, Y, X = np.meshgrid(ax, ax, ax, indexing="ij")
  c = (size - 1) / 2
  mask = ((X - c) ** 2 + (Y - c) ** 2 + (Z - c) ** 2 <= radius ** 2).astype(F32)
  return marching_cubes(t.from_numpy(mask)[None]), np.array([c + 1, c + 1, c + 1])          # the padded index space


def cases(tiles):
  """name -> (vertices, faces, num_vertices, num_faces): every mesh the topology / smoothing / normal tests share."""
  rng = np.random.RandomState(7)
  out = {}
  out["fans"] = batch([fan(k, rng) for k in fan_valences(tiles)])
  small = small_objects(rng)
  out["small"] = batch([(v, f) for _, v, f, _ in small])
  for d in (-1, 0, 1):
    out[f"workgroup{d:+d}"] = batch([fan(tiles.threads + d - 1, rng)])                       # V = threads + d
  out["two_workgroups"] = batch([fan(tiles.threads - 1, rng), fan(5, rng), fan(tiles.threads + 7, rng)])
  out["empty"] = batch([])
  m = ball_mesh()[0]
  out["ball"] = (m.vertices, m.faces, m.num_vertices, m.num_faces)
  return out


# ---- topology ----------------------------------------------------------------------------------------------------------
def np_offsets(counts):
  return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int64)


def np_global_faces(faces, nv, nf):
  voff = np_offsets(nv)
  obj = np.repeat(np.arange(len(nf)), np.asarray(nf, np.int64))
  return np.asarray(faces, np.int64) + voff[obj][:, None], obj


def np_topology(faces, nv, nf):
  """dict of the MeshTopology tables."""
  g, _ = np_global_faces(faces, nv, nf)
  V, Fn = int(np.sum(nv)), len(g)
  corner = np.arange(3 * Fn, dtype=np.int64)                                 # 3 f + c
  src = g.reshape(-1)
  order = np.lexsort((corner, src))
  vf_offsets = np_offsets(np.bincount(src, minlength=V))
  nxt, prv = np.roll(g, -1, 1).reshape(-1), np.roll(g, 1, 1).reshape(-1)
  outk, ink = src * V + nxt, src * V + prv                                  # v -> w as seen from v, w -> v as seen from v
  pairs = np.unique(np.concatenate([outk, ink]))
  ko, co = np.unique(outk, return_counts=True)
  ki, ci = np.unique(ink, return_counts=True)
  nout, nin = np.zeros(len(pairs), np.int64), np.zeros(len(pairs), np.int64)
  nout[np.searchsorted(pairs, ko)] = co
  nin[np.searchsorted(pairs, ki)] = ci
  pv, pw = pairs // max(V, 1), pairs % max(V, 1)
  notreg = (nout != 1) | (nin != 1) | (pv == pw)
  irregular = np.zeros(V, bool)
  irregular[pv[notreg]] = True
  keep = pv != pw
  vv_offsets = np_offsets(np.bincount(pv[keep], minlength=V))
  return dict(vf_offsets=vf_offsets, vf_corners=corner[order].astype(np.int32), vv_offsets=vv_offsets,
              vv_neighbours=pw[keep].astype(np.int32), irregular=irregular)


def check_topology(topo, ref):
  for name, want in ref.items():
    same(getattr(topo, name), t.from_numpy(want), name)


# ---- smoothing and normals ---------------------------------------------------------------------------------------------
def _columns(offsets, values):
  """Yields (rows, values[offsets[rows] + j]) for j = 0, 1, ...: column j of the lists padded to the longest one, for the rows
  that have one -- adding column by column is the sequential sum of every list."""
  offsets, values = np.asarray(offsets, np.int64), np.asarray(values)
  k = offsets[1:] - offsets[:-1]
  for j in range(int(k.max()) if len(k) else 0):
    rows = np.nonzero(k > j)[0]
    yield rows, values[offsets[rows] + j]


def np_smooth_step(v, vv_offsets, vv, f, fixed=None):
  v = np.asarray(v, F32)
  k = np.diff(np.asarray(vv_offsets, np.int64))
  out = v.copy()
  s = np.zeros_like(v)
  with np.errstate(all="ignore"):
    for j, (rows, nb) in enumerate(_columns(vv_offsets, vv)):
      s[rows] = v[nb] if j == 0 else s[rows] + v[nb]
    m = s / np.maximum(k, 1).astype(F32)[:, None]
    new = v + F32(f) * (m - v)
  move = k >= 1
  if fixed is not None:
    move &= ~np.asarray(fixed, bool)
  out[move] = new[move]
  return out


def np_taubin(v, topo_ref, iterations, lam=0.5, mu=-0.53, fixed=None):
  v = np.asarray(v, F32).copy()
  for _ in range(iterations):
    v = np_smooth_step(v, topo_ref["vv_offsets"], topo_ref["vv_neighbours"], lam, fixed)
    if mu is not None:
      v = np_smooth_step(v, topo_ref["vv_offsets"], topo_ref["vv_neighbours"], mu, fixed)
  return v


def np_face_normals(v, faces, nv, nf):
  v = np.asarray(v, F32)
  g, _ = np_global_faces(faces, nv, nf)
  with np.errstate(all="ignore"):
    a, b, c = v[g[:, 0]], v[g[:, 1]], v[g[:, 2]]
    u, w = b - a, c - a
    return np.stack([(u[:, 1] * w[:, 2]) - (u[:, 2] * w[:, 1]), (u[:, 2] * w[:, 0]) - (u[:, 0] * w[:, 2]),
                     (u[:, 0] * w[:, 1]) - (u[:, 1] * w[:, 0])], 1).astype(F32)


def np_vertex_normals(v, faces, nv, nf, topo_ref):
  fn = np_face_normals(v, faces, nv, nf)
  s = np.zeros((len(v), 3), F32)
  with np.errstate(all="ignore"):
    for rows, cf in _columns(topo_ref["vf_offsets"], topo_ref["vf_corners"].astype(np.int64) // 3):
      s[rows] = s[rows] + fn[cf]
    ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])[:, None]
    return np.where(ln == 0, F32(0), s / ln).astype(F32)


# ---- clustering --------------------------------------------------------------------------------------------------------
def np_cluster(v, faces, nv, nf, cell):
  """dict(vertices, faces, num_vertices, num_faces, vertex_map, cluster_size) of cluster_decimate, normals aside."""
  v, cell = np.asarray(v, F32), F32(cell)
  V = len(v)
  x = v / cell
  c = np.floor(x)
  u = ((x - c) * F32(1048576.0)).astype(np.int64)
  vobj = np.repeat(np.arange(len(nv)), np.asarray(nv, np.int64))
  key = np.concatenate([vobj[:, None], c.astype(np.int64)], 1)
  _, inv = np.unique(key, axis=0, return_inverse=True)
  inv = inv.reshape(-1)
  K = int(inv.max()) + 1 if V else 0
  leader = np.full(K, V, np.int64)
  np.minimum.at(leader, inv, np.arange(V))
  rank = np.empty(K, np.int64)
  rank[np.argsort(leader)] = np.arange(K)
  vmap = rank[inv]
  count = np.bincount(vmap, minlength=K)
  sums = np.zeros((K, 3), np.int64)
  np.add.at(sums, vmap, u)
  cc = np.zeros((K, 3), np.float64)
  cc[vmap] = c.astype(np.float64)
  pos = ((cc + (sums.astype(np.float64) / np.maximum(count, 1).astype(np.float64)[:, None]) * 2.0 ** -20) * np.float64(cell)).astype(F32)
  new_nv = np.bincount(vobj[np.sort(leader)], minlength=len(nv)).astype(np.int64)
  g, fobj = np_global_faces(faces, nv, nf)
  m = vmap[g] if len(g) else np.zeros((0, 3), np.int64)
  keep = (m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 0] != m[:, 2])
  new_f = (m[keep] - np_offsets(new_nv)[fobj[keep]][:, None]).astype(np.int32)
  return dict(vertices=pos, faces=new_f, num_vertices=new_nv, num_faces=np.bincount(fobj[keep], minlength=len(nf)).astype(np.int64),
              vertex_map=vmap.astype(np.int32), cluster_size=count.astype(np.int32))


def check_decimated(dec, ref):
  for name in ("vertices", "faces", "num_vertices", "num_faces"):
    same(getattr(dec.meshes, name), t.from_numpy(ref[name]), name)
  same(dec.vertex_map, t.from_numpy(ref["vertex_map"]), "vertex_map")
  same(dec.cluster_size, t.from_numpy(ref["cluster_size"]), "cluster_size")


def decimation_cases(tiles):
  """name -> ((vertices, faces, num_vertices, num_faces), cell_size)."""
  rng = np.random.RandomState(11)
  m = ball_mesh()[0]
  ball = (m.vertices.numpy(), m.faces.numpy())
  shifted = (ball[0] - F32(12.5), ball[1])
  out = {}
  for cell in (0.3, 2.0, 0.5):                                               # 0.5: every vertex of a mask mesh lies on a cell face
    out[f"ball_negative_{cell}"] = (batch([shifted]), cell)
  out["one_cluster"] = (batch([ball]), 64.0)
  out["identical_objects"] = (batch([ball, (ball[0][:0], ball[1][:0]), ball]), 2.0)
  for name, V, extent in (("few_hundred_cells", 5000, 6.0), ("about_5000_cells", 5000, 17.0), ("half_full_table", 4096, 200.0)):
    v = rng.uniform(-extent / 2, extent / 2, (V, 3)).astype(F32)
    out[name] = (batch([(v, rng.randint(0, V, (V, 3)))]), 1.0)
  lo, hi = tiles.cell_min, tiles.cell_max
  out["cell_bounds"] = (batch([([[lo, lo + 0.25, hi + 0.5], [hi, hi + 0.75, lo], [0, 0, 0], [lo, hi + 0.5, lo + 0.25]], [[0, 1, 2], [0, 3, 2]])]), 1.0)
  out["empty"] = (batch([]), 1.0)
  return out
