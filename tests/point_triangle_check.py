"""Shared inputs and the float64 oracle of the point-to-triangle tests (test_point_triangle_cpu.py / _gpu.py).

The library computes z^2 plus an in-plane distance in a per-triangle frame (csrc/point_metrics_common.h).  The oracle is
written the other way: the region walk of the closest-point algorithm (Ericson, Real-Time Collision Detection, 5.1.5:
vertex regions, then edge regions, then the face, by the signs of six dot products), in numpy float64, and it returns the
distance to EVERY triangle."""
import functools
import os

import numpy as np

import point_metrics_check as PC

# Tolerances on distances (not squared): 4 x the largest error of the host twin against the oracle, measured on the CPU on
# the inputs of accuracy_case() / sliver_case().  accuracy_case: |sqrt(d2) - oracle minimum| is at
# most 1.58e-7 (a float32 ulp at the distances of up to 1.7 its single-triangle object gives), and the chosen triangle
# is the oracle's nearest every time.  sliver_case: sqrt(d2) falls below the oracle minimum by at most 4.08e-8 and exceeds
# the distance to the nearest vertex of the chosen triangle by at most 2.95e-8.  The margin is for other seeds, not for
# other arithmetic: the GPU equals the twin bit for bit.
TOL = 4 * 1.58e-7
TOL_SLIVER = 4 * 4.08e-8

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TAUS = (0.01, 0.02, 0.05)                # the default F-score thresholds of evaluation_results

ONE = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)

# (query, d2) on ONE: the face, the three edges, the three vertices, then points on a vertex, an edge and the face
REGIONS = [((0.25, 0.25, 0.5), 0.25),
           ((0.5, -0.5, 0), 0.25), ((-0.5, 0.5, 0), 0.25), ((1, 1, 0), 0.5),
           ((-1, -1, 0), 2), ((2, -0.5, 0), 1.25), ((-0.5, 2, 0), 1.25),
           ((1, 0, 0), 0), ((0, 1, 0), 0), ((0, 0, 0), 0), ((0.5, 0.5, 0), 0), ((0.5, 0, 0), 0), ((0, 0.25, 0), 0),
           ((0.25, 0.25, 0), 0), ((0.125, 0.5, 0), 0),
           ((0.25, 0.5, -2), 4), ((0.5, -0.5, 1), 1.25), ((-1, -1, 1), 3)]


def offsets(counts):
  return PC.offsets(counts)


def closest_distances(p, tri, chunk=128):
  """f64 [Q, T]: the distance from every point of p [Q, 3] to every triangle of tri [T, 3, 3], by the region walk."""
  p, tri = np.asarray(p, np.float64), np.asarray(tri, np.float64)
  out = np.empty((len(p), len(tri)), np.float64)
  for t0 in range(0, len(tri), chunk):
    out[:, t0:t0 + chunk] = _walk(p[:, None, :], tri[None, t0:t0 + chunk])
  return out


def _walk(p, tri):
  a, b, c = tri[:, :, 0], tri[:, :, 1], tri[:, :, 2]
  ab, ac = b - a, c - a

  def dot(u, v):
    return (u * v).sum(-1)
  ap, bp, cp = p - a, p - b, p - c
  d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
  vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
  shape = np.broadcast(d1, d1).shape
  point = np.zeros(shape + (3,))
  done = np.zeros(shape, bool)

  def region(cond, where):
    take = cond & ~done
    point[take] = np.broadcast_to(where, point.shape)[take]
    done[take] = True
  with np.errstate(all="ignore"):
    region((d1 <= 0) & (d2 <= 0), a)                                                       # vertex A
    region((d3 >= 0) & (d4 <= d3), b)                                                      # vertex B
    region((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + ab * (d1 / (d1 - d3))[..., None])        # edge AB
    region((d6 >= 0) & (d5 <= d6), c)                                                      # vertex C
    region((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + ac * (d2 / (d2 - d6))[..., None])        # edge AC
    region((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0),
           b + (c - b) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None])                 # edge BC
    den = va + vb + vc
    region(np.ones(shape, bool), a + ab * (vb / den)[..., None] + ac * (vc / den)[..., None])   # the face
  return np.sqrt(dot(p - point, p - point))


def eligible(tri):
  """The contract's rule, restated in float32: |cross(B - A, C - A)| positive and finite."""
  t = np.asarray(tri, np.float32)
  with np.errstate(all="ignore"):
    e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    area = np.sqrt((cx * cx + cy * cy) + cz * cz)
  return (area > 0) & (area < np.inf)


def min_angle_deg(tri):
  t = np.asarray(tri, np.float64)
  out = np.full(len(t), 180.0)
  for i in range(3):
    u, v = t[:, (i + 1) % 3] - t[:, i], t[:, (i + 2) % 3] - t[:, i]
    cos = (u * v).sum(1) / (np.linalg.norm(u, axis=1) * np.linalg.norm(v, axis=1))
    out = np.minimum(out, np.degrees(np.arccos(np.clip(cos, -1, 1))))
  return out


def edge_lengths(tri):
  t = np.asarray(tri, np.float64)
  return np.stack([np.linalg.norm(t[:, (i + 1) % 3] - t[:, i], axis=1) for i in range(3)], 1)


def _unit(rng, n):
  v = rng.randn(n, 3)
  return v / np.linalg.norm(v, axis=1, keepdims=True)


def well_shaped(rng, n):
  """n float32 triangles in the unit cube, edges in [0.01, 0.2], smallest angle >= 15 degrees, by rejection."""
  keep = []
  while sum(len(k) for k in keep) < n:
    m = 4 * n + 64
    a = rng.rand(m, 3)
    tri = np.stack([a, a + _unit(rng, m) * rng.uniform(0.01, 0.2, (m, 1)), a + _unit(rng, m) * rng.uniform(0.01, 0.2, (m, 1))],
                   1).astype(np.float32)
    e = edge_lengths(tri)
    ok = (tri.min((1, 2)) >= 0) & (tri.max((1, 2)) <= 1) & (e.min(1) >= 0.01) & (e.max(1) <= 0.2) & (min_angle_deg(tri) >= 15)
    keep.append(tri[ok])
  return np.concatenate(keep)[:n]


def slivers(rng, n):
  """n float32 triangles in the unit cube whose smallest angle lies in [0.01, 1] degrees: needles (one short edge) and
  caps (the third vertex close to the middle of the long edge), longest edge in [0.05, 0.2]."""
  keep = []
  while sum(len(k) for k in keep) < n:
    m = 4 * n + 64
    a = rng.rand(m, 3)
    L = rng.uniform(0.05, 0.2, (m, 1))
    u = _unit(rng, m)
    w = np.cross(u, _unit(rng, m))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    theta = np.radians(10 ** rng.uniform(-2, 0, (m, 1)))
    s = np.where(rng.rand(m, 1) < 0.5, rng.uniform(0.2, 0.8, (m, 1)), 0.0)              # cap, or needle at A
    h = np.where(s > 0, np.tan(theta) * L * np.minimum(s, 1 - s), theta * L)
    tri = np.stack([a, a + u * L, a + u * L * s + w * h], 1).astype(np.float32)
    ang = min_angle_deg(tri)
    ok = (tri.min((1, 2)) >= 0) & (tri.max((1, 2)) <= 1) & (ang >= 0.01) & (ang <= 1) & eligible(tri)
    keep.append(tri[ok])
  return np.concatenate(keep)[:n]


def _freeze(*xs):
  for x in xs:
    x.setflags(write=False)
  return xs


@functools.lru_cache(maxsize=None)
def accuracy_case():
  """(points, p_off, triangles, t_off, oracle): 3 objects of 1, 300 and 1500 well-shaped triangles, 2000 queries each,
  uniform in the cube; oracle: a list of f64 [2000, T_n], computed once."""
  rng = np.random.RandomState(11)
  counts = [1, 300, 1500]
  tri = well_shaped(rng, sum(counts))
  pts = rng.rand(3 * 2000, 3).astype(np.float32)
  p_off, t_off = offsets([2000] * 3), offsets(counts)
  oracle = [closest_distances(pts[p_off[n]:p_off[n + 1]], tri[t_off[n]:t_off[n + 1]]) for n in range(3)]
  return _freeze(pts, p_off, tri, t_off) + (oracle,)


@functools.lru_cache(maxsize=None)
def sliver_case():
  """(points, p_off, triangles, t_off, oracle): 2 objects of 300 slivers; 1000 queries each: half uniform in the cube,
  half on the slivers themselves or 1e-4 / 1e-2 off them along a random direction."""
  rng = np.random.RandomState(12)
  counts = [300, 300]
  tri = slivers(rng, sum(counts))
  t_off = offsets(counts)
  pts = []
  for n in range(2):
    own = tri[t_off[n]:t_off[n + 1]].astype(np.float64)
    k = rng.randint(0, len(own), 500)
    bary = rng.dirichlet([1, 1, 1], 500)
    on = (own[k] * bary[:, :, None]).sum(1) + _unit(rng, 500) * rng.choice([0.0, 1e-4, 1e-2], (500, 1))
    pts += [rng.rand(500, 3), on]
  pts = np.concatenate(pts).astype(np.float32)
  p_off = offsets([1000, 1000])
  oracle = [closest_distances(pts[p_off[n]:p_off[n + 1]], tri[t_off[n]:t_off[n + 1]]) for n in range(2)]
  return _freeze(pts, p_off, tri, t_off) + (oracle,)


def bad_triangles():
  """Four triangles that are not eligible: a point, collinear vertices, a NaN vertex, an infinite area."""
  bad = np.zeros((4, 3, 3), np.float32)
  bad[0] = 0.25
  bad[1] = [[0, 0, 0.25], [0.25, 0.25, 0.25], [0.5, 0.5, 0.25]]
  bad[2] = [[0, 0, 0.25], [1, 0, 0.25], [np.nan, 1, 0.25]]
  bad[3] = [[-3e38, -3e38, 0.25], [3e38, -3e38, 0.25], [-3e38, 3e38, 0.25]]
  return bad


def eligibility_case():
  """(points, p_off, triangles, t_off, expect_index, expect_d2).  Object 0: the bad triangles lie in z = 0.25, closer to
  the queries (z = 0.25 .. 0.5) than its one eligible triangle, ONE in z = 0, at index 2.  Object 1: bad triangles only.
  Object 2: empty.  Object 3: ONE, queried by NaN points."""
  bad = bad_triangles()
  tri = np.concatenate([bad[:2], ONE, bad[2:], bad, ONE]).astype(np.float32)
  t_off = offsets([5, 4, 0, 1])
  q = np.array([[0.25, 0.25, 0.25], [0.25, 0.25, 0.5], [0.125, 0.5, 0.375]], np.float32)
  nanq = np.array([[np.nan, 0.25, 0.25], [0.25, np.nan, 0.25], [0.25, 0.25, np.nan]], np.float32)
  pts = np.concatenate([q, q, q, nanq])
  p_off = offsets([3, 3, 3, 3])
  idx = np.array([2, 2, 2] + [-1] * 9, np.int32)
  d2 = np.concatenate([q[:, 2] * q[:, 2], np.full(9, np.inf, np.float32)]).astype(np.float32)
  return pts, p_off, tri, t_off, idx, d2


def ties_case():
  """(points, p_off, triangles, t_off).  Object 0: two triangles at a right angle sharing the edge (0,0,0)-(1,0,0),
  queried in that edge's region (outside both), on the edge and in the region of a shared vertex; the frames are the
  coordinate axes, so both distances are exact and equal.  Object 1: a soup of 200 triangles on a grid of 1/8, every
  triangle present twice (the copy 200 places later), queries on the same grid."""
  rng = np.random.RandomState(13)
  pair = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 0], [1, 0, 0], [0, 0, 1]]], np.float32)
  q0 = np.array([[0.5, -1, -1], [0.25, -0.5, -2], [0.5, 0, 0], [-1, -1, -1], [0.75, -2, -0.5]], np.float32)
  soup = (rng.randint(0, 9, (200, 3, 3)) / 8.0).astype(np.float32)
  q1 = (rng.randint(0, 9, (500, 3)) / 8.0).astype(np.float32)
  tri = np.concatenate([pair, soup, soup])
  return np.concatenate([q0, q1]), offsets([len(q0), len(q1)]), tri, offsets([2, 400])


def sizes_case(query_tile, triangle_tile):
  """(points, p_off, triangles, t_off): objects with 0, 1, 3 and triangle_tile + 1 triangles and with 0, 1 and
  query_tile + 1 queries, in every order the kernel's early exits can meet them."""
  rng = np.random.RandomState(14)
  nt = [0, 1, 3, triangle_tile + 1, 3, 0, triangle_tile + 1]
  nq = [5, 1, 0, query_tile + 1, query_tile + 1, 0, 1]
  tri = well_shaped(rng, sum(nt))
  pts = rng.rand(sum(nq), 3).astype(np.float32)
  return pts, offsets(nq), tri, offsets(nt)


def small_triangles(rng, n):
  """n float32 triangles anywhere in the unit cube with edges up to about 0.1 (any shape: for bit-for-bit comparisons)."""
  a = rng.rand(n, 1, 3)
  return np.concatenate([a, a + (rng.rand(n, 2, 3) - 0.5) * 0.1], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def many_tiles_case(kind, triangle_tile):
  """(points, p_off, triangles, t_off) that make one workgroup walk several tiles of triangle records.
  'plain': 1024 objects of 1 query, alternately triangle_tile + 1 and 600 triangles (the second 300 repeat the first).
  'split': 8 objects of 100 queries and 2 * 128 * triangle_tile + 1 triangles, [40000, 50000) repeating [0, 10000); query
  5 is NaN."""
  rng = np.random.RandomState({"plain": 15, "split": 16}[kind])
  if kind == "plain":
    nt = [triangle_tile + 1, 600] * 512
    tri = small_triangles(rng, sum(nt))
    t_off = offsets(nt)
    for n in range(1, 1024, 2):
      tri[t_off[n] + 300:t_off[n] + 600] = tri[t_off[n]:t_off[n] + 300]
    pts = rng.rand(1024, 3).astype(np.float32)
    return _freeze(pts, offsets([1] * 1024), tri, t_off)
  nt = 2 * 128 * triangle_tile + 1
  tri = small_triangles(rng, 8 * nt)
  t_off = offsets([nt] * 8)
  for n in range(8):
    tri[t_off[n] + 40000:t_off[n] + 50000] = tri[t_off[n]:t_off[n] + 10000]
  pts = rng.rand(800, 3).astype(np.float32)
  pts[5, 1] = np.nan
  return _freeze(pts, offsets([100] * 8), tri, t_off)


def square(axis=2, value=0.0, cells=1):
  """The unit square in the plane `axis` = value as 2 * cells^2 triangles... cells = 1: 2 triangles; cells = 2: 8."""
  tri = []
  h = 1.0 / cells
  for i in range(cells):
    for j in range(cells):
      c = [(i * h, j * h), ((i + 1) * h, j * h), ((i + 1) * h, (j + 1) * h), (i * h, (j + 1) * h)]
      for k in ((0, 1, 2), (0, 2, 3)):
        tri.append([np.insert(np.array(c[v], np.float64), axis, value) for v in k])
  return np.array(tri, np.float32)


def check_accuracy(d2, idx, case, tol):
  """(a) |sqrt(d2) - oracle minimum| <= tol and (b) the oracle's distance to the chosen triangle <= minimum + tol, for
  every query of every object."""
  pts, p_off, tri, t_off, oracle = case
  d = np.sqrt(d2.astype(np.float64))
  worst_a = worst_b = 0.0
  for n, o in enumerate(oracle):
    q = slice(p_off[n], p_off[n + 1])
    assert (idx[q] >= 0).all() and (idx[q] < o.shape[1]).all()
    omin = o.min(1)
    worst_a = max(worst_a, float(np.abs(d[q] - omin).max()))
    worst_b = max(worst_b, float((o[np.arange(o.shape[0]), idx[q]] - omin).max()))
  print(f"accuracy: |sqrt(d2) - min| <= {worst_a:.3e}, chosen - min <= {worst_b:.3e}, tol {tol:.3e}")
  assert worst_a <= tol and worst_b <= tol


def check_slivers(d2, idx, case, tol):
  """oracle minimum - tol <= sqrt(d2) <= distance to the nearest vertex of the chosen triangle + tol, every query."""
  pts, p_off, tri, t_off, oracle = case
  d = np.sqrt(d2.astype(np.float64))
  lo = hi = 0.0
  for n, o in enumerate(oracle):
    q = slice(p_off[n], p_off[n + 1])
    assert (idx[q] >= 0).all() and (idx[q] < o.shape[1]).all()
    chosen = tri[t_off[n]:t_off[n + 1]].astype(np.float64)[idx[q]]
    vertex = np.linalg.norm(chosen - pts[q].astype(np.float64)[:, None, :], axis=2).min(1)
    lo = max(lo, float((o.min(1) - d[q]).max()))
    hi = max(hi, float((d[q] - vertex).max()))
  print(f"slivers: min - sqrt(d2) <= {lo:.3e}, sqrt(d2) - vertex <= {hi:.3e}, tol {tol:.3e}")
  assert lo <= tol and hi <= tol


def fixture_batch_cpu(R=32):
  """The two fixture scenes on CPU tensors: their meshes in view space (the 4x4 products applied in torch), and a pmf
  that is high inside the bounding box of every class's meshes, so that every class has a predicted surface."""
  import torch as t
  from corenet_amd.data import dataset as D
  from corenet_amd.data.batched_example import BatchedExample
  from corenet_amd.geometry import transformations as T
  root = os.path.join(G, "n2_dataset")
  ds = D.CoReNetDatasetImpl(os.path.join(root, "dataset.json"), os.path.join(root, "meshes"))
  els = [ds[0], ds[1]]
  verts, nc = [], 4
  pmf = t.full((2, nc, R, R, R), 0.1)
  centre = (t.arange(R, dtype=t.float32) + 0.5) / R
  for b, e in enumerate(els):
    start = 0
    for m, n in enumerate(e.mesh_num_tri.tolist()):
      mat = (e.view_transform @ e.o2w_transforms[m]).to(t.float32)
      v = e.mesh_vertices[start:start + n].to(t.float32)
      h = t.cat([v, t.ones_like(v[..., :1])], -1) @ mat.T
      v = h[..., :3] / h[..., 3:]
      verts.append(v)
      start += n
      k = int(e.mesh_labels[m])
      if 1 <= k < nc:
        lo, hi = v.reshape(-1, 3).min(0)[0].clamp(0.1, 0.8), v.reshape(-1, 3).max(0)[0].clamp(0.2, 0.9)
        ins = [(centre >= lo[a]) & (centre <= hi[a]) for a in range(3)]            # x, y, z
        pmf[b, k][ins[2][:, None, None] & ins[1][None, :, None] & ins[0][None, None, :]] = 0.9
  ex = BatchedExample(
      vertices=t.cat(verts), view_transform=t.stack([e.view_transform for e in els]),
      camera_transform=t.stack([e.camera_transform for e in els]), mesh_num_tri=[e.mesh_num_tri for e in els],
      mesh_labels=[e.mesh_labels for e in els], input_image=t.stack([e.input_image for e in els]),
      scene_id=[e.scene_id for e in els], grid_sampling_offset=t.full((2, 3), 0.5),
      v2x_transform=T.scale([float(R)] * 3).expand(2, 4, 4).clone(), grid=t.zeros((2, R, R, R), dtype=t.int32))
  return pmf, ex
