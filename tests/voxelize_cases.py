"""The case table of the ground-truth voxelizer (csrc/voxelize.hip: crn_voxelize_mesh, crn_merge_labels, crn_transform_meshes)
and an independent float64 reference of its geometry.  TEST INFRASTRUCTURE ONLY.

One row = one call: grid D x H x W, image_resolution_multiplier, projection_depth_multiplier, conservative flag, sub-grid
mode, a list of meshes and their view2voxel matrices.  tests/test_voxelize_ref_cpu.py holds the oracle (O.voxelize_mesh, the
fp32 restatement the kernel is bit-equal to) inside the band of every row and shows that seeded wrong oracles leave it;
tests/test_voxelize_gpu.py runs every row on the GPU.

band(case) -> (MUST, MAY), bool [M, Dg, Hg, Wg] each.  The reference shares no formula with the kernel or the oracle: no NDC, no
viewport, no edge-function coefficients, no barycentric interpolation.  Per triangle, on the fp32 inputs widened to float64:
  * vertices -> voxel space with rows 0-2 of the mesh's matrix;
  * n = cross product of two edges; the projection axis is the strictly dominant |n| component, z without one
    (voxelize.geom:53-55);
  * the sample lattice lives in voxel space: along a voxel axis of extent E (W, H, D * pdm for x, y, z) the samples are
    (k + 1/2) E / R, k = 0 .. R - 1, R = round_half_even(max(W, H, D * pdm) * multiplier) (voxelization.py:146-148);
  * plain mode: a lattice point yields a fragment if its signed distance to the three edge lines of the projected triangle is
    positive; conservative mode: MUST if the sample's E_u/R x E_v/R cell overlaps the triangle (separating axes of the rectangle
    and the triangle), MAY if the cell lies within two pixels of the triangle's bounding box and passes the offset-edge test
    (distance to each edge line >= -(half cell projected on the edge normal)): GL allows that over-coverage;
  * the fragment's position is the point of the triangle's plane over the sample (the plane equation solved for the depth
    coordinate; extrapolated in conservative mode); it is kept if the depth coordinate is within [0, E_depth] and the point inside
    [0, W) x [0, H) x [0, D) (voxelize.frag:36-38);
  * the voxel is floor(p), in sub-grid mode the virtual-voxel rule of voxelize.frag:48-55.
A fragment is DECIDED when none of its decisions lies within tau of its boundary: the three edge distances (tau), the depth clip,
the grid bounds and each coordinate's distance to the next (virtual-)voxel border (4 tau).  A triangle whose two largest
normalised |n| components lie within 1e-5 of each other is undecided as a whole; its candidates are taken over every axis the tie
can break to (z included: the shader's choice at an exact tie).  MUST = the voxels of decided fragments, MAY = the voxels of every
possible outcome of every candidate fragment.  A correct rasterizer gives MUST <= result <= MAY.

tau = 2^-18 (largest |voxel-space coordinate| of the triangle + largest extent), in voxel units: 64 fp32 roundings of the largest
term, where the kernel's chain from vertex to edge value has about ten.  The factor is a choice, nobody has measured the kernel's
error, and it is not tuned against the kernel: the CPU module validates it against the oracle.

Triangles with a non-finite voxel-space vertex and triangles of zero area yield nothing.  The raster-spanning triangle has its
vertices at most three extents outside the grid: much larger triangles lose fp32 precision in the edge functions (the constant
term is a difference of products of pixel coordinates) and are outside what is pinned here.

Cap: |MAY \\ MUST| <= 5 % of |MUST| for each row and each mesh, |MUST| >= 200 per row (the rows with T <= 1 cannot reach the
floor: they are `tiny` and must have MAY == MUST instead).  Measured |MAY \\ MUST| / |MUST| per row (largest mesh share in
brackets), from the reference alone:
  w14_m4             |MUST|   586    0.00 %  ( 0.00 %)
  w14_m4_cons        |MUST|   643    2.33 %  ( 2.50 %)
  d12_m3_pdm2        |MUST|   397    0.76 %  ( 1.00 %)
  d12_m3_pdm2_cons   |MUST|   448    2.46 %  ( 4.00 %)
  h16_m8             |MUST|   520    0.38 %  ( 0.90 %)
  h16_m8_cons        |MUST|   550    1.27 %  ( 1.67 %)
  w20_m1             |MUST|   295    0.00 %  ( 0.00 %)
  w20_m1_cons        |MUST|   357    3.64 %  ( 5.00 %)
  w20_m3_pdm2        |MUST|   310    1.94 %  ( 2.69 %)
  w20_m3_pdm2_cons   |MUST|   338    2.37 %  ( 2.53 %)
  c3_m15             |MUST|   226    0.00 %  ( 0.00 %)
  c3_m15_cons        |MUST|   287    0.00 %  ( 0.00 %)
  c7_m15             |MUST|   286    0.00 %  ( 0.00 %)
  c7p_m15            |MUST|   269    0.00 %  ( 0.00 %)
  c7p_m15_cons       |MUST|   312    0.00 %  ( 0.00 %)
  affine_m4          |MUST|   515    0.00 %  ( 0.00 %)
  affine_m4_cons     |MUST|   539    2.60 %  ( 4.03 %)
  ties_m4            |MUST|   753    1.46 %  ( 1.46 %)
  ties_m4_cons       |MUST|   765    4.84 %  ( 4.84 %)
  sub3_cons          |MUST|   690    2.75 %  ( 3.91 %)
  sub5_cons          |MUST|  1058    2.65 %  ( 3.83 %)
  sub9_cons          |MUST|  1104    0.91 %  ( 1.26 %)
  sub3               |MUST|   811    0.00 %  ( 0.00 %)
  sub5               |MUST|   918    0.22 %  ( 0.22 %)
  list_5_0_7_0       |MUST|   310    0.32 %  ( 0.59 %)
  nonfinite          |MUST|   473    0.00 %  ( 0.00 %)
  finite_twin        |MUST|   473    0.00 %  ( 0.00 %)
  t0_m2              |MUST|     0    0.00 %  ( 0.00 %)
  t1                 |MUST|    29    0.00 %  ( 0.00 %)
The seeds and mesh choices of the rows were taken so that the reference alone meets the cap; no figure here comes from the kernel.
"""
from __future__ import annotations

import dataclasses
import functools
import math
from typing import Tuple

import numpy as np

from oracle import corenet_oracle as O

SENTINEL = -1234.5
TAIL = 64                     # floats behind the grid in its storage
TIE = 1e-5                    # normalised |n| components closer than this: the axis choice is undecided
CAP = 0.05
FLOOR = 200


@dataclasses.dataclass(frozen=True)
class Case:
  name: str
  grid: Tuple[int, int, int]                 # D, H, W
  mult: float
  meshes: Tuple[Tuple[str, ...], ...]        # one tuple of parts per mesh; () = an empty mesh
  pdm: int = 1
  cons: bool = False
  sub: bool = False
  mats: str = "identity"                     # identity | affine (per-mesh rotation, non-uniform scale, translation)
  seed: int = 0
  tiny: bool = False                         # T <= 1: no floor, MAY == MUST instead
  pins: Tuple[str, ...] = ()


def _rows():
  std = (("ellipsoid", "slivers", "degenerate"), ("cross", "big"), ("negative",))
  r = []
  def both(name, grid, mult, meshes=std, **kw):
    r.append(Case(name, grid, mult, meshes, **kw))                       # the same geometry, plain and conservative
    r.append(Case(name + "_cons", grid, mult, meshes, cons=True, **kw))
  both("w14_m4", (6, 10, 14), 4, pins=("W largest", "T = 4k + 1", "slivers", "zero area", "six faces", "raster-spanning"))
  both("d12_m3_pdm2", (12, 5, 9), 3, pdm=2, pins=("D * pdm largest",))
  both("h16_m8", (5, 16, 8), 8, pins=("H largest",))
  both("w20_m1", (4, 4, 20), 1, meshes=std + (("ellipsoid2",),), pins=("multiplier 1",))
  both("w20_m3_pdm2", (4, 4, 20), 3, pdm=2, seed=5, pins=("D * pdm not largest",))
  # the x 1.5 rows: conservative cells of 0.7 voxels over-cover every acute corner inside the grid (GL allows it), which an
  # ellipsoid at this size cannot keep under the cap: the conservative rows use triangles whose corners lie outside the grid
  both("c3_m15", (3, 3, 3), 1.5, meshes=(("planes",),) * 20, seed=1, pins=("R = 4, not 5",))
  r.append(Case("c7_m15", (7, 7, 7), 1.5, (("ellipsoid",), ("cross", "big"), ("ellipsoid2",), ("planes",)), pins=("R = 10, not 11",)))
  both("c7p_m15", (7, 7, 7), 1.5, meshes=(("planes",),) * 4, seed=1, pins=("R = 10, not 11",))
  both("affine_m4", (6, 10, 14), 4, meshes=(("unit_sphere",), ("unit_sphere",), ("unit_cross",)), mats="affine", seed=1,
       pins=("per-mesh rotation and non-uniform scale",))
  both("ties_m4", (16, 16, 16), 4, meshes=(("ellipsoid", "ties"),), pins=("normals (1,1,0) (0,1,1) (1,0,1) (1,1,1)",))
  r.append(Case("sub3_cons", (5, 8, 6), 3, (("planes",), ("planes", "slivers", "degenerate"), ("negative",)), cons=True, sub=True,
                seed=3, pins=("sub-grid side 3",)))            # cells of a third of a voxel: corners outside the grid, as above
  for vs in (5, 9):
    r.append(Case(f"sub{vs}_cons", (5, 8, 6), vs, std, cons=True, sub=True, pins=(f"sub-grid side {vs}",)))
  for vs in (3, 5):
    r.append(Case(f"sub{vs}", (5, 8, 6), vs, std, sub=True, pins=(f"sub-grid side {vs}, plain",)))
  r.append(Case("list_5_0_7_0", (6, 10, 14), 4, (("tri5",), (), ("tri7",), ()), pins=("empty meshes in the middle and at the end",)))
  r.append(Case("nonfinite", (6, 10, 14), 4, (("ellipsoid", "nonfinite"), ("cross", "nonfinite")), pins=("NaN and +-Inf vertices",)))
  r.append(Case("finite_twin", (6, 10, 14), 4, (("ellipsoid",), ("cross",))))
  r.append(Case("t0_m2", (6, 10, 14), 4, ((), ()), tiny=True, pins=("T = 0",)))
  r.append(Case("t1", (6, 10, 14), 4, (("one",),), tiny=True, pins=("T = 1",)))
  return tuple(r)


# ---------------------------------------------------------------------------------------------------------------- meshes
def _rot(ax, ay, az):
  cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
  rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
  ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
  rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
  return rz @ ry @ rx


def _uv_sphere(n_lat, n_lon):
  th = np.linspace(0, np.pi, n_lat + 1); ph = np.linspace(0, 2 * np.pi, n_lon + 1)
  p = lambda a, b: np.array([np.sin(a) * np.cos(b), np.sin(a) * np.sin(b), np.cos(a)])
  tris = []
  for i in range(n_lat):
    for j in range(n_lon):
      a, b, c, d = p(th[i], ph[j]), p(th[i + 1], ph[j]), p(th[i + 1], ph[j + 1]), p(th[i], ph[j + 1])
      tris += [[a, b, c], [a, c, d]]
  return np.array(tris)


def _part(kind, dims, rng):
  """Triangles [n, 3, 3] (x, y, z) in voxel space (unit_*: in object space) of one part of a mesh.  dims = (W, H, D)."""
  dims = np.asarray(dims, np.float64)
  if kind in ("ellipsoid", "ellipsoid2"):              # tilted off every 45-degree symmetry
    ang, frac, cen = ((0.37, 0.21, 0.53), 0.43, 0.5) if kind == "ellipsoid" else ((-0.23, 0.61, 0.17), 0.31, 0.46)
    return (_uv_sphere(8, 11) * (frac * dims)) @ _rot(*ang).T + cen * dims
  if kind == "unit_sphere":
    return _uv_sphere(7, 9)
  if kind == "unit_cross":                              # object space [-1, 1]^3, reaches beyond the grid after the matrix
    c = rng.uniform(-1.2, 1.2, (30, 1, 3))
    return c + rng.uniform(-0.45, 0.45, (30, 3, 3))
  if kind == "cross":                                   # straddles each of the six faces in turn
    out = []
    for i in range(42):
      c = rng.uniform(0.1, 0.9, 3) * dims
      c[(i % 6) // 2] = 0.0 if i % 2 == 0 else dims[(i % 6) // 2]
      out.append(c + rng.uniform(-0.3, 0.3, (3, 3)) * dims)
    return np.array(out)
  if kind == "big":                                     # covers the whole raster of the z projection
    W, H, D = dims
    z = lambda x, y: D * (0.3 + 0.25 * x / W + 0.2 * y / H)
    xy = [(-2.5 * W, -0.8 * H), (3.5 * W, -0.8 * H), (0.5 * W, 3.6 * H)]
    return np.array([[[x, y, z(x, y)] for x, y in xy]])
  if kind == "slivers":                                 # longest edge / height = 1500
    out = []
    for _ in range(8):
      d = rng.normal(size=3); d /= np.linalg.norm(d)
      q = np.cross(d, rng.normal(size=3)); q /= np.linalg.norm(q)
      L = 0.7 * dims.min()
      p = 0.5 * dims + rng.uniform(-0.15, 0.15, 3) * dims - 0.5 * L * d
      out.append([p, p + L * d, p + 0.5 * L * d + (L / 1500) * q])
    return np.array(out)
  if kind == "degenerate":                              # repeated vertices, collinear vertices on an axis
    a, b, c = np.array([1., 2., 1.]), np.array([2., 1., 2.]), np.array([2., 2., 1.])
    return np.array([[a, a, b], [a, b, a], [b, a, a], [a, a, a], [[1, 2, 1], [2, 2, 1], [3, 2, 1]], [[1, 1, 0], [1, 2, 0], [1, 3, 0]]],
                    np.float64)
  if kind == "negative":
    return rng.uniform(-9, -1, (4, 3, 3))
  if kind == "nonfinite":
    t = rng.uniform(0.2, 0.8, (3, 3, 3)) * dims
    t[0, 1, 0] = np.nan; t[1, 2, 1] = np.inf; t[2, 0, 2] = -np.inf
    return t
  if kind == "ties":                                    # integer coordinates: exact ties in fp32 as well
    o = np.array([3., 2., 9.])
    return np.array([[[0, 1, 0], [1, 0, 0], [0, 1, 1]], [[0, 0, 1], [0, 1, 0], [1, 0, 1]], [[0, 0, 1], [1, 0, 0], [0, 1, 1]],
                     [[1, 0, 0], [0, 1, 0], [0, 0, 1]]], np.float64) * 2 + o + np.array([[[0, 0, 0]], [[3, 0, 0]], [[6, 0, 0]], [[9, 0, 0]]])
  if kind == "planes":                                  # large tilted triangles through the whole grid
    out = []
    for _ in range(6):
      c = rng.uniform(0.2, 0.8, 3) * dims
      out.append(c + rng.uniform(-1.4, 1.4, (3, 3)) * dims)
    return np.array(out)
  if kind in ("tri5", "tri7", "one"):
    n = {"tri5": 5, "tri7": 7, "one": 1}[kind]
    c = rng.uniform(0.3, 0.7, (n, 1, 3)) * dims
    return c + rng.uniform(-0.45, 0.45, (n, 3, 3)) * dims
  raise KeyError(kind)


@dataclasses.dataclass
class Built:
  tri: np.ndarray          # f32 [T, 3, 3]
  num_tri: list
  v2v: np.ndarray          # f32 [M, 4, 4]


@functools.lru_cache(maxsize=None)
def build(c: Case) -> Built:
  D, H, W = c.grid
  dims = (W, H, D)
  tris, num, mats = [], [], []
  for m, parts in enumerate(c.meshes):
    rng = np.random.RandomState(1000 * c.seed + 17 * m + 5)
    ts = [np.asarray(_part(k, dims, rng), np.float64).reshape(-1, 3, 3) for k in parts]
    n = sum(len(x) for x in ts)
    tris += ts; num.append(n)
    A = np.eye(4)
    if c.mats == "affine":
      A[:3, :3] = _rot(0.4 + 0.5 * m, -0.3 + 0.2 * m, 0.7 - 0.4 * m) @ np.diag(np.array([0.41, 0.33, 0.27]) * np.array(dims))
      A[:3, 3] = np.array([0.5, 0.47, 0.52]) * np.array(dims)
    mats.append(A)
  tri = np.concatenate(tris).astype(np.float32) if tris else np.zeros((0, 3, 3), np.float32)
  return Built(tri, num, np.stack(mats).astype(np.float32))


CASES = _rows()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------------------------------- reference
def round_half_even(x: float) -> int:
  f = math.floor(x)
  r = x - f
  if r != 0.5:
    return f + (1 if r > 0.5 else 0)
  return f if f % 2 == 0 else f + 1


def raster_size(grid, mult, pdm) -> int:
  D, H, W = grid
  return round_half_even(max(W, H, D * pdm) * float(mult))


def _voxel_index(e, vs):
  """The grid index of coordinate e: floor, or the virtual-voxel rule of voxelize.frag:48-55."""
  if vs <= 0:
    return np.floor(e).astype(np.int64)
  v = np.floor(e * vs).astype(np.int64) + vs // 2
  return 2 * (v // vs) + (v % vs == vs - 1)


def band_arrays(tri, num_tri, v2v, grid, mult, pdm=1, cons=False, sub=False, closed=False):
  """(MUST, MAY) of one call.  closed: lattice points within tau of an edge line count as inside and decided (the union of two
  triangles that share that edge owns them exactly once under any consistent fill rule)."""
  D, H, W = grid
  tri = np.asarray(tri, np.float32).astype(np.float64).reshape(-1, 3, 3)
  A = np.asarray(v2v, np.float32).astype(np.float64)
  M = len(num_tri)
  if A.ndim == 2:
    A = np.broadcast_to(A, (M, 4, 4))
  mesh_of = np.repeat(np.arange(M), np.asarray(num_tri, np.int64))
  ext = np.array([W, H, D * pdm], np.float64)
  bound = np.array([W, H, D], np.float64)
  R = raster_size(grid, mult, pdm)
  vs = int(mult) if sub else -1
  shape = (2 * D + 1, 2 * H + 1, 2 * W + 1) if sub else (D, H, W)
  must = np.zeros((M,) + shape, bool)
  may = np.zeros((M,) + shape, bool)
  for t in range(tri.shape[0]):
    m = mesh_of[t]
    if not np.isfinite(tri[t]).all():
      continue
    P = tri[t] @ A[m, :3, :3].T + A[m, :3, 3]
    if not np.isfinite(P).all():
      continue
    n = np.cross(P[1] - P[0], P[2] - P[0])
    nn = np.linalg.norm(n)
    if nn == 0:
      continue
    a = np.abs(n) / nn
    axes = [k for k in range(3) if a.max() - a[k] <= TIE]
    tie = len(axes) > 1
    if tie:
      axes = sorted(set(axes) | {2})
    tau = 2.0 ** -18 * (np.abs(P).max() + ext.max())
    for d in axes:
      if n[d] == 0:
        continue
      u, v = ((1, 2), (2, 0), (0, 1))[d]
      cu, cv = ext[u] / R, ext[v] / R
      Q = P[:, [u, v]]
      pad = 3 if cons else 1
      lo_u = max(int(math.floor(Q[:, 0].min() / cu - 0.5)) - pad, 0); hi_u = min(int(math.ceil(Q[:, 0].max() / cu - 0.5)) + pad, R - 1)
      lo_v = max(int(math.floor(Q[:, 1].min() / cv - 0.5)) - pad, 0); hi_v = min(int(math.ceil(Q[:, 1].max() / cv - 0.5)) + pad, R - 1)
      if hi_u < lo_u or hi_v < lo_v:
        continue
      qu, qv = np.meshgrid((np.arange(lo_u, hi_u + 1) + 0.5) * cu, (np.arange(lo_v, hi_v + 1) + 0.5) * cv, indexing="ij")
      qu, qv = qu.ravel(), qv.ravel()
      s = 1.0 if n[d] > 0 else -1.0
      cand = np.ones(qu.shape, bool)
      dec = np.ones(qu.shape, bool)
      for i in range(3):
        p0, p1, p2 = Q[i], Q[(i + 1) % 3], Q[(i + 2) % 3]
        e = p1 - p0
        le = math.hypot(e[0], e[1])
        dist = s * (e[0] * (qv - p0[1]) - e[1] * (qu - p0[0])) / le
        if cons:
          reach = (0.5 * cu * abs(e[1]) + 0.5 * cv * abs(e[0])) / le
          height = s * (e[0] * (p2[1] - p0[1]) - e[1] * (p2[0] - p0[0])) / le
          cand &= dist + reach >= -tau
          dec &= (dist + reach > tau) & (dist - reach < height - tau)
        elif closed:
          cand &= dist >= -tau
          dec &= dist >= -tau
        else:
          cand &= dist > -tau
          dec &= dist > tau
      if cons:
        for q, c, k in ((qu, cu, 0), (qv, cv, 1)):
          cand &= (q >= Q[:, k].min() - 2 * c) & (q <= Q[:, k].max() + 2 * c)
          dec &= np.minimum(Q[:, k].max(), q + 0.5 * c) - np.maximum(Q[:, k].min(), q - 0.5 * c) > tau
      qu, qv, dec = qu[cand], qv[cand], dec[cand]
      if qu.size == 0:
        continue
      depth = P[0, d] - (n[u] * (qu - P[0, u]) + n[v] * (qv - P[0, v])) / n[d]
      t4 = 4 * tau
      pos = [None] * 3
      pos[u], pos[v], pos[d] = qu, qv, depth
      ends = [(p - t4, p + t4) for p in pos]
      clip = [(e >= 0) & (e <= ext[d]) for e in ends[d]]
      ok = [[(e >= 0) & (e < bound[k]) for e in ends[k]] for k in range(3)]
      idx = [[_voxel_index(np.where(o, e, 0.0), vs) for e, o in zip(ends[k], ok[k])] for k in range(3)]
      dec = dec & clip[0] & clip[1] & (not tie)
      for k in range(3):
        dec &= ok[k][0] & ok[k][1] & (idx[k][0] == idx[k][1])
      must[m, idx[2][0][dec], idx[1][0][dec], idx[0][0][dec]] = True
      alive = clip[0] | clip[1]
      for cx in (0, 1):
        for cy in (0, 1):
          for cz in (0, 1):
            w = alive & ok[0][cx] & ok[1][cy] & ok[2][cz]
            may[m, idx[2][cz][w], idx[1][cy][w], idx[0][cx][w]] = True
  assert not (must & ~may).any()
  return must, may


@functools.lru_cache(maxsize=None)
def band(c: Case):
  b = build(c)
  return band_arrays(b.tri, b.num_tri, b.v2v, c.grid, c.mult, c.pdm, c.cons, c.sub)


def shares(c: Case):
  """(|MUST|, row share, largest mesh share) of |MAY \\ MUST| / |MUST|."""
  must, may = band(c)
  nm, ne = must.reshape(len(must), -1).sum(1), (may & ~must).reshape(len(must), -1).sum(1)
  per = [e / n if n else (0.0 if e == 0 else math.inf) for n, e in zip(nm, ne)]
  tot = int(nm.sum())
  return tot, (float(ne.sum()) / tot if tot else (0.0 if ne.sum() == 0 else math.inf)), max(per) if per else 0.0


def share_table() -> str:
  """The lines of the module docstring's table, measured now."""
  out = []
  for c in CASES:
    tot, row, worst = shares(c)
    out.append(f"  {c.name:18s} |MUST| {tot:5d}   {100 * row:5.2f} %  ({100 * worst:5.2f} %)")
  return "\n".join(out)


def watertight_cases():
  """(name, triangles f32 [2, 3, 3], grid, multiplier): an axis-aligned quad of an 8^3 grid cut along a diagonal that passes through
  sample points ((k + 1/2) / multiplier on both screen axes), in each projection plane, along either diagonal, in both windings.
  The outer edges (at 1 and 6) and the depth (2.25) stay clear of the lattice and of the voxel borders."""
  out = []
  A, B, C, D = (1., 1.), (6., 1.), (6., 6.), (1., 6.)
  for mult in (1, 2):
    for d in range(3):
      u, v = ((1, 2), (2, 0), (0, 1))[d]
      for diag, pairs in (("main", ((A, B, C), (A, C, D))), ("anti", ((A, B, D), (B, C, D)))):
        for winding in (0, 1):
          tri = np.zeros((2, 3, 3), np.float32)
          for k, corners in enumerate(pairs):
            for i, (cu, cv) in enumerate(corners[::-1] if winding else corners):
              tri[k, i, u], tri[k, i, v], tri[k, i, d] = cu, cv, 2.25
          out.append((f"plane{d}_{diag}_w{winding}_m{mult}", tri, (8, 8, 8), mult))
  return out


# ------------------------------------------------------------------------------------------------- crn_transform_meshes
TRANSFORM_SHAPES = {            # name -> triangles per mesh
    "t0_m2": [0, 0], "t1": [1], "t86_m1": [86], "t86_empty_meshes": [30, 0, 0, 55, 1, 0], "t259": [100, 159],
}


def transform_inputs(num_tri, seed=0):
  """(triangles f32 [T, 3, 3] in [-1, 1]^3, tri_mesh i32 [T], matrices f32 [M, 4, 4]): perspective matrices whose w over the cube
  stays within 0.5 <= |w| <= 4, negative for every other mesh."""
  rng = np.random.RandomState(seed)
  T, M = int(sum(num_tri)), len(num_tri)
  tri = rng.uniform(-1, 1, (T, 3, 3)).astype(np.float32)
  mats = rng.uniform(-2, 2, (M, 4, 4))
  for m in range(M):
    row = rng.uniform(-1, 1, 3)
    mats[m, 3, :3] = 0.75 * row / np.abs(row).sum()                 # |a x + b y + c z| <= 0.75 on the cube
    mats[m, 3, 3] = (1.5, -1.25, 3.0, -3.25)[m % 4]
  return tri, np.repeat(np.arange(M), num_tri).astype(np.int32), mats.astype(np.float32)


def transform_reference(tri, tri_mesh, mats):
  """(float64 result, bound) per component: with N = sum_j |M_nj p_j| and Wn = sum_j |M_3j p_j| (p = (x, y, z, 1)),
  |got - ref| <= 2 * 2^-24 (3 N / |w| + |ref| (3 Wn / |w| + 1)): three fma roundings in each dot product, one for the quotient,
  doubled for the second-order terms."""
  p = np.concatenate([tri.astype(np.float64), np.ones(tri.shape[:2] + (1,))], -1)          # [T, 3, 4]
  A = mats.astype(np.float64)[tri_mesh]                                                     # [T, 4, 4]
  r = np.einsum("tnj,tvj->tvn", A, p)
  ra = np.einsum("tnj,tvj->tvn", np.abs(A), np.abs(p))
  w = r[..., 3:4]
  assert (np.abs(w) >= 0.5).all() and (np.abs(w) <= 4).all()
  ref = r[..., :3] / w
  bound = 2 * 2.0 ** -24 * (3 * ra[..., :3] / np.abs(w) + np.abs(ref) * (3 * ra[..., 3:4] / np.abs(w) + 1))
  return ref, bound


SHIFT_GRID, SHIFT_MULT = (16, 16, 16), 4


def dyadic_triangles(seed=2, n=24):
  """Triangles with coordinates k / 8 inside [5, 11]^3 of a 16^3 grid (every fp32 operation up to the edge values is exact there);
  translated by up to +-4 whole voxels they stay inside the grid.  Coverage is then decided by exact numbers, so a translation by
  whole voxels and pixels must move the result without changing it; only the interpolated position rounds differently (a few
  2^-24 of 16), which could move a voxel only for a fragment that close to a voxel border: tests/test_voxelize_ref_cpu.py shows on
  the oracle that these triangles have none."""
  rng = np.random.RandomState(seed)
  return (rng.randint(40, 89, (n, 3, 3)) / 8.0).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ the oracle
def oracle(c: Case, tri=None, v2v=None, grid=None, mult=None, pdm=None, cons=None):
  """O.voxelize_mesh on the row, with arguments replaced from the outside (the seeded wrong oracles)."""
  b = build(c)
  return O.voxelize_mesh(b.tri if tri is None else tri, b.num_tri, c.grid if grid is None else grid, b.v2v if v2v is None else v2v,
                         sub_grid_sampling=c.sub, image_resolution_multiplier=c.mult if mult is None else mult,
                         conservative_rasterization=c.cons if cons is None else cons,
                         projection_depth_multiplier=c.pdm if pdm is None else pdm)


def in_band(c: Case, got) -> Tuple[int, int]:
  """(MUST voxels the result misses, result voxels outside MAY)."""
  must, may = band(c)
  g = np.asarray(got) != 0
  assert g.shape == must.shape, (g.shape, must.shape)
  return int((must & ~g).sum()), int((g & ~may).sum())


# ---------------------------------------------------------------------------------------------------------------- GPU side
def run_kernel(be, c: Case, dev, tri=None, num_tri=None, v2v=None, garbage=7.5):
  """crn_voxelize_mesh on the row.  The grid is a view into a wider storage: the view starts as garbage (the entry's clear has to
  remove it), the tail holds the sentinel.  Returns (grid as numpy, storage tail as int32 bits, expected tail bits)."""
  import torch as t
  from corenet_amd.geometry import voxelization
  b = build(c) if tri is None or num_tri is None or v2v is None else None
  tri = t.as_tensor(b.tri if tri is None else tri, dtype=t.float32)
  num_tri = b.num_tri if num_tri is None else num_tri
  v2v = t.as_tensor(b.v2v if v2v is None else v2v, dtype=t.float32)
  D, H, W = c.grid
  M = len(num_tri)
  shape = (M, 2 * D + 1, 2 * H + 1, 2 * W + 1) if c.sub else (M, D, H, W)
  n = int(np.prod(shape))
  st = t.full((n + TAIL,), SENTINEL, dtype=t.float32, device=dev)
  st[:n] = garbage
  st[:n:3] = float("nan")
  tm = voxelization.dynamic_tile(t.as_tensor(num_tri, dtype=t.int32)).to(dev)
  be.voxelize_mesh(tri.to(dev).contiguous(), tm, v2v.to(dev).contiguous(), M, D, H, W, int(c.mult) if c.sub else 0, c.mult, c.cons,
                   c.pdm, st[:n].view(shape))
  t.cuda.synchronize()
  want_tail = t.full((TAIL,), SENTINEL, dtype=t.float32).view(t.int32)
  return st[:n].view(shape).cpu().numpy(), st[n:].cpu().view(t.int32), want_tail
