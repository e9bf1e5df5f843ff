"""CPU side of tests/voxelize_cases.py (the ground-truth voxelizer, csrc/voxelize.hip): the oracle the kernel is bit-equal to lies
inside the band of the independent float64 reference on every row, the band is tight (cap and floor, from the reference alone),
the fill rule is watertight on the sample lattice, conservative coverage contains plain coverage, seeded wrong oracles leave the
band on rows named here, and the host logic of the Python wrapper follows the reference.  No GPU."""
import functools

import numpy as np
import pytest
import torch as t

import voxelize_cases as K
from voxelize_cases import CASES, BY_NAME
from oracle import corenet_oracle as O

NAMES = [c.name for c in CASES]


@functools.lru_cache(maxsize=None)
def oracle(name):
  g = K.oracle(BY_NAME[name])
  g.setflags(write=False)
  return g


# ------------------------------------------------------------------------------------------------------------------ band
@pytest.mark.parametrize("name", NAMES)
def test_oracle_inside_band(name):
  c = BY_NAME[name]
  miss, extra = K.in_band(c, oracle(name))
  tot, row, worst = K.shares(c)
  print(f"{name}: |MUST| {tot}, |MAY - MUST| / |MUST| {100 * row:.2f} % (largest mesh {100 * worst:.2f} %), oracle misses {miss}, "
        f"outside {extra}")
  assert miss == 0, f"{name}: the oracle misses {miss} voxels the reference decides"
  assert extra == 0, f"{name}: the oracle marks {extra} voxels no outcome of the reference reaches"
  assert set(np.unique(oracle(name))) <= {0.0, 1.0}


@pytest.mark.parametrize("name", NAMES)
def test_band_is_tight(name):
  """From the reference alone: |MAY - MUST| <= 5 % of |MUST| per row and per mesh, |MUST| >= 200 per row; the rows of at most one
  triangle cannot reach the floor and have no undecided voxel at all."""
  c = BY_NAME[name]
  must, may = K.band(c)
  tot, row, worst = K.shares(c)
  if c.tiny:
    assert np.array_equal(must, may)
    assert len(K.build(c).tri) <= 1
    return
  assert tot >= K.FLOOR, (name, tot)
  assert row <= K.CAP and worst <= K.CAP, (name, row, worst)


def test_recorded_shares_are_the_measured_ones():
  for line in K.share_table().splitlines():
    assert line in K.__doc__, f"tests/voxelize_cases.py docstring: expected the line {line!r}"


def test_rows_cover_the_issue():
  grids = {c.grid for c in CASES}
  assert {(6, 10, 14), (12, 5, 9), (5, 16, 8), (4, 4, 20), (3, 3, 3), (7, 7, 7)} <= grids
  assert {1, 1.5, 3, 4, 8} <= {c.mult for c in CASES if not c.sub}
  assert {3, 5, 9} <= {c.mult for c in CASES if c.sub} and all(len(set(c.grid)) == 3 for c in CASES if c.sub)
  pdm2 = [c for c in CASES if c.pdm == 2]
  assert any(c.grid[0] * 2 > max(c.grid[1:]) for c in pdm2) and any(c.grid[0] * 2 < max(c.grid[1:]) for c in pdm2)
  assert K.build(BY_NAME["list_5_0_7_0"]).num_tri == [5, 0, 7, 0]
  assert K.build(BY_NAME["t0_m2"]).num_tri == [0, 0] and len(K.build(BY_NAME["t1"]).tri) == 1
  assert len(K.build(BY_NAME["w14_m4"]).tri) % 4 == 1
  assert all(len(K.build(c).tri) <= 420 for c in CASES)
  for c in CASES:                       # the x 1.5 products end in .5 and round to even
    if c.mult == 1.5:
      assert (max(c.grid) * 1.5) % 1 == 0.5 and K.raster_size(c.grid, c.mult, c.pdm) % 2 == 0
    assert K.raster_size(c.grid, c.mult, c.pdm) == int(round(max(c.grid[2], c.grid[1], c.grid[0] * c.pdm) * c.mult))


def test_meshes_are_what_they_claim():
  c = BY_NAME["w14_m4"]
  D, H, W = c.grid
  dims = np.array([W, H, D], float)
  rng = np.random.RandomState(0)
  sl = K._part("slivers", dims, rng)
  for a, b, cc in sl:
    longest = max(np.linalg.norm(b - a), np.linalg.norm(cc - a), np.linalg.norm(cc - b))
    height = np.linalg.norm(np.cross(b - a, cc - a)) / longest
    assert longest / height >= 1000
  cr = K._part("cross", dims, rng)
  lo, hi = cr.min(1), cr.max(1)
  for ax in range(3):                   # every face is straddled by some triangle
    assert ((lo[:, ax] < 0) & (hi[:, ax] > 0)).any() and ((lo[:, ax] < dims[ax]) & (hi[:, ax] > dims[ax])).any()
  big = K._part("big", dims, rng)[0]
  assert (np.abs(big) <= 4 * dims.max()).all() and (big >= -3 * dims).all() and (big <= 4 * dims).all()
  one = BY_NAME["w14_m4"]
  must, _ = K.band_arrays(big[None].astype(np.float32), [1], np.eye(4, dtype=np.float32), one.grid, one.mult)
  assert must.any(0).any(0).all(), "the raster-spanning triangle reaches every (y, x) column of the grid"
  for tri in K._part("degenerate", dims, rng):
    assert np.linalg.norm(np.cross(tri[1] - tri[0], tri[2] - tri[0])) == 0
  assert (K._part("negative", dims, rng) < 0).all()
  must, may = K.band(c)
  assert not may[2].any(), "the mesh at negative coordinates marks nothing"
  normals = [np.cross(x[1] - x[0], x[2] - x[0]) for x in K._part("ties", (16, 16, 16), rng)]
  got = sorted(tuple(int(v) for v in np.abs(n) / np.abs(n).max()) for n in normals)
  assert got == [(0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1)]


def test_non_finite_vertices_change_nothing():
  """Triangles with a NaN, +Inf or -Inf vertex among finite ones: exactly the result of the finite triangles alone."""
  a, b = BY_NAME["nonfinite"], BY_NAME["finite_twin"]
  ta, tb = K.build(a).tri, K.build(b).tri
  assert (~np.isfinite(ta)).sum() == 6 and np.isfinite(tb).all() and len(ta) == len(tb) + 6
  assert np.array_equal(ta[np.isfinite(ta).all((1, 2))], tb)
  assert np.array_equal(oracle("nonfinite"), oracle("finite_twin"))
  assert all(np.array_equal(x, y) for x, y in zip(K.band(a), K.band(b)))


# ------------------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("name", [w[0] for w in K.watertight_cases()])
def test_watertight_on_the_lattice(name):
  """Two triangles whose shared diagonal passes exactly through sample points (dyadic coordinates: fp32 is exact): every sample on
  the diagonal belongs to exactly one of them, whatever the plane and the winding -- the top-left rule through the y flip."""
  _, tri, grid, mult = next(w for w in K.watertight_cases() if w[0] == name)
  eye = np.eye(4, dtype=np.float32)
  must, may = K.band_arrays(tri, [2], eye, grid, mult, closed=True)
  assert np.array_equal(must, may), "the quad is chosen so that nothing but the diagonal lies on an edge"
  open_must, _ = K.band_arrays(tri, [2], eye, grid, mult)
  got = O.voxelize_mesh(tri, [2], grid, eye, image_resolution_multiplier=mult) != 0
  assert np.array_equal(got, must), f"{name}: {int((got != must).sum())} voxels differ"
  if mult == 1:                          # one sample per voxel
    assert (must & ~open_must).sum() == 5, "the diagonal carries five samples"
    halves = [O.voxelize_mesh(tri[k:k + 1], [1], grid, eye, image_resolution_multiplier=mult) != 0 for k in (0, 1)]
    assert not (halves[0] & halves[1]).any(), "a sample on the diagonal is rasterized twice"


@pytest.mark.parametrize("name", NAMES)
def test_conservative_contains_plain(name):
  c = BY_NAME[name]
  plain = oracle(name) if not c.cons else K.oracle(c, cons=False)
  cons = oracle(name) if c.cons else K.oracle(c, cons=True)
  assert not ((plain != 0) & (cons == 0)).any()


@pytest.mark.parametrize("cons", [False, True])
def test_translation_by_whole_voxels_is_a_shift(cons):
  tri = K.dyadic_triangles()
  eye = np.eye(4, dtype=np.float32)
  kw = dict(image_resolution_multiplier=K.SHIFT_MULT, conservative_rasterization=cons)
  base = O.voxelize_mesh(tri, [len(tri)], K.SHIFT_GRID, eye, **kw)
  miss, extra = (lambda mm: (int((mm[0] & (base == 0)).sum()), int(((base != 0) & ~mm[1]).sum())))(
      K.band_arrays(tri, [len(tri)], eye, K.SHIFT_GRID, K.SHIFT_MULT, cons=cons))
  assert base.sum() > 100 and miss == 0 and extra == 0
  for axis in range(3):
    for s in (-4, 3):
      moved = tri.copy()
      moved[:, :, axis] += s
      got = O.voxelize_mesh(moved, [len(tri)], K.SHIFT_GRID, eye, **kw)
      assert np.array_equal(got, np.roll(base, s, axis=3 - axis)), (axis, s)


# -------------------------------------------------------------------------------------------------- seeded wrong oracles
def _left(c, got):
  miss, extra = K.in_band(c, got)
  return miss + extra


def test_seeded_raster_size_off_by_one():
  for name in ("w14_m4", "c7_m15", "c3_m15", "c7p_m15_cons"):
    c = BY_NAME[name]
    ext, R = max(c.grid[2], c.grid[1], c.grid[0] * c.pdm), K.raster_size(c.grid, c.mult, c.pdm)
    for r in (R - 1, R + 1):
      assert _left(c, K.oracle(c, mult=r / ext)) > 0, (name, r)


def test_seeded_h_w_exchanged():
  c = BY_NAME["w14_m4"]
  D, H, W = c.grid
  assert _left(c, K.oracle(c, grid=(D, W, H)).transpose(0, 1, 3, 2)) > 0


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_seeded_half_pixel_shift(axis):
  for name in ("w14_m4", "d12_m3_pdm2_cons", "sub5"):
    c = BY_NAME[name]
    D, H, W = c.grid
    v2v = K.build(c).v2v.copy()
    v2v[:, axis, 3] += 0.5 * (W, H, D * c.pdm)[axis] / K.raster_size(c.grid, c.mult, c.pdm)
    assert _left(c, K.oracle(c, v2v=v2v)) > 0, name


def test_seeded_pdm_ignored():
  for name in ("d12_m3_pdm2", "d12_m3_pdm2_cons", "w20_m3_pdm2"):
    assert _left(BY_NAME[name], K.oracle(BY_NAME[name], pdm=1)) > 0, name


def test_seeded_conservative_flag_inverted():
  for name in ("w14_m4", "w14_m4_cons", "c3_m15", "c3_m15_cons", "sub9_cons"):
    c = BY_NAME[name]
    assert _left(c, K.oracle(c, cons=not c.cons)) > 0, name


def test_seeded_matrices_transposed():
  for name in ("affine_m4", "affine_m4_cons"):
    c = BY_NAME[name]
    assert _left(c, K.oracle(c, v2v=np.ascontiguousarray(K.build(c).v2v.transpose(0, 2, 1)))) > 0, name


# ------------------------------------------------------------------------------------------------------------ host logic
def test_wrapper_errors_and_expansion():
  """voxelization.py:98-113: shapes, the (4, 4) -> (M, 4, 4) expansion, the two ValueErrors of the reference, and a depth
  multiplier below 1.  Everything is decided before the GPU is touched."""
  from corenet_amd.geometry import voxelization as V
  tri = np.zeros((5, 3, 3), np.float32)
  eye = np.eye(4, dtype=np.float32)
  a, n, m = V.check_arguments(tri, [2, 0, 3], 2 * eye, False, 4, 1)
  assert a.dtype == t.float32 and a.shape == (5, 3, 3) and n.dtype == t.int32 and n.tolist() == [2, 0, 3]
  assert m.shape == (3, 4, 4) and m.dtype == t.float32 and bool((m == t.as_tensor(2 * eye)).all())
  per_mesh = np.stack([eye, 2 * eye, 3 * eye])
  assert t.equal(V.check_arguments(tri, [2, 0, 3], per_mesh, False, 4, 1)[2], t.as_tensor(per_mesh))
  a64, n64, _ = V.check_arguments(tri.astype(np.float64), t.tensor([5], dtype=t.int64), eye.astype(np.float64), True, 3, 1)
  assert a64.dtype == t.float32 and n64.dtype == t.int32
  for bad in (lambda: V.check_arguments(np.zeros((5, 3, 2), np.float32), [5], eye, False, 4, 1),
              lambda: V.check_arguments(tri, [[5]], eye, False, 4, 1),
              lambda: V.check_arguments(tri, [2, 3], per_mesh, False, 4, 1)):
    with pytest.raises(AssertionError):
      bad()
  for mult in (2, 4, 8):
    with pytest.raises(ValueError):
      V.voxelize_mesh(tri, [5], (3, 3, 3), eye, sub_grid_sampling=True, image_resolution_multiplier=mult)
    with pytest.raises(ValueError):
      O.voxelize_mesh(tri, [5], (3, 3, 3), eye, sub_grid_sampling=True, image_resolution_multiplier=mult)
  with pytest.raises(ValueError):
    V.voxelize_mesh(tri, [5], (3, 3, 3), eye, sub_grid_sampling=True, image_resolution_multiplier=3, projection_depth_multiplier=0)
  for pdm in (0, -1):
    with pytest.raises(ValueError):
      V.voxelize_mesh(tri, [5], (3, 3, 3), eye, projection_depth_multiplier=pdm)
  V.check_arguments(tri, [5], eye, True, 3, 2)
  V.check_arguments(tri, [5], eye, False, 1.5, 1)


def test_dynamic_tile_with_empty_partitions():
  from corenet_amd.geometry import voxelization as V
  for lens in ([5, 0, 7, 0], [0, 0], [0, 3], [1], []):
    got = V.dynamic_tile(t.tensor(lens, dtype=t.int32))
    assert got.dtype == t.int32 and got.tolist() == [i for i, n in enumerate(lens) for _ in range(n)]


def test_view2voxel_matrices():
  """batched_example.py:153-163 on non-cubic grids: translate(offset - 0.5) . scale(max(D, H, W)), in float64."""
  from corenet_amd.data import batched_example as B
  off = t.tensor([[0.5, 0.5, 0.5], [0.25, 0.75, 0.0], [1.0, 0.0, 0.625]])
  for res in ((6, 10, 14), (12, 5, 9), (5, 16, 8), (7, 7, 7)):
    got = B.view2voxel_matrices(off, res)
    assert got.shape == (3, 4, 4) and got.dtype == t.float32
    for b in range(3):
      want = np.eye(4)
      want[:3, 3] = off[b].double().numpy() - 0.5
      want = want @ np.diag([max(res)] * 3 + [1.0])
      assert np.array_equal(got[b].double().numpy(), want)
    assert t.equal(got, O.view2voxel_matrices(off, res))
