"""The ground-truth voxelizer and label path (csrc/voxelize.hip: crn_voxelize_mesh, crn_merge_labels, crn_transform_meshes) on the
GPU, every row of tests/voxelize_cases.py: bit-equal to the oracle AND inside the band of the independent float64 reference
(MUST <= kernel <= MAY), the grid a view into a wider storage whose tail must come back bit-identical and whose garbage the entry
has to clear.  The fill rule on the sample lattice, conservative >= plain, invariance under triangle order / vertex rotation /
winding, translation by whole voxels, voxelize_labels end to end in sub-grid mode on a non-cubic grid; crn_transform_meshes with
perspective matrices against float64 within the derived bound of tests/voxelize_cases.py; crn_merge_labels at its edge shapes; and
rejected argument sets (CRN_EINVAL, nothing written).  tests/test_voxelize_ref_cpu.py validates the reference and the rows."""
import dataclasses
import functools
import time

import numpy as np
import pytest
import torch as t

import voxelize_cases as K
from voxelize_cases import CASES, BY_NAME
from kernel_contract_emu import EmuBackend
from oracle import corenet_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
EMU = EmuBackend()
EINVAL = -1
RATIO = {}


@pytest.fixture(scope="module")
def be():
  t0 = time.time()
  from corenet_amd.backend import HipBackend
  assert t.cuda.is_available(), "gpu tests need an MI355X"
  yield HipBackend()
  for k in sorted(RATIO):
    print(f"\ncrn_transform_meshes {k}: largest err / bound {RATIO[k]:.3f}")
  print(f"\n  module wall time {time.time() - t0:.1f} s")


@functools.lru_cache(maxsize=None)
def oracle(name):
  g = K.oracle(BY_NAME[name])
  g.setflags(write=False)
  return g


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------------ rows
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_row(be, name):
  c = BY_NAME[name]
  got, tail, want_tail = K.run_kernel(be, c, DEV)
  assert t.equal(tail, want_tail), f"{name}: the storage behind the grid changed"
  assert not np.isnan(got).any() and set(np.unique(got)) <= {0.0, 1.0}, f"{name}: the entry's clear left garbage in the grid"
  diff = int((_bits(got) != _bits(oracle(name))).sum())
  miss, extra = K.in_band(c, got)
  print(f"{name}: {int(got.sum())} voxels, {diff} differ from the oracle, {miss} decided voxels missing, {extra} outside MAY")
  assert miss == 0 and extra == 0, f"{name}: {miss} decided voxels missing, {extra} voxels outside every outcome of the reference"
  assert diff == 0, f"{name}: {diff} voxels differ from the oracle"


def test_non_finite_vertices_change_nothing(be):
  a = K.run_kernel(be, BY_NAME["nonfinite"], DEV)[0]
  b = K.run_kernel(be, BY_NAME["finite_twin"], DEV)[0]
  assert b.sum() > 400 and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------------ properties
def _run(be, tri, grid, mult, cons=False, num_tri=None, v2v=None):
  c = K.Case("adhoc", grid, mult, (), cons=cons)
  num_tri = [len(tri)] if num_tri is None else num_tri
  v2v = np.tile(np.eye(4, dtype=np.float32), (len(num_tri), 1, 1)) if v2v is None else v2v
  got, tail, want_tail = K.run_kernel(be, c, DEV, tri=tri, num_tri=num_tri, v2v=v2v)
  assert t.equal(tail, want_tail)
  return got


@pytest.mark.parametrize("name", [w[0] for w in K.watertight_cases()])
def test_watertight_on_the_lattice(be, name):
  _, tri, grid, mult = next(w for w in K.watertight_cases() if w[0] == name)
  must, may = K.band_arrays(tri, [2], np.eye(4, dtype=np.float32), grid, mult, closed=True)
  assert np.array_equal(must, may)
  got = _run(be, tri, grid, mult, num_tri=[2]) != 0
  assert np.array_equal(got, must), f"{name}: {int((got != must).sum())} voxels differ"
  if mult == 1:
    halves = [_run(be, tri[k:k + 1], grid, mult) != 0 for k in (0, 1)]
    assert not (halves[0] & halves[1]).any(), "a sample on the diagonal is rasterized twice"


@pytest.mark.parametrize("name", [c.name for c in CASES if not c.cons])
def test_conservative_contains_plain(be, name):
  c = BY_NAME[name]
  plain = K.run_kernel(be, c, DEV)[0]
  cons = K.run_kernel(be, dataclasses.replace(c, cons=True), DEV)[0]
  assert not ((plain != 0) & (cons == 0)).any()
  assert c.tiny or cons.sum() > plain.sum()


@pytest.mark.parametrize("name", ["w14_m4", "d12_m3_pdm2_cons", "sub5_cons", "affine_m4", "c7_m15"])
def test_triangle_order_vertex_rotation_and_winding(be, name):
  c = BY_NAME[name]
  b = K.build(c)
  base = K.run_kernel(be, c, DEV)[0]
  rng = np.random.RandomState(3)
  order = np.concatenate([o + rng.permutation(n) for o, n in zip(np.cumsum([0] + b.num_tri[:-1]), b.num_tri)]).astype(np.int64)
  assert not np.array_equal(order, np.arange(len(order)))
  shuffled = K.run_kernel(be, c, DEV, tri=b.tri[order])[0]
  assert np.array_equal(_bits(shuffled), _bits(base)), f"{name}: the result depends on the order of the triangles"
  for what, perm in (("rotated", [1, 2, 0]), ("rotated twice", [2, 0, 1]), ("reversed", [0, 2, 1])):
    got = K.run_kernel(be, c, DEV, tri=np.ascontiguousarray(b.tri[:, perm]))[0]
    miss, extra = K.in_band(c, got)
    print(f"{name}, vertices {what}: {int((got != base).sum())} voxels differ from the given order")
    assert miss == 0 and extra == 0, (name, what, miss, extra)


@pytest.mark.parametrize("cons", [False, True])
def test_translation_by_whole_voxels_is_a_shift(be, cons):
  tri = K.dyadic_triangles()
  base = _run(be, tri, K.SHIFT_GRID, K.SHIFT_MULT, cons)
  assert base.sum() > 100
  for axis in range(3):
    for s in (-4, 3):
      moved = tri.copy()
      moved[:, :, axis] += s
      got = _run(be, moved, K.SHIFT_GRID, K.SHIFT_MULT, cons)
      assert np.array_equal(_bits(got), _bits(np.roll(base, s, axis=3 - axis))), (axis, s)


def test_voxelize_labels_sub_grid_non_cubic(be):
  """voxelize_labels on a non-cubic grid in sub-grid mode against oracle raster -> C fill oracle -> sub-grid centres -> oracle merge."""
  import fill_oracle_c
  from corenet_amd.data import batched_example as B
  res = (5, 8, 6)
  D, H, W = res
  m = float(max(res))
  off = t.tensor([[0.5, 0.5, 0.5], [0.25, 0.75, 0.375]])
  dims = np.array([W, H, D], float)
  rng = np.random.RandomState(0)
  vox = [K._part("ellipsoid", dims, rng), K._part("ellipsoid2", dims, rng), K._part("ellipsoid", dims, rng) * 0.8 + 0.1 * dims]
  scene_of = [0, 0, 1]
  verts = np.concatenate([(v - (off[s].numpy().astype(np.float64) - 0.5)) / m for v, s in zip(vox, scene_of)]).astype(np.float32)
  nt = [t.tensor([len(vox[0]), len(vox[1])], dtype=t.int32), t.tensor([len(vox[2])], dtype=t.int32)]
  labels = [[3, 5], [2]]
  kw = dict(sub_grid_sampling=True, conservative_rasterization=True, image_resolution_multiplier=5)
  got = B.voxelize_labels(t.tensor(verts).to(DEV), nt, labels, off, res, **kw).cpu().numpy()
  v2v = B.view2voxel_matrices(off, res).numpy()
  ref = O.voxelize_mesh(verts, [len(v) for v in vox], res, v2v[scene_of], **kw)
  want = O.merge_labels(O.get_sub_grid_centers(fill_oracle_c.fill(ref)), [2, 1], labels)
  assert got.shape == (2, D, H, W) and got.dtype == np.int32
  assert set(np.unique(want)) == {0, 2, 3, 5}
  np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------------------------------- crn_transform_meshes
def _transform(be, tri, tm, mats, in_place):
  n = tri.size
  src = t.full((n + K.TAIL,), K.SENTINEL, dtype=t.float32, device=DEV)
  src[:n] = t.as_tensor(tri).reshape(-1).to(DEV)
  dst = src if in_place else t.full((n + K.TAIL,), K.SENTINEL, dtype=t.float32, device=DEV)
  be.transform_meshes(src[:n].view(-1, 3, 3), t.as_tensor(tm).to(DEV), t.as_tensor(mats).to(DEV), dst[:n].view(-1, 3, 3))
  t.cuda.synchronize()
  assert bool((dst[n:] == K.SENTINEL).all()), "the storage behind the output changed"
  if not in_place:
    assert t.equal(src[:n].cpu().view(t.int32), t.as_tensor(tri).reshape(-1).view(t.int32)), "the input changed"
  return dst[:n].view(-1, 3, 3).cpu().numpy()


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("name", list(K.TRANSFORM_SHAPES))
def test_transform_meshes_perspective(be, name, in_place):
  num = K.TRANSFORM_SHAPES[name]
  tri, tm, mats = K.transform_inputs(num)
  got = _transform(be, tri, tm, mats, in_place)
  if tri.shape[0] == 0:
    assert got.shape == (0, 3, 3)
    return
  ref, bound = K.transform_reference(tri, tm, mats)
  assert len(num) == 1 or (mats[np.unique(tm), 3, 3] < 0).any(), "some mesh has negative w"
  ratio = float((np.abs(got.astype(np.float64) - ref) / bound).max())
  RATIO[name] = max(RATIO.get(name, 0.0), ratio)
  print(f"{name} (in place {in_place}): err / bound {ratio:.3f}")
  assert ratio <= 1.0, f"{name}: {ratio:.3f} of the bound"
  emu = np.empty_like(tri)
  EMU.transform_meshes(t.as_tensor(tri), t.as_tensor(tm), t.as_tensor(mats), t.as_tensor(emu))
  assert float((np.abs(emu.astype(np.float64) - ref) / bound).max()) <= 1.0


# ----------------------------------------------------------------------------------------------------- crn_merge_labels
MERGE = {      # name -> ((D, H, W), sub-grid, meshes per scene)
    "one_voxel": ((1, 1, 1), False, [3, 0, 1]),
    "one_voxel_sub": ((1, 1, 1), True, [2, 1]),
    "sub_non_cubic": ((5, 8, 6), True, [3, 1, 0, 4]),
    "scene_of_40": ((6, 10, 14), False, [40, 2]),
    "one_scene": ((12, 5, 9), False, [5]),
    "one_scene_sub": ((3, 7, 5), True, [1]),
}


@pytest.mark.parametrize("name", list(MERGE))
def test_merge_labels(be, name):
  (D, H, W), sub, num = MERGE[name]
  g = t.Generator().manual_seed(len(name))
  Mn, B = sum(num), len(num)
  shape = (Mn, 2 * D + 1, 2 * H + 1, 2 * W + 1) if sub else (Mn, D, H, W)
  grids = (t.rand(shape, generator=g) < 0.35).float()
  flat = t.randint(0, 9, (Mn,), generator=g, dtype=t.int32)             # label 0 and repeated labels among 40 meshes
  if Mn >= 40:
    assert int((flat == 0).sum()) >= 1 and len(set(flat[:40].tolist())) < 40
  start = t.tensor(np.concatenate([[0], np.cumsum(num)]).astype(np.int32))
  n = B * D * H * W
  st = t.full((n + K.TAIL,), -7, dtype=t.int32, device=DEV)
  out = st[:n].view(B, D, H, W)
  be.merge_labels(grids.to(DEV), start.to(DEV), flat.to(DEV), B, D, H, W, sub, out)
  t.cuda.synchronize()
  assert bool((st[n:] == -7).all()), "the storage behind the output changed"
  got = out.cpu()
  centers = O.get_sub_grid_centers(grids.numpy()) if sub else grids.numpy()
  off = 0
  for b, k in enumerate(num):
    want = O.merge_labels(centers[off:off + k], [k], [flat[off:off + k].tolist()])[0] if k else np.zeros((D, H, W), np.int32)
    np.testing.assert_array_equal(got[b].numpy(), want)
    off += k
  emu = t.zeros((B, D, H, W), dtype=t.int32)
  EMU.merge_labels(grids, start, flat, B, D, H, W, sub, emu)
  assert t.equal(got, emu)


# --------------------------------------------------------------------------------------------------- argument rejection
def test_rejected_calls_write_nothing(be):
  """CRN_EINVAL before anything is written or launched: every output keeps its sentinel."""
  from corenet_amd import _lib
  L = be.lib
  st = _lib.stream()
  D, H, W, M, T = 3, 4, 5, 2, 6
  tri = t.rand(T, 3, 3, device=DEV) * 3
  tm = t.tensor([0, 0, 0, 1, 1, 1], dtype=t.int32, device=DEV)
  v2v = t.eye(4, device=DEV).repeat(M, 1, 1).contiguous()
  grid = t.full((M * 7 * 9 * 11 + K.TAIL,), K.SENTINEL, device=DEV)
  good = dict(tri=tri.data_ptr(), tm=tm.data_ptr(), T=T, v2v=v2v.data_ptr(), M=M, D=D, H=H, W=W, sub=0, mult=4.0, cons=0, pdm=1,
              grid=grid.data_ptr())
  def vox(**kw):
    a = dict(good, **kw)
    return L._crn_voxelize_mesh(a["tri"], a["tm"], a["T"], a["v2v"], a["M"], a["D"], a["H"], a["W"], a["sub"], a["mult"], a["cons"],
                                a["pdm"], a["grid"], st)
  bad = [dict(tri=None), dict(tm=None), dict(v2v=None), dict(grid=None), dict(pdm=0), dict(pdm=-1), dict(D=0), dict(H=0), dict(W=-1),
         dict(M=0), dict(T=-1), dict(sub=4, mult=4.0), dict(sub=2, mult=2.0)]
  for kw in bad:
    assert vox(**kw) == EINVAL, kw
  t.cuda.synchronize()
  assert bool((grid == K.SENTINEL).all()), "a rejected crn_voxelize_mesh call wrote to the grid"
  # T = 0 needs no triangle pointers: the grid is cleared, nothing else
  assert vox(tri=None, tm=None, v2v=None, T=0) == 0
  t.cuda.synchronize()
  n = M * D * H * W
  assert bool((grid[:n] == 0).all()) and bool((grid[n:] == K.SENTINEL).all())
  assert vox() == 0

  B = 2
  mg = (t.rand(3, D, H, W, device=DEV) < 0.5).float()
  start = t.tensor([0, 2, 3], dtype=t.int32, device=DEV)
  lab = t.tensor([4, 2, 7], dtype=t.int32, device=DEV)
  out = t.full((B * D * H * W + K.TAIL,), -7, dtype=t.int32, device=DEV)
  goodm = dict(mg=mg.data_ptr(), start=start.data_ptr(), lab=lab.data_ptr(), B=B, D=D, H=H, W=W, sub=0, out=out.data_ptr())
  def merge(**kw):
    a = dict(goodm, **kw)
    return L._crn_merge_labels(a["mg"], a["start"], a["lab"], a["B"], a["D"], a["H"], a["W"], a["sub"], a["out"], st)
  for kw in (dict(mg=None), dict(start=None), dict(lab=None), dict(out=None), dict(B=0), dict(D=0), dict(H=-2), dict(W=0)):
    assert merge(**kw) == EINVAL, kw
  t.cuda.synchronize()
  assert bool((out == -7).all()), "a rejected crn_merge_labels call wrote to the output"
  assert merge() == 0

  dst = t.full((T * 9 + K.TAIL,), K.SENTINEL, device=DEV)
  mats = v2v
  def tf(tri_=tri.data_ptr(), tm_=tm.data_ptr(), T_=T, mats_=mats.data_ptr(), M_=M, out_=dst.data_ptr()):
    return L._crn_transform_meshes(tri_, tm_, T_, mats_, M_, out_, st)
  for kw in (dict(tri_=None), dict(tm_=None), dict(mats_=None), dict(out_=None), dict(T_=-1), dict(M_=-1)):
    assert tf(**kw) == EINVAL, kw
  t.cuda.synchronize()
  assert bool((dst == K.SENTINEL).all()), "a rejected crn_transform_meshes call wrote to the output"
  assert tf(tri_=None, tm_=None, mats_=None, out_=None, T_=0) == 0 and tf() == 0
  t.cuda.synchronize()


def test_wrapper_rejects_depth_multiplier_below_one(be):
  from corenet_amd.geometry import voxelization as V
  tri = t.rand(4, 3, 3)
  for pdm in (0, -1):
    with pytest.raises(ValueError):
      V.voxelize_mesh(tri, [4], (3, 3, 3), t.eye(4), projection_depth_multiplier=pdm)
  assert V.voxelize_mesh(tri * 3, [4], (3, 3, 3), t.eye(4), projection_depth_multiplier=2).shape == (1, 3, 3, 3)
