"""corenet_amd.mesh_ops on the GPU against its host twin (which tests/test_mesh_ops_cpu.py anchors against numpy), bit for
bit, on the meshes of tests/mesh_ops_check.py: they sit on every seam mesh_ops_tiles() reports."""
import numpy as np
import pytest
import torch as t

import mesh_check as MC
import mesh_ops_check as K
from corenet_amd import mesh_ops as M
from corenet_amd import visualization as VZ

pytestmark = pytest.mark.gpu

TILES = M.mesh_ops_tiles()
CASES = K.cases(TILES)
DECIMATION = K.decimation_cases(TILES)
TOPOLOGY_FIELDS = ("vertex_offsets", "face_offsets", "vf_offsets", "vf_corners", "vv_offsets", "vv_neighbours", "irregular")
_twin = {}


def twin_topology(name):
  if name not in _twin:
    _, f, nv, nf = CASES[name]
    _twin[name] = M.mesh_topology(f, nv, nf)
  return _twin[name]


def gpu_topology(name, device_counts=False):
  v, f, nv, nf = CASES[name]
  if device_counts:
    return M.mesh_topology(f.cuda(), nv.cuda(), nf.cuda(), total_vertices=v.shape[0])
  return M.mesh_topology(f.cuda(), nv, nf)


def check_topology(got, want):
  for name in TOPOLOGY_FIELDS:
    K.same(getattr(got, name), getattr(want, name), name)
  assert got.vf_corners.is_cuda and got.irregular.is_cuda and not got.vertex_offsets.is_cuda and got.vertex_offsets_dev.is_cuda


@pytest.mark.parametrize("device_counts", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_topology_equals_twin(name, device_counts):
  got = gpu_topology(name, device_counts)
  check_topology(got, twin_topology(name))
  K.same(M.is_closed(got), M.is_closed(twin_topology(name)))


def test_topology_is_the_same_every_run():
  a, b = gpu_topology("ball"), gpu_topology("ball")
  for name in TOPOLOGY_FIELDS:
    K.same(getattr(a, name), getattr(b, name), name)


def test_marching_cubes_meshes_are_closed():
  rng = np.random.RandomState(3)
  for g in (t.from_numpy(MC.ellipsoid_fields(3, 20, 5)), t.from_numpy(np.stack([MC.case_field(c, rng) for c in range(1, 256)]))):
    m = VZ.marching_cubes(g.cuda())
    topo = M.mesh_topology(m.faces, m.num_vertices, m.num_faces, total_vertices=m.vertices.shape[0])
    assert bool(M.is_closed(topo).all())
    check_topology(topo, M.mesh_topology(m.faces.cpu(), m.num_vertices.cpu(), m.num_faces.cpu()))


@pytest.mark.parametrize("bad", [4, -1])
def test_bad_face_ids_raise(bad):
  v, f, nv, nf = K.batch([(np.zeros((4, 3)), K.TETRA), (np.zeros((5, 3)), K.TETRA)])
  f = f.clone()
  f[2, 1] = bad
  with pytest.raises(ValueError):
    M.mesh_topology(f.cuda(), nv, nf)
  with pytest.raises(ValueError):
    M.mesh_topology(f.cuda(), nv.cuda(), nf.cuda(), total_vertices=9)
  with pytest.raises(ValueError):
    M.cluster_decimate(v.cuda(), f.cuda(), nv, nf, 1.0)
  with pytest.raises(ValueError):
    M.mesh_topology(f.cuda(), nv.cuda(), nf.cuda(), total_vertices=8)       # counts that do not add up


@pytest.mark.parametrize("mu", [-0.53, None])
@pytest.mark.parametrize("iterations", [0, 1, 3])
@pytest.mark.parametrize("name", ["fans", "small", "ball", "workgroup+1"])
def test_smoothing_equals_twin(name, iterations, mu):
  v = CASES[name][0]
  topo, ref = gpu_topology(name), twin_topology(name)
  got = M.taubin_smooth(v.cuda(), topo, iterations, 0.5, mu)
  assert got.is_cuda
  K.same(got, M.taubin_smooth(v, ref, iterations, 0.5, mu))
  fixed = t.from_numpy(np.random.RandomState(1).rand(len(v)) < 0.3)
  K.same(M.taubin_smooth(v.cuda(), topo, iterations, 0.5, mu, fixed=fixed.cuda()), M.taubin_smooth(v, ref, iterations, 0.5, mu, fixed=fixed))


def test_a_nan_spreads_as_on_the_host():
  v = CASES["ball"][0].clone()
  v[700, 1] = float("nan")
  v[3, 2] = float("inf")
  got = M.taubin_smooth(v.cuda(), gpu_topology("ball"), 2)
  want = M.taubin_smooth(v, twin_topology("ball"), 2)
  K.same(got, want)
  assert 1 < int(t.isnan(want[:, 1]).sum()) < len(v)
  lonely = CASES["small"][0]
  K.same(M.taubin_smooth(lonely.cuda(), gpu_topology("small"), 3), M.taubin_smooth(lonely, twin_topology("small"), 3))


@pytest.mark.parametrize("name", sorted(CASES))
def test_normals_equal_twin(name):
  v, f, nv, nf = CASES[name]
  K.same(M.face_normals(v.cuda(), f.cuda(), nv, nf), M.face_normals(v, f, nv, nf))
  K.same(M.vertex_normals(v.cuda(), f.cuda(), gpu_topology(name)), M.vertex_normals(v, f, twin_topology(name)))


@pytest.mark.parametrize("name", sorted(DECIMATION))
def test_decimation_equals_twin(name):
  (v, f, nv, nf), cell = DECIMATION[name]
  got, want = M.cluster_decimate(v.cuda(), f.cuda(), nv.cuda(), nf.cuda(), cell), M.cluster_decimate(v, f, nv, nf, cell)
  for field in ("vertices", "normals", "faces", "num_vertices", "num_faces"):
    K.same(getattr(got.meshes, field), getattr(want.meshes, field), field)
  K.same(got.vertex_map, want.vertex_map, "vertex_map")
  K.same(got.cluster_size, want.cluster_size, "cluster_size")
  assert got.meshes.vertices.is_cuda and got.vertex_map.is_cuda


def test_decimation_errors():
  lo, hi = TILES.cell_min, TILES.cell_max
  for bad in (lo - 0.5, hi + 1.0, float("nan"), float("inf")):
    v = t.tensor([[0, 0, 0], [1, 0, 0], [0, bad, 0]], dtype=t.float32)
    with pytest.raises(ValueError):
      M.cluster_decimate(v.cuda(), t.tensor([[0, 1, 2]]).cuda(), [3], [1], 1.0)


@pytest.mark.parametrize("cell", [None, 2.0])
def test_refine_meshes_equals_twin(cell):
  mask = (t.from_numpy(MC.ellipsoid_fields(3, 20, 5)) > 0.5).float()
  mask[1] = 0
  got = VZ.refine_meshes(VZ.marching_cubes(mask.cuda()), cell_size=cell, smooth_iterations=5)
  want = VZ.refine_meshes(VZ.marching_cubes(mask), cell_size=cell, smooth_iterations=5)
  for field in ("vertices", "normals", "faces", "num_vertices", "num_faces"):
    K.same(getattr(got, field), getattr(want, field), field)
  vol, area = M.mesh_volume_area(got.vertices, got.faces, got.num_vertices, got.num_faces)
  assert vol.is_cuda and vol.dtype == t.float64 and vol.shape == area.shape == (3,)          # torch sums: no bit pattern is promised
  assert float(vol[1]) == 0 and float(area[1]) == 0 and float(vol[0]) > 0 and float(area[0]) > 0
