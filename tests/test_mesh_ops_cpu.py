"""corenet_amd.mesh_ops on the host: the twin against the numpy restatement of tests/mesh_ops_check.py, bit for bit, and
the properties the operations are there for.  No tolerance anywhere: integers by value, floats on their bit patterns."""
import numpy as np
import pytest
import torch as t

import mesh_check as MC
import mesh_ops_check as K
from corenet_amd import mesh_ops as M
from corenet_amd import visualization as VZ

TILES = M.mesh_ops_tiles()
CASES = K.cases(TILES)
DECIMATION = K.decimation_cases(TILES)


def test_tiles():
  assert TILES.threads % 64 == 0 and TILES.sort_lane >= 2 and TILES.sort_tile > TILES.sort_lane
  assert TILES.cell_min <= -2 ** 15 and TILES.cell_max >= 2 ** 15 - 1 and TILES.max_objects >= 2 ** 16 - 2


@pytest.mark.parametrize("name", sorted(CASES))
def test_topology_equals_numpy(name):
  v, f, nv, nf = CASES[name]
  topo = M.mesh_topology(f, nv, nf)
  K.check_topology(topo, K.np_topology(f.numpy(), nv.numpy(), nf.numpy()))
  K.same(topo.vertex_offsets, t.from_numpy(K.np_offsets(nv.numpy())))
  K.same(topo.face_offsets, t.from_numpy(K.np_offsets(nf.numpy())))
  assert topo.vf_corners.numel() == 3 * f.shape[0] and topo.irregular.dtype == t.bool


def test_fan_hubs_have_the_valences_of_the_seams():
  v, f, nv, nf = CASES["fans"]
  topo = M.mesh_topology(f, nv, nf)
  hubs = topo.vertex_offsets[:-1]
  assert (topo.vv_offsets[hubs + 1] - topo.vv_offsets[hubs]).tolist() == K.fan_valences(TILES)
  assert (topo.vf_offsets[hubs + 1] - topo.vf_offsets[hubs]).tolist() == K.fan_valences(TILES)
  assert K.fan_valences(TILES)[-1] > 2 * TILES.sort_tile


def test_is_closed_small_objects():
  v, f, nv, nf = CASES["small"]
  want = [c for _, _, _, c in K.small_objects(np.random.RandomState(0))]
  assert M.is_closed(M.mesh_topology(f, nv, nf)).tolist() == want
  assert M.is_closed(M.mesh_topology(*CASES["empty"][1:])).shape == (0,)


def test_degenerate_and_repeated_faces_are_listed_per_corner():
  topo = M.mesh_topology(t.tensor([[0, 0, 1], [0, 1, 2], [0, 1, 2]], dtype=t.int32), [3], [3])
  assert topo.vf_corners[topo.vf_offsets[0]:topo.vf_offsets[1]].tolist() == [0, 1, 3, 6]
  assert topo.vv_neighbours[topo.vv_offsets[0]:topo.vv_offsets[1]].tolist() == [1, 2]
  assert topo.irregular.tolist() == [True, True, True]


@pytest.mark.parametrize("bad", [4, -1])
def test_bad_face_ids_raise(bad):
  v, f, nv, nf = K.batch([(np.zeros((4, 3)), K.TETRA), (np.zeros((5, 3)), K.TETRA)])
  f = f.clone()
  f[2, 1] = bad                                                             # object 0 has 4 vertices: 4 is object 1's first
  with pytest.raises(ValueError):
    M.mesh_topology(f, nv, nf)
  with pytest.raises(ValueError):
    M.cluster_decimate(v, f, nv, nf, 1.0)
  with pytest.raises(ValueError):
    M.mesh_topology(f, nv, [4, 3])                                          # counts that do not add up


def test_marching_cubes_meshes_are_closed():
  rng = np.random.RandomState(3)
  grids = [t.from_numpy(MC.ellipsoid_fields(3, 20, 5)), t.from_numpy(np.stack([MC.case_field(c, rng) for c in range(1, 256)]))]
  for g in grids:
    m = VZ.marching_cubes(g)
    topo = M.mesh_topology(m.faces, m.num_vertices, m.num_faces)
    assert bool(M.is_closed(topo).all()) and not bool(topo.irregular.any())
    for (v, _, f) in MC.split(m):
      if len(f):
        MC.check_closed_oriented(f, len(v))                                # the independent witness
    K.check_topology(topo, K.np_topology(m.faces.numpy(), m.num_vertices.numpy(), m.num_faces.numpy()))


@pytest.mark.parametrize("mu", [-0.53, None])
@pytest.mark.parametrize("iterations", [0, 1, 3])
@pytest.mark.parametrize("name", ["fans", "small", "ball"])
def test_smoothing_equals_numpy(name, iterations, mu):
  v, f, nv, nf = CASES[name]
  topo = M.mesh_topology(f, nv, nf)
  ref = K.np_topology(f.numpy(), nv.numpy(), nf.numpy())
  got = M.taubin_smooth(v, topo, iterations, 0.5, mu)
  K.same(got, t.from_numpy(K.np_taubin(v.numpy(), ref, iterations, 0.5, mu)))
  assert got.data_ptr() != v.data_ptr()
  fixed = t.from_numpy(np.random.RandomState(1).rand(len(v)) < 0.3)
  K.same(M.taubin_smooth(v, topo, iterations, 0.5, mu, fixed=fixed), t.from_numpy(K.np_taubin(v.numpy(), ref, iterations, 0.5, mu, fixed.numpy())))


def test_isolated_vertices_and_fixed_ones_stay():
  v, f, nv, nf = CASES["small"]
  topo = M.mesh_topology(f, nv, nf)
  lonely = (topo.vv_offsets[1:] == topo.vv_offsets[:-1])
  assert int(lonely.sum()) >= 5
  out = M.taubin_smooth(v, topo, 3)
  K.same(out[lonely], v[lonely])
  assert not t.equal(out[~lonely], v[~lonely])
  everything = t.ones(len(v), dtype=t.bool)
  K.same(M.taubin_smooth(v, topo, 3, fixed=everything), v)


@pytest.mark.parametrize("iterations", [1, 2])
def test_a_nan_reaches_its_neighbourhood_and_nothing_more(iterations):
  v, f, nv, nf = CASES["ball"]
  topo = M.mesh_topology(f, nv, nf)
  v = v.clone()
  start = 700
  v[start, 1] = float("nan")
  reached = np.zeros(len(v), bool)
  reached[start] = True
  off, nb = topo.vv_offsets.numpy(), topo.vv_neighbours.numpy()
  for _ in range(2 * iterations):                                           # two steps per iteration
    grow = reached.copy()
    for i in np.nonzero(reached)[0]:
      grow[nb[off[i]:off[i + 1]]] = True
    reached = grow
  out = M.taubin_smooth(v, topo, iterations)
  assert np.array_equal(t.isnan(out[:, 1]).numpy(), reached) and 1 < reached.sum() < len(v)
  assert not bool(t.isnan(out[:, 0]).any())
  K.same(out, t.from_numpy(K.np_taubin(v.numpy(), K.np_topology(f.numpy(), nv.numpy(), nf.numpy()), iterations)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_normals_equal_numpy(name):
  v, f, nv, nf = CASES[name]
  topo = M.mesh_topology(f, nv, nf)
  ref = K.np_topology(f.numpy(), nv.numpy(), nf.numpy())
  K.same(M.face_normals(v, f, nv, nf), t.from_numpy(K.np_face_normals(v.numpy(), f.numpy(), nv.numpy(), nf.numpy())).reshape(-1, 3))
  K.same(M.vertex_normals(v, f, topo), t.from_numpy(K.np_vertex_normals(v.numpy(), f.numpy(), nv.numpy(), nf.numpy(), ref)).reshape(-1, 3))


def test_normals_that_cancel_and_unit_length():
  names = [n for n, _, _, _ in K.small_objects(np.random.RandomState(0))]
  v, f, nv, nf = CASES["small"]
  topo = M.mesh_topology(f, nv, nf)
  n = M.vertex_normals(v, f, topo)
  o = int(topo.vertex_offsets[names.index("two_sided_triangle")])
  K.same(n[o:o + 3], t.zeros(3, 3))
  length = n.norm(dim=1)
  assert bool(((length == 0) | ((length - 1).abs() < 1e-6)).all())
  with pytest.raises(ValueError):
    M.face_normals(v, f, nv)                                                # several objects need num_faces


@pytest.mark.parametrize("name", sorted(DECIMATION))
def test_decimation_equals_numpy(name):
  (v, f, nv, nf), cell = DECIMATION[name]
  dec = M.cluster_decimate(v, f, nv, nf, cell)
  ref = K.np_cluster(v.numpy(), f.numpy(), nv.numpy(), nf.numpy(), cell)
  K.check_decimated(dec, ref)
  m = dec.meshes
  topo = M.mesh_topology(m.faces, m.num_vertices, m.num_faces)
  K.same(m.normals, M.vertex_normals(m.vertices, m.faces, topo))
  assert int(m.num_vertices.sum()) == m.vertices.shape[0] == dec.cluster_size.numel() and int(m.num_faces.sum()) == m.faces.shape[0]


def test_decimation_counts_of_the_cases():
  dec = M.cluster_decimate(*DECIMATION["one_cluster"][0], 64.0)
  assert dec.meshes.num_vertices.tolist() == [1] and dec.meshes.num_faces.tolist() == [0]
  (v, f, nv, nf), cell = DECIMATION["identical_objects"]
  dec = M.cluster_decimate(v, f, nv, nf, cell)
  a, b, c = dec.meshes.num_vertices.tolist()
  assert a == c > 100 and b == 0
  K.same(dec.meshes.vertices[:a], dec.meshes.vertices[a:])                 # the same coordinates, kept apart
  assert int(dec.vertex_map[:nv[0]].max()) < a <= int(dec.vertex_map[nv[0]:].min())
  assert len(np.unique(DECIMATION["few_hundred_cells"][0][0].numpy() // 1, axis=0)) < 400
  dec = M.cluster_decimate(*DECIMATION["cell_bounds"][0], 1.0)
  assert dec.meshes.num_vertices.tolist() == [4]


def test_decimation_errors():
  lo, hi = TILES.cell_min, TILES.cell_max
  tri = [[0, 1, 2]]
  for bad in (lo - 0.5, hi + 1.0, float("nan"), float("inf")):
    v = t.tensor([[0, 0, 0], [1, 0, 0], [0, bad, 0]], dtype=t.float32)
    with pytest.raises(ValueError):
      M.cluster_decimate(v, tri, [3], [1], 1.0)
  v = t.zeros(3, 3)
  for cell in (0.0, -1.0, float("nan"), float("inf")):
    with pytest.raises(ValueError):
      M.cluster_decimate(v, tri, [3], [1], cell)


def _directed(faces, nv):
  f = np.asarray(faces, np.int64)
  d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
  return d[:, 0] * nv + d[:, 1], d[:, 1] * nv + d[:, 0]


@pytest.mark.parametrize("cell", [0.7, 2.0, 3.0])
def test_decimation_properties_on_the_ball(cell):
  m = K.ball_mesh()[0]
  V = m.vertices.shape[0]
  dec = M.cluster_decimate(m.vertices, m.faces, m.num_vertices, m.num_faces, cell)
  d = dec.meshes
  nv = d.vertices.shape[0]
  assert 1 < nv < V
  fwd, rev = _directed(d.faces.numpy(), nv)                                 # every directed edge as often as its reverse
  ka, ca = np.unique(fwd, return_counts=True)
  kb, cb = np.unique(rev, return_counts=True)
  assert np.array_equal(ka, kb) and np.array_equal(ca, cb)
  c32 = np.float32(cell)
  cells = np.floor(m.vertices.numpy() / c32).astype(np.float64)            # every new vertex in its closed cell, to one ulp
  got = d.vertices.numpy().astype(np.float64)
  lo, hi = cells * float(c32), (cells + 1) * float(c32)
  ulp = np.spacing(np.abs(d.vertices.numpy())).astype(np.float64)
  mapped = got[dec.vertex_map.numpy().astype(np.int64)]
  assert (mapped >= lo - ulp[dec.vertex_map.numpy()]).all() and (mapped <= hi + ulp[dec.vertex_map.numpy()]).all()
  assert int(dec.cluster_size.sum()) == V and int(dec.cluster_size.min()) >= 1
  assert np.array_equal(np.unique(dec.vertex_map.numpy()), np.arange(nv))  # onto
  assert np.array_equal(np.bincount(dec.vertex_map.numpy()), dec.cluster_size.numpy())


def _radial_agreement(v, f, centre):
  v = v.astype(np.float64)
  a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
  n = np.cross(b - a, c - a)
  r = (a + b + c) / 3 - centre
  return float(np.mean(np.einsum("ij,ij->i", n, r) / (np.linalg.norm(n, axis=1) * np.linalg.norm(r, axis=1))))


def test_taubin_keeps_the_volume_and_smooths_the_staircase():
  m, centre = K.ball_mesh()
  f = m.faces.numpy().astype(np.int64)
  topo = M.mesh_topology(m.faces, m.num_vertices, m.num_faces)
  taubin = M.taubin_smooth(m.vertices, topo, 10).numpy()
  laplace = M.taubin_smooth(m.vertices, topo, 10, mu=None).numpy()
  v0 = MC.signed_volume(m.vertices.numpy(), f)
  assert abs(MC.signed_volume(taubin, f) - v0) < abs(MC.signed_volume(laplace, f) - v0)
  assert _radial_agreement(taubin, f, centre) > _radial_agreement(m.vertices.numpy(), f, centre)
  vol, area = M.mesh_volume_area(m.vertices, m.faces, m.num_vertices, m.num_faces)
  assert abs(float(vol[0]) - v0) <= 1e-9 * abs(v0) and abs(float(area[0]) - MC.areas(m.vertices.numpy(), f).sum()) <= 1e-9 * float(area[0])


@pytest.mark.parametrize("cell", [None, 2.0])
def test_refine_meshes_feeds_the_writers(tmp_path, cell):
  from corenet_amd.visualization.marching_cubes import _triangle_soup
  mask = (t.from_numpy(MC.ellipsoid_fields(2, 16, 9)) > 0.5).float()
  mask[1] = 0                                                               # an object without a surface
  m = VZ.marching_cubes(mask)
  r = VZ.refine_meshes(m, cell_size=cell, smooth_iterations=4)
  assert r.vertices.shape == r.normals.shape and r.vertices.shape[0] == int(r.num_vertices.sum())
  assert r.faces.shape[0] == int(r.num_faces.sum()) and r.faces.dtype == t.int32 and r.num_faces.tolist()[1] == 0
  if cell is None:
    assert t.equal(r.faces, m.faces) and not t.equal(r.vertices, m.vertices)
  assert int(r.faces.max()) < int(r.num_vertices[0])
  topo = M.mesh_topology(r.faces, r.num_vertices, r.num_faces)
  K.same(r.normals, M.vertex_normals(r.vertices, r.faces, topo))
  VZ.write_ply(str(tmp_path / "m.ply"), r.vertices, r.faces, r.normals)
  tri, nrm, cnt = _triangle_soup(r, t.ones(3, 3), t.ones(3, 3))
  assert tri.shape == nrm.shape and cnt.tolist() == [int(r.num_faces[0]), 1]
