"""corenet_amd.visualization through the library's host twin (no GPU): the marching-cubes contract, checked without the
triangle table, and the reference contract of MarchingCubesArtifact (visualization/artifacts.py:202-289)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as t
import torch.nn.functional as F

import mesh_check as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def V():
  from corenet_amd import build as B
  if not os.path.exists(B.LIB):
    B.build(verbose=False)
  import corenet_amd.visualization as V
  return V


def test_generated_table_is_committed():
  r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_mc_tables.py"), "--check"])
  assert r.returncode == 0, "corenet_amd/csrc/mc_tables.h differs from tools/gen_mc_tables.py's output"


def test_all_256_cases_closed_oriented(V):
  rng = np.random.RandomState(0)
  for case in range(1, 256):
    fields = np.stack([MC.case_field(case, rng) for _ in range(4)])
    m = V.marching_cubes(t.from_numpy(fields))
    for v, n, f in MC.split(m):
      MC.check_closed_oriented(f, len(v))
      assert (MC.areas(v, f) > 1e-9).all(), case
      assert MC.signed_volume(v, f) > 0, case
  m = V.marching_cubes(t.from_numpy(np.stack([MC.case_field(0, rng)])))
  assert int(m.num_faces[0]) == 0 and int(m.num_vertices[0]) == 0


def _check_vertex_set(m, grids, level=0.5):
  for (v, n, f), g in zip(MC.split(m), grids):
    pos, nrm, cond = MC.expected_vertices(g, level, with_cond=True)
    assert v.shape == pos.shape
    assert v.tobytes() == pos.tobytes(), "positions are not bit-equal to the float32 formula"
    # float32 normals: within 1e-6 of the float64 formula, scaled by the cancellation in g0 + t (g1 - g0) where the
    # interpolated gradient is much shorter than the endpoint gradients (random noise)
    err = np.abs(n.astype(np.float64) - nrm).max(1) if len(v) else np.zeros(0)
    assert (err < 1e-6 * cond).all(), float((err / cond).max())
    assert (err[cond < 4] < 1e-6).all()


def test_vertex_set_pinned(V):
  rng = np.random.RandomState(1)
  cases = np.stack([MC.case_field(c, rng) for c in range(256)])
  _check_vertex_set(V.marching_cubes(t.from_numpy(cases)), cases)
  noise = rng.rand(2, 33, 47, 29).astype(np.float32)
  _check_vertex_set(V.marching_cubes(t.from_numpy(noise)), noise)
  _check_vertex_set(V.marching_cubes(t.from_numpy(noise), level=0.3), noise, 0.3)
  # strided views: pmf[b, 1:], pmf[:, 1] and a view with stepped D / offset H need no copy
  pmf = t.from_numpy(rng.rand(2, 4, 9, 10, 11).astype(np.float32))
  for view in (pmf[1, 1:], pmf[:, 1], pmf[0, :, ::2, 1:, :]):
    assert view.stride(-1) == 1 and view.data_ptr() != pmf.data_ptr() or not view.is_contiguous()
    _check_vertex_set(V.marching_cubes(view), view.numpy())
  for v, n, f in MC.split(V.marching_cubes(t.from_numpy(noise))):
    MC.check_closed_oriented(f, len(v))


def test_nan_and_level_ties_are_outside(V):
  g = np.zeros((1, 3, 3, 3), np.float32)
  g[0, 1, 1, 1] = 1
  g[0, 0, 0, 0] = np.nan
  g[0, 2, 2, 2] = 0.5
  m = V.marching_cubes(t.from_numpy(g))
  assert int(m.num_vertices[0]) == 6 and int(m.num_faces[0]) == 8
  assert np.isfinite(m.vertices.numpy()).all() and np.isfinite(m.normals.numpy()).all()


def test_single_voxel(V):
  g = np.zeros((1, 3, 4, 5), np.float32)
  g[0, 1, 2, 3] = 1
  m = V.marching_cubes(t.from_numpy(g))
  v, n, f = MC.split(m)[0]
  assert len(v) == 6 and len(f) == 8
  c = np.array([3 + 1, 2 + 1, 1 + 1], np.float32)                 # (w + 1, h + 1, d + 1)
  d = v - c
  assert sorted(map(tuple, np.round(d, 6).tolist())) == sorted(
      [(s * (i == 0), s * (i == 1), s * (i == 2)) for i in range(3) for s in (-0.5, 0.5)])
  assert abs(MC.signed_volume(v, f) - 1 / 6) < 1e-6
  assert np.allclose(n, d / 0.5, atol=1e-6)                        # outward


def _sdf(shape, fn):
  z, y, x = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")
  return np.clip(0.5 + 0.1 * fn(x, y, z), 0, 1).astype(np.float32)


def test_sphere_known_answers(V):
  r, c = 20.0, 31.3
  g = _sdf((64, 64, 64), lambda x, y, z: r - np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2))
  v, n, f = MC.split(V.marching_cubes(t.from_numpy(g[None])))[0]
  MC.check_closed_oriented(f, len(v))
  assert MC.euler(len(v), f) == 2
  assert abs(MC.signed_volume(v, f) / (4 / 3 * np.pi * r ** 3) - 1) < 0.01
  assert abs(MC.areas(v, f).sum() / (4 * np.pi * r ** 2) - 1) < 0.02
  radial = v.astype(np.float64) - (c + 1)
  radial /= np.linalg.norm(radial, axis=1, keepdims=True)
  assert np.abs(n - radial).max() < 1e-2


def test_torus_and_two_spheres(V):
  R, r, c = 16.0, 6.0, 31.5
  torus = _sdf((64, 64, 64), lambda x, y, z: r - np.sqrt((np.sqrt((x - c) ** 2 + (y - c) ** 2) - R) ** 2 + (z - c) ** 2))
  two = _sdf((48, 48, 64), lambda x, y, z: np.maximum(
      10 - np.sqrt((x - 16) ** 2 + (y - 24) ** 2 + (z - 24) ** 2), 10 - np.sqrt((x - 46) ** 2 + (y - 24) ** 2 + (z - 24) ** 2)))
  (vt, _, ft), = MC.split(V.marching_cubes(t.from_numpy(torus[None])))
  (vs, _, fs), = MC.split(V.marching_cubes(t.from_numpy(two[None])))
  for v, f in ((vt, ft), (vs, fs)):
    MC.check_closed_oriented(f, len(v))
  assert MC.euler(len(vt), ft) == 0
  assert MC.euler(len(vs), fs) == 4


def test_to_marching_cubes_reference_contract(V):
  g = np.zeros((4, 5, 6, 7), np.float32)
  g[1, 2, 3, 4] = 1                                        # object 0 and 2 empty, 3 has values <= 0.5 only
  g[3] = 0.5
  tri, nrm, cnt = V.to_marching_cubes(t.from_numpy(g))
  assert tri.dtype == t.float32 and nrm.dtype == t.float32 and cnt.dtype == t.int32
  assert tri.shape == (int(cnt.sum()), 3, 3) and nrm.shape == tri.shape
  assert cnt.tolist() == [1, 8, 1, 1]
  assert (tri[0] == 1).all() and (nrm[0] == 1).all() and (tri[9] == 1).all() and (tri[10] == 1).all()
  centre = tri[1:9].reshape(-1, 3).mean(0)
  assert t.allclose(centre, t.tensor([4 + 1.0, 3 + 1.0, 2 + 1.0]))            # (x, y, z) = (w, h, d) + 1
  # the same soup as the indexed form
  m = V.marching_cubes(t.from_numpy(g[1:2]))
  assert t.equal(tri[1:9], m.vertices[m.faces.long()]) and t.equal(nrm[1:9], m.normals[m.faces.long()])


@pytest.mark.parametrize("k", [2, 3, 4])
def test_box_filter_matches_conv3d(V, k):
  g = t.rand(3, 9, 10, 11, generator=t.Generator().manual_seed(k))
  pad = t.constant_pad_nd(g, [(k - 1) // 2, k - 1 - (k - 1) // 2] * 3)
  want = F.conv3d(pad[:, None], g.new_ones([1, 1, k, k, k]) / k ** 3)[:, 0]
  got = V.box_filter(g, k)
  assert got.shape == g.shape and float((got - want).abs().max()) < 1e-6
  view = t.rand(2, 5, 9, 10, 11)[1, 1:]
  assert t.equal(V.box_filter(view, k), V.box_filter(view.contiguous(), k))
  m1 = V.marching_cubes(g, filter_kernel=k)
  m2 = V.marching_cubes(V.box_filter(g, k))
  for a, b in zip(m1, m2):
    assert t.equal(a, b)


def test_matrix_path_matches_einsum(V):
  rng = np.random.RandomState(5)
  g = t.from_numpy(rng.rand(3, 12, 13, 14).astype(np.float32))
  mats = t.eye(4).repeat(3, 1, 1) + 0.05 * t.from_numpy(rng.randn(3, 4, 4).astype(np.float32))
  mats[:, 3] = t.tensor([0.01, -0.02, 0.03, 1.0])
  plain = V.marching_cubes(g)
  tm = V.marching_cubes(g, matrices=mats)
  assert t.equal(tm.faces, plain.faces) and t.equal(tm.num_vertices, plain.num_vertices)
  obj = t.repeat_interleave(t.arange(3), plain.num_vertices)
  hv = t.einsum("bnm,bm->bn", mats[obj], t.constant_pad_nd(plain.vertices, [0, 1], value=1))
  want_v = hv[:, :3] / hv[:, 3:4]
  want_n = t.einsum("bnm,bm->bn", mats[obj], t.constant_pad_nd(plain.normals, [0, 1], value=0))[:, :3]
  assert float((tm.vertices - want_v).abs().max()) < 1e-6 * float(want_v.abs().max())
  assert float((tm.normals - want_n).abs().max()) < 1e-6


def test_artifact_mesh(V):
  rng = np.random.RandomState(6)
  g = t.from_numpy(rng.rand(3, 10, 11, 12).astype(np.float32))
  g[2] = 0                                                                       # an empty class
  v2w = t.tensor([[0.5, 0, 0, 1], [0, 0.25, 0, -1], [0, 0, 2, 0.5], [0, 0, 0, 1.0]])
  tri, nrm, cnt = V.marching_cubes_artifact_mesh(g, v2w, filter_kernel=2)
  rt, rn, rc = V.to_marching_cubes(V.box_filter(g, 2)[1:])
  assert t.equal(cnt, rc)
  h = t.einsum("nm,tvm->tvn", v2w, t.constant_pad_nd(rt, [0, 1], value=1))
  assert float((tri - h[..., :3] / h[..., 3:]).abs().max()) < 1e-5
  assert float((nrm - t.einsum("nm,tvm->tvn", v2w, t.constant_pad_nd(rn, [0, 1], value=0))[..., :3]).abs().max()) < 1e-5


def _read_ply(path):
  with open(path, "rb") as fh:
    head = []
    while True:
      line = fh.readline().decode("ascii").strip()
      head.append(line)
      if line == "end_header":
        break
    nv = int(next(l for l in head if l.startswith("element vertex")).split()[-1])
    nf = int(next(l for l in head if l.startswith("element face")).split()[-1])
    props = [l.split()[-1] for l in head if l.startswith("property float")]
    assert "format binary_little_endian 1.0" in head
    v = np.frombuffer(fh.read(4 * len(props) * nv), "<f4").reshape(nv, len(props))
    fr = np.frombuffer(fh.read(13 * nf), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    assert (fr["n"] == 3).all() and fh.read() == b""
  return v, fr["i"]


def test_write_ply_roundtrip(V, tmp_path):
  g = t.from_numpy(np.random.RandomState(7).rand(1, 8, 9, 10).astype(np.float32))
  m = V.marching_cubes(g)
  p = str(tmp_path / "m.ply")
  V.write_ply(p, m.vertices, m.faces, m.normals)
  v, f = _read_ply(p)
  assert np.array_equal(v[:, :3], m.vertices.numpy()) and np.array_equal(v[:, 3:], m.normals.numpy())
  assert np.array_equal(f, m.faces.numpy())
  V.write_ply(p, m.vertices, m.faces)
  v, f = _read_ply(p)
  assert v.shape == (len(m.vertices), 3) and np.array_equal(f, m.faces.numpy())


def test_errors_and_casts(V):
  with pytest.raises(ValueError):
    V.marching_cubes(t.zeros(4, 4, 4))
  with pytest.raises(ValueError):
    V.marching_cubes(t.zeros(1, 4, 0, 4))
  for lv in (0.0, -0.5, float("nan")):
    with pytest.raises(ValueError):
      V.marching_cubes(t.zeros(1, 4, 4, 4), level=lv)
  with pytest.raises(ValueError):
    V.to_marching_cubes(t.zeros(2, 3, 4, 5, 6))
  with pytest.raises(ValueError):
    V.box_filter(t.zeros(3, 4, 5), 2)
  with pytest.raises(ValueError):
    V.marching_cubes(t.zeros(2, 4, 4, 4), matrices=t.eye(4).repeat(3, 1, 1))
  g = (np.random.RandomState(8).rand(2, 6, 7, 8) > 0.5)
  a = V.marching_cubes(t.from_numpy(g.astype(np.uint8)))
  b = V.marching_cubes(t.from_numpy(g.astype(np.float32)))
  for x, y in zip(a, b):
    assert t.equal(x, y)
  a = V.marching_cubes(t.from_numpy(g.astype(np.float64)).transpose(2, 3))      # W stride != 1: copied first
  b = V.marching_cubes(t.from_numpy(g.astype(np.float32)).transpose(2, 3).contiguous())
  for x, y in zip(a, b):
    assert t.equal(x, y)
