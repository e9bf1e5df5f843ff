"""corenet_amd.visualization on the MI355X: the HIP marching cubes against the library's host twin, bit for bit."""
import os

import numpy as np
import pytest
import torch as t

import mesh_check as MC
from oracle import corenet_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def V():
  import corenet_amd.visualization as V
  return V


def _same(a, b):
  for x, y in zip(a, b):
    assert x.device.type == "cuda" and y.device.type == "cpu"
    assert x.dtype == y.dtype and x.shape == y.shape
    assert t.equal(x.cpu(), y), (x.shape, (x.cpu() != y).sum())


def _both(V, grid, **kw):
  g = grid.cuda() if not grid.is_cuda else grid
  gpu = V.marching_cubes(g, **kw)
  cpu = V.marching_cubes(g.cpu(), **kw)
  _same(gpu, cpu)
  return gpu


def test_gpu_equals_host_twin_small_fields(V):
  rng = np.random.RandomState(11)
  cases = t.from_numpy(np.stack([MC.case_field(c, rng) for c in range(256)]))
  _both(V, cases)
  noise = t.from_numpy(rng.rand(3, 33, 47, 29).astype(np.float32))
  _both(V, noise)
  _both(V, noise, level=0.3)
  _both(V, noise, filter_kernel=3)
  pmf = t.from_numpy(rng.rand(2, 4, 19, 20, 21).astype(np.float32)).cuda()
  for view in (pmf[1, 1:], pmf[:, 1], pmf[0, :, ::2, 1:, :]):
    gpu = V.marching_cubes(view)
    _same(gpu, V.marching_cubes(view.cpu()))
  mats = t.eye(4).repeat(3, 1, 1) + 0.05 * t.from_numpy(rng.randn(3, 4, 4).astype(np.float32))
  mats[:, 3] = t.tensor([0.01, -0.02, 0.03, 1.0])
  _same(V.marching_cubes(noise.cuda(), matrices=mats.cuda()), V.marching_cubes(noise, matrices=mats))
  for k in (2, 3, 4):
    assert t.equal(V.box_filter(noise.cuda(), k).cpu(), V.box_filter(noise, k))
  empty = V.marching_cubes(t.zeros(2, 5, 6, 7, device="cuda"))
  assert empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3) and empty.num_faces.tolist() == [0, 0]


def test_gpu_large_objects_topology_and_determinism(V):
  g128 = t.from_numpy(MC.ellipsoid_fields(4, 128, seed=1))
  _both(V, g128)
  g256 = t.from_numpy(MC.ellipsoid_fields(1, 256, seed=2)).cuda()
  a = _both(V, g256)
  b = V.marching_cubes(g256)
  for x, y in zip(a, b):
    assert t.equal(x, y)                                                # two runs: bit-identical
  v, n, f = MC.split(a)[0]
  assert len(f) > 0
  MC.check_closed_oriented(f, len(v))
  assert MC.euler(len(v), f) % 2 == 0 and MC.signed_volume(v, f) > 0
  pos, _ = MC.expected_vertices(g256[0].cpu().numpy())
  assert v.tobytes() == pos.tobytes()


def test_gpu_52_objects_chunked(V):
  """m7 x2 super-resolution at B = 4: 52 objects of 256^3 in one call -- more cells than one apply / emit chunk holds."""
  base = t.from_numpy(MC.ellipsoid_fields(4, 256, seed=3))
  g = t.empty(52, 256, 256, 256, device="cuda")
  for i in range(52):
    g[i] = base[i % 4].cuda().roll(shifts=(i, 2 * i, 3 * i), dims=(0, 1, 2))
  assert 52 * 257 ** 3 > (1 << 26)
  m = _both(V, g)
  assert int(m.num_faces.min()) > 0
  vb = t.cumsum(m.num_vertices, 0) - m.num_vertices
  fb = t.cumsum(m.num_faces, 0) - m.num_faces
  for i in (0, 3, 25, 51):
    one = V.marching_cubes(g[i:i + 1])
    assert t.equal(one.vertices, m.vertices[vb[i]:vb[i] + m.num_vertices[i]])
    assert t.equal(one.normals, m.normals[vb[i]:vb[i] + m.num_vertices[i]])
    assert t.equal(one.faces, m.faces[fb[i]:fb[i] + m.num_faces[i]])


def _model(nc, sd):
  from corenet_amd.model.core_net import CoreNet, CoreNetConfig, DecoderConfig
  m = CoreNet(CoreNetConfig(DecoderConfig((128, 128, 128), nc, 2, 64, 0.75)), device="cuda", decoder_math="bf16x3")
  m.load_state_dict(sd)
  return m.eval()


def test_model_path_h7_eval_and_m7_superres(V):
  from corenet_amd import super_resolution as SR
  # h7 eval pmf -> MarchingCubesArtifact's mesh
  m = _model(2, O.make_state(0, 2, nbt=100))
  image, v2s, off, _ = O.synthetic_batch(1, 0, 2)
  with t.no_grad():
    pmf = m(image.cuda(), v2s.cuda(), off.cuda()).softmax(1)
  v2w = O.scale([1 / 128.0] * 3).cuda()
  tri, nrm, cnt = V.marching_cubes_artifact_mesh(pmf[0], v2w)
  ct, cn, cc = V.marching_cubes_artifact_mesh(pmf[0].cpu(), v2w.cpu())
  assert t.equal(tri.cpu(), ct) and t.equal(nrm.cpu(), cn) and t.equal(cnt.cpu(), cc)
  assert int(cnt[0]) > 1 and (pmf[0, 1] > 0.5).any()
  mesh = V.marching_cubes(pmf[:, 1])                                   # [B, 128^3] strided view
  _same(mesh, V.marching_cubes(pmf[:, 1].cpu()))
  v, n, f = MC.split(mesh)[0]
  MC.check_closed_oriented(f, len(v))
  # m7 x2 super-resolution, B = 4: all 13 foreground classes of the [4, 14, 256^3] pmf in one call
  m14 = _model(14, O.make_state(0, 14, nbt=100))

  class State: pass
  st = State(); st.model = m14
  sr = SR.super_resolution_from_state(st)
  image, _, _, _ = O.synthetic_batch(4, 0, 14)
  camera = O.canonical_camera()[None].repeat(4, 1, 1).cuda()
  v2v = O.scale([128.0] * 3)[None].repeat(4, 1, 1).cuda()
  with t.no_grad():
    pmf = sr(image.cuda(), camera, v2v, t.full((4, 3), 0.5).cuda(), (256, 256, 256))
  assert pmf.shape == (4, 14, 256, 256, 256)
  grid = pmf[:, 1:].reshape(52, 256, 256, 256)
  got = V.marching_cubes(grid)
  assert int(got.num_faces.sum()) > 0
  _same(got, V.marching_cubes(grid.cpu()))
  for v, n, f in MC.split(got):
    if len(f):
      MC.check_closed_oriented(f, len(v))
