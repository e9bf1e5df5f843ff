"""Label overlaps on the GPU (csrc/voxel_overlap.hip) against the library's host twin: every field of
label_overlaps is equal exactly.  The twin itself is anchored to np.unique in test_voxel_overlap_cpu.py.  Shapes come
from overlap_tiles() and are the smallest that reach each seam: the chunk of a workgroup, the 16-byte loads with their
scalar head and tail, the LDS table and the table in global memory, the 64 grids of a launch, the groups of a call."""
import types

import numpy as np
import pytest
import torch as t

import voxel_overlap_check as VC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
  from corenet_amd import voxel_overlap as M
  return M


def _equal(M, a, b, num_a=None, num_b=None, msg="", **kw):
  """GPU == twin on the CPU tensors a, b [N, D, H, W] (any strides: the device copies keep them)."""
  a, b = t.as_tensor(a), t.as_tensor(b)
  want = M.label_overlaps(a, b, num_a, num_b)
  da = t.empty_strided(a.shape, a.stride(), dtype=a.dtype, device="cuda").copy_(a) if a.numel() else a.cuda()
  db = t.empty_strided(b.shape, b.stride(), dtype=b.dtype, device="cuda").copy_(b) if b.numel() else b.cuda()
  return _equal_on(M, da, db, want, num_a, num_b, msg, **kw)


def _equal_on(M, da, db, want, num_a=None, num_b=None, msg="", **kw):
  got = M.label_overlaps(da, db, num_a, num_b, **kw)
  assert not got.offsets.is_cuda and got.a.is_cuda and got.a.dtype == t.int32 and got.count.dtype == t.int64
  for name, x, y in zip(got._fields, got, want):
    assert t.equal(x.cpu(), y), (msg, name)
  return want


def _view(base, sl):
  """The view base[sl] on the device with the strides it has on the host (base is copied whole)."""
  return base.cuda()[sl]


def test_chunk_seams(M):
  chunk = M.overlap_tiles()[0]
  rng = np.random.default_rng(0)
  for voxels in (chunk - 1, chunk, chunk + 1):
    a, b = VC.random_labels(rng, (2, 1, 1, voxels), 5), VC.random_labels(rng, (2, 1, 1, voxels), 3, np.uint8)
    a[:, 0, 0, -2:] = [[5, 4], [1, 2]]                                       # the last voxels of the last chunk count
    want = _equal(M, a, b, msg=voxels)
    assert int(want.count.sum()) == 2 * voxels


@pytest.mark.parametrize("W", [1, 3, 4, 5, 17])
def test_row_heads_and_tails(M, W):
  rng = np.random.default_rng(W)
  base_a, base_b = t.from_numpy(VC.random_labels(rng, (2, 5, 7, W + 4), 6)), t.from_numpy(VC.random_labels(rng, (2, 5, 7, W + 4), 2))
  _equal(M, base_a[..., :W].contiguous(), base_b[..., :W].contiguous(), msg="one row")
  for start in (0, 1, 3):                                                    # rows of W voxels at every alignment
    sl = (Ellipsis, slice(start, start + W))
    want = M.label_overlaps(base_a[sl], base_b[sl])
    _equal_on(M, _view(base_a, sl), _view(base_b, sl), want, msg=start)
    _equal_on(M, _view(base_a, sl), _view(base_b.to(t.uint8), sl), want, msg=(start, "u8"))
  sl_b = (Ellipsis, slice(2, 2 + W))                                         # alignments that never agree
  _equal_on(M, _view(base_a, (Ellipsis, slice(1, 1 + W))), _view(base_b, sl_b), M.label_overlaps(base_a[..., 1:1 + W], base_b[sl_b]))


def test_views(M):
  rng = np.random.default_rng(1)
  a, b = t.from_numpy(VC.random_labels(rng, (2, 6, 9, 261), 40)), t.from_numpy(VC.random_labels(rng, (2, 6, 9, 261), 7, np.uint8))
  for sl in ((Ellipsis, slice(1, None)), (slice(None), slice(None, None, 2)), (slice(None), slice(None), slice(1, None, 3)),
             (slice(1, None),)):
    _equal_on(M, _view(a, sl), _view(b, sl), M.label_overlaps(a[sl], b[sl]), msg=sl)
  _equal_on(M, a.cuda()[..., ::2], b.cuda()[..., ::2], M.label_overlaps(a[..., ::2], b[..., ::2]), msg="W stride 2")
  _equal_on(M, a.cuda()[:1].expand(2, -1, -1, -1), b.cuda(), M.label_overlaps(a[:1].expand(2, -1, -1, -1), b), msg="N stride 0")


def test_dtype_mixes(M):
  rng = np.random.default_rng(2)
  shape = (2, 4, 33, 130)
  u, i = VC.random_labels(rng, shape, 9, np.uint8), VC.random_labels(rng, shape, 70, np.int32)
  for a, b in ((u, i), (i, u), (u, u[::-1].copy()), (i, i[::-1].copy()), (i.astype(np.int64), u > 4)):
    _equal(M, a, b)


def _every_entry(rng, na, nb, voxels):
  """Grids of `voxels` voxels in which every pair (i, j), i <= na, j <= nb, occurs, in random order."""
  entries = (na + 1) * (nb + 1)
  key = np.concatenate([np.arange(entries), rng.integers(0, entries, voxels - entries)])
  key = rng.permutation(key)
  return (key // (nb + 1)).astype(np.int32), (key % (nb + 1)).astype(np.int32)


def test_lds_and_global_tables(M):
  lds = M.overlap_tiles()[1]
  rng = np.random.default_rng(3)
  side = 1
  while side * side < lds:
    side *= 2
  assert side * side == lds and (lds + 1) % 5 == 0
  cases = [(side - 1, side - 1), (4, (lds + 1) // 5 - 1), (lds - 1, 0), (0, lds)]   # lds, lds + 1, lds, lds + 1 entries
  a, b = zip(*(_every_entry(rng, na, nb, 2 * 32 ** 3) for na, nb in cases))
  a, b = np.stack(a).reshape(4, 64, 32, 32), np.stack(b).reshape(4, 64, 32, 32)
  want = _equal(M, a, b)
  assert (want.offsets[1:] - want.offsets[:-1]).tolist() == [lds, lds + 1, lds, lds + 1]
  _equal(M, a[:, ::-1].copy(), b, num_a=[side + 2, 4, lds - 1, 1], num_b=[side - 1, lds, 0, lds])   # both paths, other widths


def test_register_counts(M):
  """All background and all one pair: nothing but the counts a lane keeps in registers, and one run per lane."""
  chunk = M.overlap_tiles()[0]
  z = np.zeros((3, 2, 3, chunk // 4 + 5), np.int32)
  want = _equal(M, z, z.astype(np.uint8))
  assert want.count.tolist() == [z[0].size] * 3 and want.a.tolist() == [0] * 3
  a = z.copy()
  a[1] = 3
  a[2] = 1
  want = _equal(M, a, np.where(a > 0, 2, 0).astype(np.int32), num_a=[0, 3, 9], num_b=[0, 2, 2])
  assert want.count.tolist() == [z[0].size] * 3 and want.a.tolist() == [0, 3, 1] and want.b.tolist() == [0, 2, 2]


def test_bad_labels(M):
  rng = np.random.default_rng(4)
  a, b = VC.random_labels(rng, (3, 5, 11, 67), 12), VC.random_labels(rng, (3, 5, 11, 67), 6)
  a[0, 0, 0, :5] = -1
  b[1, 2, 3, 66] = -(2 ** 31)
  b[2] = 7                                                                   # a whole grid out of range
  want = _equal(M, a, b, num_a=[9, 12, 12], num_b=[6, 3, 6])
  assert want.bad[2] == a[2].size and (want.bad > 0).all() and int(want.count.sum() + want.bad.sum()) == a.size
  _equal(M, a.astype(np.uint8), b.astype(np.uint8), num_a=[255, 0, 3], num_b=[6, 255, 300])


def test_empty_batch(M):
  got = M.label_overlaps(t.zeros((0, 4, 5, 6), dtype=t.int32, device="cuda"), t.zeros((0, 4, 5, 6), dtype=t.uint8, device="cuda"))
  assert got.offsets.tolist() == [0] and all(x.numel() == 0 and x.is_cuda for x in got[1:])


def test_more_grids_than_a_launch(M):
  rng = np.random.default_rng(5)
  a, b = VC.random_labels(rng, (131, 3, 5, 9), 4), VC.random_labels(rng, (131, 3, 5, 9), 3, np.uint8)
  a[64] = 4                                                                  # the first grid of the second launch
  a[130, 2, 4, 8] = 3
  _equal(M, a, b)


def test_groups_and_sorted_fallback(M):
  rng = np.random.default_rng(6)
  a, b = VC.random_labels(rng, (5, 4, 9, 31), 20), VC.random_labels(rng, (5, 4, 9, 31), 9)
  a[2] %= 3                                                                  # grid 2: a table of 3 x 10
  a[3, 0, 0, 0] = -1
  num_a, num_b = [20, 20, 2, 20, 20], [9] * 5
  for cap in (1, 29, 30, 210, 211, 450):                                     # all sorted / mixed / one grid per group / two
    _equal(M, a, b, num_a, num_b, msg=cap, _max_table_entries=cap)


def test_non_default_stream(M):
  rng = np.random.default_rng(7)
  a, b = t.from_numpy(VC.random_labels(rng, (2, 16, 32, 160), 30)), t.from_numpy(VC.random_labels(rng, (2, 16, 32, 160), 5))
  want = M.label_overlaps(a, b)
  s = t.cuda.Stream()
  with t.cuda.stream(s):
    da, db = a.cuda(), b.cuda()
    got = M.label_overlaps(da, db)
  s.synchronize()
  for x, y in zip(got, want):
    assert t.equal(x.cpu(), y)


def _instance_case(seed, dev):
  sem, labels, inst = VC.instance_arrays(seed)
  pmf = t.from_numpy(np.stack([(sem == c) for c in range(4)], 1).astype(np.float32))
  ex = types.SimpleNamespace(scene_id=[f"scene{seed}_{b}" for b in range(len(labels))], mesh_labels=[t.from_numpy(v) for v in labels],
                             grid=t.from_numpy(sem).to(dev))
  return pmf.to(dev), ex, t.from_numpy(inst).to(dev)


def _rows_equal(got, want):
  assert got.scene_id == want.scene_id
  for name in ("tp", "fp", "fn"):
    assert t.equal(getattr(got.counts, name).cpu(), getattr(want.counts, name)), name
  # sums of a few IoUs <= 1 in float64: the order of the adds may differ, each add rounds by at most 2^-53 of the sum
  assert t.allclose(got.counts.sum_iou.cpu(), want.counts.sum_iou, rtol=0, atol=1e-13)
  for name in ("scene_index", "mesh_index", "class_index", "gt_voxels", "matched", "matched_iou", "best_iou"):
    assert t.equal(getattr(got, name), getattr(want, name)), name            # every IoU is one float64 division of equal integers


def test_instance_metrics_equal_cpu():
  from corenet_amd import evaluation_results as ER
  gpu, cpu = ER.InstanceResults("semantic", min_component_voxels=3), ER.InstanceResults("semantic", min_component_voxels=3)
  for seed in (0, 1):
    got = gpu.add_batch(*_instance_case(seed, "cuda"))
    want = cpu.add_batch(*_instance_case(seed, "cpu"))
    assert got.counts.tp.is_cuda and int(want.counts.tp.sum()) > 0
    _rows_equal(got, want)
  g, c = gpu.summary(), cpu.summary()
  assert g.keys() == c.keys() and g["per_class"].keys() == c["per_class"].keys()
  for eg, ec in [(g["overall"], c["overall"])] + [(g["per_class"][k], c["per_class"][k]) for k in c["per_class"]]:
    for k in ec:
      assert (np.isnan(eg[k]) and np.isnan(ec[k])) or abs(eg[k] - ec[k]) <= 1e-12, k


def test_instance_metrics_on_the_fixture_scenes():
  """The ground-truth instances voxelized from the batch itself (one id per mesh) equal passing them in, and the one-hot
  of the semantic ground truth finds objects: scenes of 2 and 3 meshes at 32^3."""
  import os
  from corenet_amd import evaluation_results as ER, pipeline
  from corenet_amd.data import batched_example as B, dataset as D
  root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "n2_dataset")
  ds = D.CoReNetDatasetImpl(os.path.join(root, "dataset.json"), os.path.join(root, "meshes"))
  ex = pipeline.voxelize_batch(B.batch([ds[0], ds[1]]), "semantic", resolution=(32, 32, 32))
  inst = B.voxelize(ex, (32, 32, 32), B.voxel_content_mesh_index, image_resolution_multiplier=8).grid
  assert t.equal(inst > 0, ex.grid > 0) and 1 <= int(inst.amax()) <= 3
  pmf = t.nn.functional.one_hot(ex.grid.to(t.int64).clamp(0, 3), 4).permute(0, 4, 1, 2, 3).float()
  got = ER.instance_metrics_for_batch(pmf, ex, "semantic", image_resolution_multiplier=8)
  want = ER.instance_metrics_for_batch(pmf, ex, "semantic", gt_instances=inst)
  _rows_equal(got, _counts_on_host(want))
  meshes = [len(v) for v in ex.mesh_labels]
  assert sorted(meshes) == [2, 3]
  assert got.scene_index.tolist() == [b for b, m in enumerate(meshes) for _ in range(m)]
  assert got.mesh_index.tolist() == [i for m in meshes for i in range(m)]
  assert got.class_index.tolist() == t.cat([t.as_tensor(v).reshape(-1) for v in ex.mesh_labels]).tolist()
  assert int(got.counts.tp.sum() + got.counts.fn.sum()) == 5 and bool((got.best_iou[got.gt_voxels > 0] > 0).all())
  cpu_ex = types.SimpleNamespace(scene_id=ex.scene_id, mesh_labels=ex.mesh_labels, grid=ex.grid.cpu())
  _rows_equal(got, ER.instance_metrics_for_batch(pmf.cpu(), cpu_ex, "semantic", gt_instances=inst.cpu()))


def _counts_on_host(rows):
  """InstanceRows with its counts on the host, as _rows_equal expects of its second argument."""
  return rows._replace(counts=type(rows.counts)(*(x.cpu() for x in rows.counts)))
