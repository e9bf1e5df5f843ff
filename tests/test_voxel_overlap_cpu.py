"""Label overlaps on the host (csrc/voxel_overlap_cpu.cpp, corenet_amd/voxel_overlap.py): the twin
against np.unique, the matching and the panoptic counts against explicit loops over segment pairs (voxel_overlap_check),
hand-made cases with known answers, and the per-object evaluation of evaluation_results on CPU tensors.  The GPU is
compared with the twin in test_voxel_overlap_gpu.py."""
import types

import numpy as np
import pytest
import torch as t

import voxel_overlap_check as VC


@pytest.fixture(scope="module")
def M():
  from corenet_amd import voxel_overlap as M
  return M


def _np(x):
  return x.numpy() if isinstance(x, t.Tensor) else np.asarray(x)


def _check(M, a, b, num_a=None, num_b=None, **kw):
  """label_overlaps(a, b) == oracle, field by field; a, b: CPU tensors or arrays."""
  a, b = t.as_tensor(a), t.as_tensor(b)
  got = M.label_overlaps(a, b, num_a, num_b, **kw)
  want = VC.oracle_overlaps(_np(a), _np(b), None if num_a is None else _np(num_a), None if num_b is None else _np(num_b))
  assert got.offsets.dtype == t.int64 and got.a.dtype == t.int32 and got.b.dtype == t.int32 and got.count.dtype == t.int64
  for name, x, y in zip(got._fields, got, want):
    assert np.array_equal(x.numpy(), y), name
  return got


@pytest.mark.parametrize("labels", [(1, 1), (3, 3), (200, 100)])
def test_random_grids(M, labels):
  rng = np.random.default_rng(labels[0])
  shape = (3, 7, 18, 37)
  for runs in (True, False):
    got = _check(M, VC.random_labels(rng, shape, labels[0], runs=runs), VC.random_labels(rng, shape, labels[1], runs=runs))
    assert int(got.bad.sum()) == 0 and int(got.count.sum()) == int(np.prod(shape))


def test_dtypes(M):
  rng = np.random.default_rng(5)
  shape = (2, 5, 9, 21)
  u, i = VC.random_labels(rng, shape, 7, np.uint8), VC.random_labels(rng, shape, 300, np.int32)
  _check(M, u, i)
  _check(M, i, u)
  _check(M, u, u[::-1].copy())
  _check(M, i.astype(np.int64), u.astype(np.int16))
  mask = t.from_numpy(u > 3)
  got = M.label_overlaps(mask, t.from_numpy(i))
  want = VC.oracle_overlaps((u > 3).astype(np.int64), i)
  assert all(np.array_equal(x.numpy(), y) for x, y in zip(got, want))
  with pytest.raises(ValueError):
    M.label_overlaps(t.from_numpy(i).float(), t.from_numpy(u))


def test_strided_views(M):
  rng = np.random.default_rng(6)
  a, b = t.from_numpy(VC.random_labels(rng, (2, 8, 6, 35), 9)), t.from_numpy(VC.random_labels(rng, (2, 8, 6, 35), 4, np.uint8))
  _check(M, a[:, ::2], b[:, ::2])
  _check(M, a[..., 1:], b[..., 1:])
  _check(M, a[..., 1:], b[..., :-1])                 # alignments that never agree
  _check(M, a[:, :, ::3], b[:, :, 1::3])
  _check(M, a[..., ::2], b[..., ::2])                # W stride 2: copied
  _check(M, a[:1].expand(2, -1, -1, -1), b)          # N stride 0


def test_empty_batch(M):
  got = M.label_overlaps(t.zeros((0, 4, 5, 6), dtype=t.int32), t.zeros((0, 4, 5, 6), dtype=t.uint8))
  assert got.offsets.tolist() == [0] and all(x.numel() == 0 for x in got[1:])
  sizes = M.segment_sizes(got)
  assert sizes[0].numel() == 0 and sizes[2].tolist() == [0]
  m = M.match_segments(got)
  assert M.panoptic_quality(m, 2).tp.shape == (0, 2)


def test_bad_labels(M):
  rng = np.random.default_rng(7)
  a, b = VC.random_labels(rng, (2, 4, 5, 19), 6), VC.random_labels(rng, (2, 4, 5, 19), 5)
  a[0, 0, 0, :3] = -1
  b[1, 3, 4, 18] = -7
  got = _check(M, a, b, num_a=[4, 6], num_b=[5, 2])
  assert (got.bad > 0).all() and int(got.count.sum() + got.bad.sum()) == a.size
  _check(M, a, b, num_a=[0, 0], num_b=[0, 0])
  with pytest.raises(ValueError):
    M.label_overlaps(t.from_numpy(a), t.from_numpy(b), num_a=[4, -1])


def test_sizes_are_histograms(M):
  rng = np.random.default_rng(8)
  a, b = VC.random_labels(rng, (3, 6, 7, 23), 11), VC.random_labels(rng, (3, 6, 7, 23), 5, np.uint8)
  size_a, size_b, off_a, off_b = M.segment_sizes(M.label_overlaps(t.from_numpy(a), t.from_numpy(b), num_a=[11, 12, 11], num_b=[5, 5, 7]))
  assert off_a.tolist() == [0, 12, 25, 37] and off_b.tolist() == [0, 6, 12, 20]
  for n, (na, nb) in enumerate(((11, 5), (12, 5), (11, 7))):
    assert np.array_equal(size_a[off_a[n]:off_a[n + 1]].numpy(), VC.oracle_sizes(a[n], na))
    assert np.array_equal(size_b[off_b[n]:off_b[n + 1]].numpy(), VC.oracle_sizes(b[n], nb))


def test_component_sizes(M):
  from corenet_amd import voxel_components as VCo
  rng = np.random.default_rng(9)
  grid = t.from_numpy(VC.random_labels(rng, (2, 9, 10, 11), 2, background=0.5))
  comps = VCo.connected_components(grid)
  stats = VCo.component_stats(comps)
  ov = M.label_overlaps(comps.labels, grid, comps.num_components)
  size_a, _, off_a, _ = M.segment_sizes(ov)
  fg = t.ones(size_a.numel(), dtype=t.bool)
  fg[off_a[:-1]] = False
  assert t.equal(size_a[fg], stats.size)
  assert bool((ov.count[ov.a > 0] == size_a[fg]).all())                    # by value: a component meets one label of its grid


def test_forced_paths_agree(M):
  rng = np.random.default_rng(10)
  a, b = VC.random_labels(rng, (4, 5, 8, 29), 20), VC.random_labels(rng, (4, 5, 8, 29), 9)
  a[2] %= 3                                                                  # grid 2: a table of 3 x 10
  full = _check(M, a, b)
  for cap in (1, 29, 30, 210, 211, 450):                                     # all sorted / mixed / one grid per group / two
    got = _check(M, a, b, _max_table_entries=cap)
    assert all(t.equal(x, y) for x, y in zip(got, full))


def test_argument_errors(M):
  z = t.zeros((1, 2, 3, 4), dtype=t.int32)
  for bad_a, bad_b in ((z[0], z[0]), (z, z[:, :1]), (z, t.zeros((2, 2, 3, 4), dtype=t.int32)), (t.zeros((1, 0, 3, 4), dtype=t.int32),) * 2):
    with pytest.raises(ValueError):
      M.label_overlaps(bad_a, bad_b)
  for num in ([0, 0], [0.5], [[0]]):
    with pytest.raises(ValueError):
      M.label_overlaps(z, z, num_a=t.tensor(num))
  ov = M.label_overlaps(z, z)
  for thr in (0.49, 0.0, -1.0, float("nan")):
    with pytest.raises(ValueError):
      M.match_segments(ov, iou_threshold=thr)
  with pytest.raises(ValueError):
    M.match_segments(ov, class_a=t.zeros(1, dtype=t.int32))
  with pytest.raises(ValueError):
    M.match_segments(ov, class_a=t.zeros(2, dtype=t.int32), class_b=t.zeros(1, dtype=t.int32))
  with pytest.raises(ValueError):
    M.match_segments(ov, min_voxels_a=-1)
  with pytest.raises(ValueError):
    M.panoptic_quality(M.match_segments(ov), 0)
  one = t.ones((1, 1, 1, 2), dtype=t.int32)
  with pytest.raises(ValueError):                                            # class 3 with num_classes 3
    M.panoptic_quality(M.match_segments(M.label_overlaps(one, one), t.tensor([0, 3]), t.tensor([0, 3])), 3)


def _csr_classes(per_grid):
  return t.tensor([c for g in per_grid for c in g], dtype=t.int32)


def _match_check(M, a, b, num_a, num_b, class_a=None, class_b=None, thr=0.5, num_classes=1, min_voxels_a=0):
  """match_segments + panoptic_quality == the loop oracle, grid by grid.  class_*: per grid a list indexed by label."""
  ov = M.label_overlaps(t.from_numpy(a), t.from_numpy(b), num_a, num_b)
  m = M.match_segments(ov, None if class_a is None else _csr_classes(class_a), None if class_b is None else _csr_classes(class_b),
                       iou_threshold=thr, min_voxels_a=min_voxels_a)
  pq = M.panoptic_quality(m, num_classes)
  for n in range(a.shape[0]):
    want = VC.oracle_match_pq(a[n], b[n], num_a[n], num_b[n], None if class_a is None else class_a[n],
                              None if class_b is None else class_b[n], thr, num_classes, min_voxels_a)
    sa, sb = slice(int(m.offsets_a[n]), int(m.offsets_a[n + 1])), slice(int(m.offsets_b[n]), int(m.offsets_b[n + 1]))
    assert m.size_a[sa].tolist() == want["size_a"] and m.size_b[sb].tolist() == want["size_b"]
    assert m.partner_a[sa].tolist() == want["partner_a"] and m.partner_b[sb].tolist() == want["partner_b"]
    assert m.iou_a[sa].tolist() == want["iou_a"] and m.iou_b[sb].tolist() == want["iou_b"]      # one float64 division each
    assert m.best_iou_b[sb].tolist() == want["best_iou_b"]
    assert pq.tp[n].tolist() == want["tp"] and pq.fp[n].tolist() == want["fp"] and pq.fn[n].tolist() == want["fn"]
    np.testing.assert_allclose(pq.sum_iou[n].numpy(), want["sum_iou"], rtol=0, atol=1e-13)       # a few terms <= 1, any order
  return m, pq


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_matching_random(M, seed):
  rng = np.random.default_rng(seed)
  N, shape, K = 3, (10, 12, 14), 7
  b = np.stack([VC.blobs(rng, shape, K, 4) for _ in range(N)])
  a = np.roll(b, 1, axis=3)                                                  # most objects still overlap themselves well
  a[:, :, :, :2] = np.stack([VC.blobs(rng, shape, K, 3) for _ in range(N)])[:, :, :, :2]
  a[0][a[0] == 2] = 1                                                        # a fused pair
  cls_a = [[0] + [int(v) for v in rng.integers(1, 3, K)] for _ in range(N)]
  cls_b = [list(c) for c in cls_a]
  cls_b[1][3] = 3 - cls_b[1][3] if cls_b[1][3] in (1, 2) else 1
  _match_check(M, a, b, [K] * N, [K + 1] * N)                                # label K + 1 of b has no voxel: a false negative
  _match_check(M, a, b, [K] * N, [K] * N, cls_a, cls_b, num_classes=3)
  _match_check(M, a, b, [K] * N, [K] * N, cls_a, cls_b, thr=0.75, num_classes=4, min_voxels_a=12)


def test_iou_exactly_half_does_not_match(M):
  a = np.array([1, 1, 0, 0], np.int32).reshape(1, 1, 1, 4)
  b = np.array([1, 0, 0, 0], np.int32).reshape(1, 1, 1, 4)
  m, pq = _match_check(M, a, b, [1], [1])
  assert m.partner_a.tolist() == [0, 0] and m.best_iou_b.tolist() == [0.0, 0.5]
  assert (pq.tp.item(), pq.fp.item(), pq.fn.item()) == (0, 1, 1)
  assert pq.pq.item() == 0.0 and np.isnan(pq.sq.item()) and pq.rq.item() == 0.0
  b[0, 0, 0, 1] = 1                                                          # identical: IoU 1
  m, pq = _match_check(M, a, b, [1], [1])
  assert (pq.tp.item(), pq.fp.item(), pq.fn.item(), pq.sum_iou.item()) == (1, 0, 0, 1.0) and pq.pq.item() == 1.0
  empty = M.panoptic_quality(M.match_segments(M.label_overlaps(t.zeros((1, 1, 1, 4), dtype=t.int32), t.zeros((1, 1, 1, 4), dtype=t.int32))), 1)
  assert np.isnan(empty.pq.item()) and np.isnan(empty.rq.item())


def test_different_class_does_not_match(M):
  a = np.array([1, 1, 1, 0, 2, 2], np.int32).reshape(1, 1, 1, 6)
  m, pq = _match_check(M, a, a.copy(), [2], [2], [[0, 1, 2]], [[0, 1, 1]], num_classes=3)
  assert m.partner_a.tolist() == [0, 1, 0] and m.best_iou_b.tolist() == [0.0, 1.0, 0.0]
  assert pq.tp.tolist() == [[0, 1, 0]] and pq.fp.tolist() == [[0, 0, 1]] and pq.fn.tolist() == [[0, 1, 0]]


def test_fused_objects(M):
  """One predicted component over two ground-truth objects: it matches the one that holds more than half of the union."""
  b = np.array([1, 1, 1, 1, 1, 1, 1, 2, 2, 0], np.int32).reshape(1, 1, 1, 10)
  a = (b > 0).astype(np.int32)
  m, pq = _match_check(M, a, b, [1], [2])                                    # IoU 7/9 and 2/9
  assert m.partner_a.tolist() == [0, 1] and m.partner_b.tolist() == [0, 1, 0]
  assert (pq.tp.item(), pq.fp.item(), pq.fn.item()) == (1, 0, 1)
  b = np.array([1, 1, 1, 1, 2, 2, 2, 2, 0, 0], np.int32).reshape(1, 1, 1, 10)
  m, pq = _match_check(M, (b > 0).astype(np.int32), b, [1], [2])             # IoU 1/2 each: nothing matches
  assert (pq.tp.item(), pq.fp.item(), pq.fn.item()) == (0, 1, 2)


def test_min_voxels_equals_filtering(M):
  from corenet_amd import voxel_components as VCo
  rng = np.random.default_rng(11)
  pred = t.from_numpy(VC.random_labels(rng, (2, 8, 9, 10), 2, background=0.6))
  gt = t.from_numpy(np.stack([VC.blobs(rng, (8, 9, 10), 4, 3) for _ in range(2)]))
  comps = VCo.connected_components(pred)
  kept = VCo.connected_components(VCo.filter_components(pred, min_voxels=4))
  assert int(kept.num_components.sum()) < int(comps.num_components.sum())
  folded = M.match_segments(M.label_overlaps(comps.labels, gt, comps.num_components, [4, 4]), min_voxels_a=4)
  direct = M.match_segments(M.label_overlaps(kept.labels, gt, kept.num_components, [4, 4]))
  fa, da = folded.valid_a, direct.valid_a
  assert int(fa.sum()) == int(da.sum()) == int(kept.num_components.sum())   # the kept components, in the same order
  assert t.equal(folded.size_a[fa], direct.size_a[da]) and t.equal(folded.iou_a[fa], direct.iou_a[da])
  assert t.equal(folded.partner_a[fa], direct.partner_a[da])
  assert t.equal(folded.size_a[folded.offsets_a[:-1]], direct.size_a[direct.offsets_a[:-1]])   # the backgrounds grew alike
  assert t.equal(folded.best_iou_b, direct.best_iou_b) and t.equal(folded.iou_b, direct.iou_b)
  assert all(t.equal(x, y) for x, y in zip(M.panoptic_quality(folded, 1), M.panoptic_quality(direct, 1)))


# ---- evaluation_results: per-object evaluation on CPU tensors (voxelize needs the GPU, so gt_instances is given) ----
def instance_case(seed, B=2, shape=(10, 12, 14), C=4):
  """A hand-made batch: (pmf one-hot of the semantic ground truth, ex, gt_instances).  The last mesh of every scene
  leaves no voxel."""
  sem, labels, inst = VC.instance_arrays(seed, B, shape, C)
  pmf = t.from_numpy(np.stack([(sem == c) for c in range(C)], 1).astype(np.float32))
  ex = types.SimpleNamespace(scene_id=[f"scene{seed}_{b}" for b in range(B)], mesh_labels=[t.from_numpy(v) for v in labels],
                             grid=t.from_numpy(sem))
  return pmf, ex, t.from_numpy(inst)


def check_instance_rows(rows, pmf, ex, inst, C, min_voxels=0):
  """rows == the loop oracle on the components of the predicted labels."""
  from corenet_amd import voxel_components as VCo
  pred = pmf.argmax(1).to(t.int32).cpu()
  comps = VCo.connected_components(pred)
  stats = VCo.component_stats(comps, pred)
  at = 0
  for b in range(pmf.shape[0]):
    k = int(comps.num_components[b])
    cls_a = [0] + stats.value[int(stats.offsets[b]):int(stats.offsets[b + 1])].tolist()
    cls_b = [0] + ex.mesh_labels[b].tolist()
    want = VC.oracle_match_pq(comps.labels[b].numpy(), inst[b].cpu().numpy(), k, len(cls_b) - 1, cls_a, cls_b, 0.5, C, min_voxels)
    assert rows.counts.tp[b].tolist() == want["tp"] and rows.counts.fp[b].tolist() == want["fp"] and rows.counts.fn[b].tolist() == want["fn"]
    np.testing.assert_allclose(rows.counts.sum_iou[b].cpu().numpy(), want["sum_iou"], rtol=0, atol=1e-13)
    m = len(cls_b) - 1
    sl = slice(at, at + m)
    assert rows.scene_index[sl].tolist() == [b] * m and rows.mesh_index[sl].tolist() == list(range(m))
    assert rows.class_index[sl].tolist() == cls_b[1:] and rows.gt_voxels[sl].tolist() == want["size_b"][1:]
    assert rows.matched[sl].tolist() == [p > 0 for p in want["partner_b"][1:]]
    assert rows.matched_iou[sl].tolist() == want["iou_b"][1:] and rows.best_iou[sl].tolist() == want["best_iou_b"][1:]
    assert rows.gt_voxels[at + m - 1] == 0 and not rows.matched[at + m - 1]   # the mesh without voxels: a false negative
    at += m
  assert at == rows.scene_index.numel()


def test_instance_metrics_for_batch():
  from corenet_amd import evaluation_results as ER
  pmf, ex, inst = instance_case(0)
  rows = ER.instance_metrics_for_batch(pmf, ex, "semantic", gt_instances=inst)
  check_instance_rows(rows, pmf, ex, inst, 4)
  assert int(rows.counts.tp.sum()) > 0 and int(rows.counts.fn.sum()) >= 2
  rows = ER.instance_metrics_for_batch(pmf, ex, "semantic", gt_instances=inst, min_component_voxels=30)
  check_instance_rows(rows, pmf, ex, inst, 4, min_voxels=30)
  with pytest.raises(ValueError):
    ER.instance_metrics_for_batch(pmf, ex, "semantic", gt_instances=inst + 9 * (inst > 0))
  with pytest.raises(ValueError):
    ER.instance_metrics_for_batch(pmf, ex, "semantic", gt_instances=inst[:, :5])


def test_instance_results_summary(M):
  from corenet_amd import evaluation_results as ER
  res = ER.InstanceResults("semantic")
  all_rows = []
  for seed in (1, 2):
    pmf, ex, inst = instance_case(seed)
    all_rows.append(res.add_batch(pmf, ex, gt_instances=inst))
  s = res.summary()
  tp = sum(r.counts.tp.sum(0) for r in all_rows)
  fp = sum(r.counts.fp.sum(0) for r in all_rows)
  fn = sum(r.counts.fn.sum(0) for r in all_rows)
  si = sum(r.counts.sum_iou.sum(0) for r in all_rows)
  cls = t.cat([r.class_index for r in all_rows])
  best = t.cat([r.best_iou for r in all_rows])
  assert res.scene_id == ["scene1_0", "scene1_1", "scene2_0", "scene2_1"]

  def same(x, y):
    return (np.isnan(x) and np.isnan(y)) or abs(x - y) <= 1e-12
  for c, e in s["per_class"].items():
    assert (e["tp"], e["fp"], e["fn"]) == (int(tp[c]), int(fp[c]), int(fn[c])) and e["num_objects"] == int((cls == c).sum())
    den = float(tp[c]) + 0.5 * float(fp[c]) + 0.5 * float(fn[c])
    assert same(e["pq"], float(si[c]) / den) and same(e["rq"], float(tp[c]) / den)
    assert same(e["sq"], float(si[c]) / float(tp[c]) if int(tp[c]) else float("nan"))
    if e["num_objects"]:
      assert same(e["mean_best_iou"], float(best[cls == c].mean()))
      assert same(e["components_per_object"], float(tp[c] + fp[c]) / e["num_objects"])
  assert sorted(s["per_class"]) == [c for c in range(4) if int(tp[c] + fp[c] + fn[c])]
  o = s["overall"]
  den = float(tp.sum()) + 0.5 * float(fp.sum()) + 0.5 * float(fn.sum())
  assert (o["tp"], o["fp"], o["fn"], o["num_objects"]) == (int(tp.sum()), int(fp.sum()), int(fn.sum()), cls.numel())
  assert same(o["pq"], float(si.sum()) / den) and same(o["sq"], float(si.sum()) / float(tp.sum())) and same(o["mean_best_iou"], float(best.mean()))
