"""Qualitative eval results (reference: evaluation_results.py:42-174): one PNG per scene with five camera rows (the
dataset camera, then four tetrahedron views) of five panels each: the input image, the marching-cubes surface of the
prediction, the ground-truth meshes, the predicted label grid and the ground-truth label grid.

The reference renders every panel from every camera on its own (20 GL renders per scene, each copied to the host).
visualize_output gathers all 3D panels x cameras of the requested batch elements into ONE batched render
(render.render_batch), after one marching-cubes call and one voxel-face call, and gives the same pictures as the
artifact-by-artifact path of visualization.artifacts.  CUDA inputs render on the GPU, CPU inputs through the host twin;
both give identical images.  TensorBoard output is out of scope.

Quantitative surface results (no counterpart in the reference, which reports voxel IoU only): surface_metrics_for_batch
measures the same marching-cubes surfaces against the ground truth with Chamfer distance and F-score
(corenet_amd.mesh_metrics) and SurfaceResults accumulates them over an evaluation run.  With
distance="triangles" the distances run from the samples of one surface to the triangles of the other and normal
consistency is reported beside them.

Quantitative voxel results (evaluation_results.py:185-279): QuantitativeResults accumulates the confusion matrix over the
dataset's classes on the device (`crn_eval_labels`: from a pmf, or streamed pass by pass at the resolution of the ground
truth), compute_voxel_metrics turns it into the reference's table (iou / precision / recall per class
plus the class-agnostic `__global__` column) and MetricsTable.to_csv writes what pandas writes for it, without pandas.

Score-level results (no counterpart in the reference): ScoreResults accumulates the per-class score histogram of
corenet_amd.score_metrics (`crn_eval_scores`) the same way and reports calibration, Brier score,
average precision and the threshold sweep.

Topology results (no counterpart in the reference): topology_metrics_for_batch compares the Betti numbers, volume,
exposed faces and Crofton area of prediction and ground truth per (scene, class) (corenet_amd.voxel_topology, DESIGN
section 23) and TopologyResults accumulates them."""
from __future__ import annotations

import csv
import io
import os
from typing import Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import PIL.Image
import torch as t

from corenet_amd import distributed as dist_util
from corenet_amd import mesh_metrics, voxel_metrics
from corenet_amd.geometry import transformations
from corenet_amd.visualization import artifacts as vis
from corenet_amd.visualization import colors, render
from corenet_amd.visualization.marching_cubes import _triangle_soup, marching_cubes

IMAGE_SIZE = (384, 384)


def _task(task_type) -> str:
  task = getattr(task_type, "value", task_type)
  task = str(task).lower()
  if task not in ("fg_bg", "semantic"):
    raise ValueError(f"unknown task type {task_type!r}")
  return task


def extract_labels(pmf: t.Tensor, b, task_type):
  """(predicted labels int32 [B, D, H, W], ground truth [B, D, H, W]) for a task (evaluation_results.py:42-54): the
  argmax class, and for fg_bg both multiplied by the scene's mesh label."""
  pred = pmf.argmax(dim=1).to(t.int32)
  gt = b.grid
  if _task(task_type) == "fg_bg":
    labels = t.cat([t.as_tensor(v).reshape(-1) for v in b.mesh_labels]).to(pred.device, t.int32)[:, None, None, None]
    pred = pred * labels
    gt = gt * labels
  return pred, gt


def visualize_output(pmf: t.Tensor, ex, task_type, batch_indices: Optional[Iterable[int]] = None) -> List[List[t.Tensor]]:
  """Per requested batch element, five uint8 rows [384, 1920, 3] on pmf's device (evaluation_results.py:57-118).

  pmf f32 [B, C, D, H, W] class probabilities; ex the voxelized BatchedExample (grid, v2x_transform, vertices, ...).
  Cameras, boxes and matrices are built on the host in float32, and every box is computed with device-independent
  arithmetic (artifacts.points_box, render.voxel_faces), so the GPU and the host path draw the same pictures."""
  task = _task(task_type)
  dev = pmf.device
  B, C = pmf.shape[:2]
  idx = [int(i) for i in batch_indices] if batch_indices else list(range(B))
  if len(ex.scene_id) != B or any(not 0 <= i < B for i in idx):
    raise ValueError(f"visualize_output: pmf has {B} elements, the batch {len(ex.scene_id)}, indices {idx}")
  n = len(idx)
  palette = t.as_tensor(colors.DEFAULT_COLOR_PALETTE, dtype=t.float32)
  pred_lbl, gt_lbl = extract_labels(pmf, ex, task)
  mesh_num_tri = [t.as_tensor(v).to(t.int64).cpu() for v in ex.mesh_num_tri]
  mesh_labels = [t.as_tensor(v).to(t.int64).cpu().reshape(-1) for v in ex.mesh_labels]
  scene_num_tri = [int(v.sum()) for v in mesh_num_tri]
  offsets = [sum(scene_num_tri[:b]) for b in range(B)]
  v2x_inv = [ex.v2x_transform[b].detach().cpu().to(t.float32).inverse() for b in idx]
  world_to_view = [ex.view_transform[b].detach().cpu().to(t.float32) for b in idx]
  view_to_world = [t.inverse(m) for m in world_to_view]
  default_cams = [ex.camera_transform[b].detach().cpu().to(t.float32) for b in idx]

  # marching cubes of every foreground class of every element, in one call
  K = C - 1
  mc_mats = t.stack([v2x_inv[e] for e in range(n) for _ in range(K)])
  mesh = marching_cubes(pmf[idx][:, 1:].reshape((n * K,) + tuple(pmf.shape[2:])), level=0.5, matrices=mc_mats.to(dev))
  mh = mc_mats.to(t.float64)
  h = mh @ t.ones(4, dtype=t.float64)
  dummy_v = (h[:, :3] / h[:, 3:]).to(t.float32)[:, None, :].expand(n * K, 3, 3)
  dummy_n = (mh[:, :3, :3] @ t.ones(3, dtype=t.float64)).to(t.float32)[:, None, :].expand(n * K, 3, 3)
  mc_tri, mc_nrm, mc_cnt = _triangle_soup(mesh, dummy_v, dummy_n)
  mc_cnt = mc_cnt.to(t.int64).cpu()

  # exposed voxel faces of the predicted and the ground-truth grids, in one call
  grids = t.cat([pred_lbl[idx], gt_lbl[idx].to(dev, t.int32)], 0)
  vmats = t.stack(v2x_inv + v2x_inv)
  bmats = t.stack([transformations.chain([view_to_world[e % n], v2x_inv[e % n]]) for e in range(2 * n)])
  faces = render.voxel_faces(grids, palette, vmats, material_base=0, box_matrices=bmats)
  vox_cnt = faces.num_triangles.cpu()
  vox_box = faces.boxes.cpu()

  # materials: the voxel palette at 0, then per element the marching-cubes and the ground-truth mesh colours
  P = palette.shape[0]
  mats = [render.voxel_materials(palette)]
  base, mc_base, gt_base = P, [], []
  for e, b in enumerate(idx):
    if task == "fg_bg":
      assert mesh_labels[b].shape == (1,)
      mc_colors = palette[mesh_labels[b]]
    else:
      mc_colors = palette[1:C]
    mc_base.append(base)
    mats.append(render.make_materials(mc_colors))
    base += mc_colors.shape[0]
    gt_base.append(base)
    mats.append(render.make_materials(palette[mesh_labels[b]]))
    base += mesh_labels[b].shape[0]
  mats = t.cat(mats, 0)

  # one buffer of triangles: [mc of all elements][gt meshes of all elements][voxel faces of all grids]
  gt_tri = [ex.vertices[offsets[b]:offsets[b] + scene_num_tri[b]].to(dev, t.float32) for b in idx]
  mc_mid = t.repeat_interleave(t.tensor([mc_base[e] + k for e in range(n) for k in range(K)], dtype=t.int32), mc_cnt)
  gt_mid = [t.repeat_interleave(t.arange(len(mesh_num_tri[b]), dtype=t.int32) + gt_base[e], mesh_num_tri[b])
            for e, b in enumerate(idx)]
  T_mc, T_gt = int(mc_cnt.sum()), sum(scene_num_tri[b] for b in idx)
  tri = t.cat([mc_tri.to(dev), *gt_tri, faces.triangles], 0)
  nrm = t.cat([mc_nrm.to(dev), t.zeros((T_gt, 3, 3), dtype=t.float32, device=dev), faces.normals], 0)
  mid = t.cat([mc_mid.to(dev), *[g.to(dev) for g in gt_mid], faces.material_ids], 0)

  # per element: the panels' triangle ranges and boxes -> the four extra cameras
  mc_start = t.cumsum(mc_cnt.reshape(n, K).sum(1), 0) - mc_cnt.reshape(n, K).sum(1)
  gt_start = T_mc
  vox_start = t.cumsum(vox_cnt, 0) - vox_cnt + T_mc + T_gt
  ranges, vps, modes = [], [], []
  aspect = IMAGE_SIZE[1] / IMAGE_SIZE[0]
  for e, b in enumerate(idx):
    r_mc = (int(mc_start[e]), int(mc_start[e]) + int(mc_cnt[e * K:(e + 1) * K].sum()))
    r_gt = (gt_start, gt_start + scene_num_tri[b])
    gt_start += scene_num_tri[b]
    r_pv = (int(vox_start[e]), int(vox_start[e]) + int(vox_cnt[e]))
    r_gv = (int(vox_start[n + e]), int(vox_start[n + e]) + int(vox_cnt[n + e]))
    boxes = [vis.points_box(tri[r_mc[0]:r_mc[1]].reshape(-1, 3), view_to_world[e]),
             vis.points_box(tri[r_gt[0]:r_gt[1]].reshape(-1, 3), view_to_world[e])]
    boxes = [x.cpu() for x in boxes] + [vox_box[e], vox_box[n + e]]
    ltf = t.stack([x[0] for x in boxes]).min(0)[0]
    rbb = t.stack([x[1] for x in boxes]).max(0)[0]
    cams = [default_cams[e]] + vis.extra_views_for_box(ltf, rbb, aspect, view_to_world[e])
    for cam in cams:
      for r, mode in ((r_mc, 1), (r_gt, 0), (r_pv, 2), (r_gv, 2)):
        ranges.append(r)
        vps.append(cam)
        modes.append(mode)
  imgs = render.render_batch(tri, mid, mats.to(dev), ranges, t.stack(vps), IMAGE_SIZE, normals=nrm, normal_modes=modes,
                             cull_back_facing=False)
  imgs = imgs.reshape(n, 5, 4, IMAGE_SIZE[0], IMAGE_SIZE[1], 3)
  out = []
  for e, b in enumerate(idx):
    picture = vis.resize_image(ex.input_image[b], IMAGE_SIZE).to(dev)
    out.append([t.cat([picture] + [imgs[e, c, p] for p in range(4)], 1) for c in range(5)])
  return out


class QualitativeResults:
  """Writes img_<scene_id with / -> _>.png (the five rows stacked) for the first num_qualitative_results scenes of
  the dataset (evaluation_results.py:121-174, without the TensorBoard part)."""

  def __init__(self, dataset, image_output_dir: str, task_type="fg_bg", num_qualitative_results: int = 10):
    n = min(int(num_qualitative_results), len(dataset))
    self.disk_result_ids = {dataset[i].scene_id for i in range(n)}
    self.image_output_dir = image_output_dir
    self.task_type = task_type

  def _write_image(self, scene_id: str, scene_images: List[t.Tensor]):
    image = t.cat(scene_images, dim=0)
    fn = os.path.join(self.image_output_dir, "img_%s.png" % scene_id.replace("/", "_"))
    os.makedirs(os.path.dirname(fn) or ".", exist_ok=True)
    PIL.Image.fromarray(image.cpu().numpy()).save(fn, format="png")

  def wants(self, ex) -> bool:
    """Whether add_batch would draw anything of this batch (callers that can score without a pmf compute one only then)."""
    return any(v in self.disk_result_ids for v in ex.scene_id)

  def add_batch(self, pmf: t.Tensor, ex):
    """Renders and writes the batch elements whose scene is of interest."""
    batch_indices = [i for i, v in enumerate(ex.scene_id) if v in self.disk_result_ids]
    if not batch_indices:
      return
    for i, images in zip(batch_indices, visualize_output(pmf, ex, self.task_type, batch_indices)):
      self._write_image(ex.scene_id[i], images)


# F-score thresholds in view-space units (the scene cube has side 1): 1 %, 2 % and 5 % of the side.  1 % is the
# threshold of Tatarchenko et al., "What Do Single-view 3D Reconstruction Networks Learn?" (CVPR 2019); it is 1.28 voxels
# of a 128^3 grid, 2 % and 5 % are the coarser levels usually listed beside it.
DEFAULT_SURFACE_THRESHOLDS = (0.01, 0.02, 0.05)


class SurfaceRows(NamedTuple):
  """One row per (scene, foreground class), scene-major: row b * (C - 1) + k is class k + 1 of batch element b."""
  scene_index: t.Tensor                    # i64 [R], host
  class_index: t.Tensor                    # i64 [R], host: 1 .. C - 1
  scene_id: List[str]                      # [R]
  thresholds: Tuple[float, ...]            # [K]
  metrics: mesh_metrics.SurfaceMetrics     # [R] / [R, K] on pmf's device; NaN rows: class absent on both sides
                                           # (a mesh_metrics.MeshSurfaceMetrics for distance="triangles")


def _mc_soup(grids: t.Tensor, matrices: t.Tensor, level: float) -> Tuple[t.Tensor, t.Tensor]:
  """One marching-cubes call over grids [n, D, H, W] -> (triangles f32 [T, 3, 3] through matrices, triangles per object
  int64 [n] on the host)."""
  m = marching_cubes(grids, level=level, matrices=matrices)
  nf = m.num_faces.cpu()
  vbase = t.cumsum(m.num_vertices, 0) - m.num_vertices
  owner = t.repeat_interleave(t.arange(len(nf), device=grids.device), m.num_faces, output_size=int(nf.sum()))
  return m.vertices[m.faces.to(t.int64) + vbase[owner][:, None]], nf


def _point_sets(triangles: t.Tensor, num_tri: t.Tensor, num_samples: int, seed: int) -> Tuple[t.Tensor, t.Tensor]:
  """One sampling call -> (points f32 [P, 3], offsets int64 [n + 1] on the host); an object without a triangle of
  positive area has no points."""
  s = mesh_metrics.sample_surface_points(triangles, num_tri, num_samples, seed)
  valid = s.valid.cpu()
  off = t.cat([t.zeros(1, dtype=t.int64), t.cumsum(valid.to(t.int64) * num_samples, 0)])
  pts = s.points if bool(valid.all()) else s.points[valid.nonzero()[:, 0].to(s.points.device)]
  return pts.reshape(-1, 3), off


def surface_metrics_for_batch(pmf: t.Tensor, ex, task_type, num_samples: int = 16384,
                              thresholds: Sequence[float] = DEFAULT_SURFACE_THRESHOLDS, seed: int = 0, level: float = 0.5,
                              gt_source: str = "mesh", distance: str = "points",
                              min_component_voxels: int = 0) -> SurfaceRows:
  """Chamfer distance and F-score of the predicted surfaces of a batch against its ground truth, per (scene, class).

  pmf f32 [B, C, D, H, W] class probabilities; ex the voxelized BatchedExample.  The predicted surface of (scene b,
  class k) is the `level` marching-cubes surface of pmf[b, k], k = 1 .. C - 1, placed in view space by
  inverse(ex.v2x_transform[b]) exactly as visualize_output places its marching-cubes panels (padded index coordinates
  through the voxel -> view matrix, like the reference's MarchingCubesArtifact), so the number and the picture describe
  the same surface.  Note that this puts a voxel's sample at its far corner: the drawn and measured surface lies half a
  voxel along (+w, +h, +d) from the iso-surface of the voxel centres; with gt_source="grid" both sides share the offset.

  gt_source:
    "mesh"  the triangles of ex.vertices (view space).  fg_bg (C must be 2): all meshes of the scene; semantic: the
            meshes of each class, by ex.mesh_labels (a label outside 1 .. C - 1 has no predicted class and is left out).
    "grid"  marching cubes of the one-hot ex.grid, through the same matrices.  ShapeNet meshes carry interior faces
            (overlapping parts, double walls) that a voxel model can never recall: against "mesh" completeness and recall
            are bounded away from their ideal by those faces, against "grid" they measure the voxel surface alone.
  thresholds are distances in view-space units (the scene cube has side 1).  Both sides are sampled with the same seed,
  so identical surfaces give identical samples and a distance of exactly 0.
  distance:
    "points"     from the samples of one surface to the nearest SAMPLE of the other (chamfer_fscore).  The numbers carry
                 the sampling floor of about 0.5 sqrt(area / num_samples).
    "triangles"  from the samples of one surface to the TRIANGLES of the other (mesh_chamfer_fscore), the same two soups:
                 no floor, and rows.metrics is a MeshSurfaceMetrics with normal consistency.
  min_component_voxels > 0 removes floaters from the prediction first: of every (scene, class) the 6-connected components
  of pmf[b, k] > level with fewer voxels are set to 0 before marching cubes (corenet_amd.voxel_components); the ground
  truth is untouched.  0 (the default) runs none of that.

  Per call: one marching-cubes call for the prediction (one more for gt_source="grid"), two sampling calls, two
  nearest-neighbour (or point-to-triangle) calls; no Python loop over kernels.  A class absent on both sides gives a NaN row."""
  task = _task(task_type)
  if gt_source not in ("mesh", "grid"):
    raise ValueError(f"surface_metrics_for_batch: gt_source must be 'mesh' or 'grid', got {gt_source!r}")
  if distance not in ("points", "triangles"):
    raise ValueError(f"surface_metrics_for_batch: distance must be 'points' or 'triangles', got {distance!r}")
  if pmf.dim() != 5 or pmf.shape[1] < 2:
    raise ValueError(f"surface_metrics_for_batch: pmf must be [B, C >= 2, D, H, W], got {tuple(pmf.shape)}")
  dev = pmf.device
  B, C = pmf.shape[:2]
  K = C - 1
  if len(ex.scene_id) != B:
    raise ValueError(f"surface_metrics_for_batch: pmf has {B} elements, the batch {len(ex.scene_id)}")
  if task == "fg_bg" and K != 1:
    raise ValueError(f"surface_metrics_for_batch: fg_bg expects 2 classes, pmf has {C}")
  v2x_inv = [ex.v2x_transform[b].detach().cpu().to(t.float32).inverse() for b in range(B)]
  mats = t.stack([v2x_inv[b] for b in range(B) for _ in range(K)]).to(dev)
  pred = pmf[:, 1:].reshape((B * K,) + tuple(pmf.shape[2:]))
  if min_component_voxels > 0:
    from corenet_amd.voxel_components import filter_components
    kept = filter_components(pred > level, min_voxels=int(min_component_voxels), connectivity=6)
    pred = t.where(kept, pred, t.zeros((), dtype=pred.dtype, device=dev))
  pred_tri, pred_cnt = _mc_soup(pred, mats, level)
  if gt_source == "grid":
    classes = t.arange(1, C, device=dev, dtype=ex.grid.dtype)[None, :, None, None, None]
    onehot = (ex.grid.to(dev)[:, None] == classes).to(t.float32)
    gt_tri, gt_cnt = _mc_soup(onehot.reshape((B * K,) + tuple(pmf.shape[2:])), mats, level)
  else:
    mesh_num_tri = [t.as_tensor(v).to(t.int64).cpu().reshape(-1) for v in ex.mesh_num_tri]
    mesh_labels = [t.as_tensor(v).to(t.int64).cpu().reshape(-1) for v in ex.mesh_labels]
    if task == "fg_bg":
      gt_tri, gt_cnt = ex.vertices.to(dev, t.float32), t.stack([v.sum() for v in mesh_num_tri])
    else:
      start, pieces, cnt = 0, [], []
      for b in range(B):
        first = start + t.cumsum(mesh_num_tri[b], 0) - mesh_num_tri[b]
        for k in range(1, C):
          sel = (mesh_labels[b] == k).nonzero()[:, 0].tolist()
          pieces += [t.arange(int(first[m]), int(first[m]) + int(mesh_num_tri[b][m])) for m in sel]
          cnt.append(sum(int(mesh_num_tri[b][m]) for m in sel))
        start += int(mesh_num_tri[b].sum())
      gather = t.cat(pieces) if pieces else t.zeros(0, dtype=t.int64)
      gt_tri, gt_cnt = ex.vertices.to(dev, t.float32)[gather.to(dev)], t.tensor(cnt, dtype=t.int64)
  if distance == "triangles":
    def csr(cnt):
      return t.cat([t.zeros(1, dtype=t.int64), t.cumsum(cnt.to(t.int64).cpu(), 0)])
    metrics = mesh_metrics.mesh_chamfer_fscore(pred_tri, csr(pred_cnt), gt_tri, csr(gt_cnt), thresholds, num_samples, seed)
  else:
    pred_pts, pred_off = _point_sets(pred_tri, pred_cnt, num_samples, seed)
    gt_pts, gt_off = _point_sets(gt_tri, gt_cnt, num_samples, seed)
    metrics = mesh_metrics.chamfer_fscore(pred_pts, pred_off, gt_pts, gt_off, thresholds)
  rows = t.arange(B * K)
  return SurfaceRows(rows // K, rows % K + 1, [ex.scene_id[b] for b in range(B) for _ in range(K)],
                     tuple(float(x) for x in thresholds), metrics)


def _nanmean(x: t.Tensor, dim: int = 0) -> t.Tensor:
  keep = ~t.isnan(x)
  return t.where(keep, x, t.zeros_like(x)).sum(dim) / keep.sum(dim).to(x.dtype)       # no row kept: 0 / 0 = NaN


class SurfaceResults:
  """Accumulates surface_metrics_for_batch over an evaluation run, in the spirit of the reference's QuantitativeResults
  for IoU: add_batch(pmf, ex) takes what pipeline.evaluate_batch returns, summary() gives the mean Chamfer-L1 and F-score
  per threshold, per class and overall, over the rows that are not NaN (classes absent on both sides are skipped; a
  class present on one side only counts with Chamfer +inf and F-score 0).  With distance="triangles" it also accumulates
  normal consistency and summary() carries it per class and overall."""

  def __init__(self, task_type="fg_bg", num_samples: int = 16384, thresholds: Sequence[float] = DEFAULT_SURFACE_THRESHOLDS,
               seed: int = 0, level: float = 0.5, gt_source: str = "mesh", distance: str = "points",
               min_component_voxels: int = 0):
    if distance not in ("points", "triangles"):
      raise ValueError(f"SurfaceResults: distance must be 'points' or 'triangles', got {distance!r}")
    self.task_type = task_type
    self.distance = distance
    self.kwargs = dict(num_samples=num_samples, thresholds=tuple(thresholds), seed=seed, level=level, gt_source=gt_source)
    if distance != "points":
      self.kwargs["distance"] = distance
    if min_component_voxels > 0:
      self.kwargs["min_component_voxels"] = int(min_component_voxels)
    self.normal_consistency: List[t.Tensor] = []
    self.thresholds = tuple(float(x) for x in thresholds)
    self.scene_id: List[str] = []
    self.class_index: List[t.Tensor] = []
    self.chamfer_l1: List[t.Tensor] = []
    self.fscore: List[t.Tensor] = []

  def add_batch(self, pmf: t.Tensor, ex) -> SurfaceRows:
    rows = surface_metrics_for_batch(pmf, ex, self.task_type, **self.kwargs)
    self.scene_id += rows.scene_id
    self.class_index.append(rows.class_index)
    self.chamfer_l1.append(rows.metrics.chamfer_l1.cpu())
    self.fscore.append(rows.metrics.fscore.cpu())
    if self.distance == "triangles":
      self.normal_consistency.append(rows.metrics.normal_consistency.cpu())
    return rows

  def rows(self) -> Tuple[t.Tensor, t.Tensor, t.Tensor]:
    """(class_index i64 [R], chamfer_l1 f64 [R], fscore f64 [R, K]) of every row added so far."""
    if not self.class_index:
      return t.zeros(0, dtype=t.int64), t.zeros(0, dtype=t.float64), t.zeros((0, len(self.thresholds)), dtype=t.float64)
    return t.cat(self.class_index), t.cat(self.chamfer_l1), t.cat(self.fscore)

  def summary(self) -> Dict:
    cls, cd, f = self.rows()
    nc = t.cat(self.normal_consistency) if self.normal_consistency else t.zeros(0, dtype=t.float64)

    def entry(sel):
      e = {"chamfer_l1": float(_nanmean(cd[sel])), "fscore": [float(v) for v in _nanmean(f[sel])],
           "num_rows": int((~t.isnan(cd[sel])).sum())}
      if self.distance == "triangles":
        e["normal_consistency"] = float(_nanmean(nc[sel]))
      return e
    return {"thresholds": list(self.thresholds), "overall": entry(t.ones_like(cls, dtype=t.bool)),
            "per_class": {int(c): entry(cls == c) for c in sorted(set(cls.tolist()))}}


def _voxel_sizes(v2x_transform: t.Tensor) -> t.Tensor:
  """f32 [B] on the host: the edge of a voxel in view space, from inverse(v2x_transform[b]).  The three column norms of
  its 3x3 block must agree to 1e-4 relative: the voxel measure assumes cubic voxels."""
  sizes = []
  for b in range(v2x_transform.shape[0]):
    inv = v2x_transform[b].detach().cpu().to(t.float64).inverse()
    norms = inv[:3, :3].norm(dim=0)
    if float(norms.max() - norms.min()) > 1e-4 * float(norms.max()):
      raise ValueError(f"voxel_surface_metrics_for_batch: the voxels of scene {b} are not cubic (edges {norms.tolist()})")
    sizes.append(float(norms.mean()))
  return t.tensor(sizes, dtype=t.float32)


def voxel_surface_metrics_for_batch(pmf: t.Tensor, ex, task_type, thresholds: Sequence[float] = DEFAULT_SURFACE_THRESHOLDS,
                                    level: float = 0.5, min_component_voxels: int = 0) -> SurfaceRows:
  """Chamfer distance and F-score per (scene, class) at voxel resolution (corenet_amd.voxel_distance): the predicted set
  of (scene b, class k) is pmf[b, k] > level, the ground truth ex.grid[b] == k, a side's points are its surface voxels
  and a point's distance is the exact distance to the nearest surface voxel of the other side, in view-space units
  (voxel edge from inverse(ex.v2x_transform[b]); ValueError unless the voxels are cubic).  Deterministic, no seed, no
  marching cubes: two distance transforms per call.  Rows, thresholds and NaN conventions are those of
  surface_metrics_for_batch; min_component_voxels > 0 removes the prediction's floaters first, as there."""
  from corenet_amd.voxel_distance import voxel_surface_metrics
  task = _task(task_type)
  if pmf.dim() != 5 or pmf.shape[1] < 2:
    raise ValueError(f"voxel_surface_metrics_for_batch: pmf must be [B, C >= 2, D, H, W], got {tuple(pmf.shape)}")
  dev = pmf.device
  B, C = pmf.shape[:2]
  K = C - 1
  if len(ex.scene_id) != B:
    raise ValueError(f"voxel_surface_metrics_for_batch: pmf has {B} elements, the batch {len(ex.scene_id)}")
  if task == "fg_bg" and K != 1:
    raise ValueError(f"voxel_surface_metrics_for_batch: fg_bg expects 2 classes, pmf has {C}")
  if tuple(ex.grid.shape) != (B,) + tuple(pmf.shape[2:]):
    raise ValueError(f"voxel_surface_metrics_for_batch: ex.grid is {tuple(ex.grid.shape)}, pmf {tuple(pmf.shape)}")
  sizes = _voxel_sizes(ex.v2x_transform)
  pred = (pmf[:, 1:] > level).reshape((B * K,) + tuple(pmf.shape[2:]))
  if min_component_voxels > 0:
    from corenet_amd.voxel_components import filter_components
    pred = filter_components(pred, min_voxels=int(min_component_voxels), connectivity=6)
  classes = t.arange(1, C, device=dev, dtype=ex.grid.dtype)[None, :, None, None, None]
  gt = (ex.grid.to(dev)[:, None] == classes).reshape(pred.shape)
  metrics = voxel_surface_metrics(pred, gt, thresholds, voxel_size=sizes.repeat_interleave(K))
  rows = t.arange(B * K)
  return SurfaceRows(rows // K, rows % K + 1, [ex.scene_id[b] for b in range(B) for _ in range(K)],
                     tuple(float(x) for x in thresholds), metrics)


class VoxelSurfaceResults(SurfaceResults):
  """SurfaceResults over voxel_surface_metrics_for_batch: add_batch measures at voxel resolution; rows() and summary()
  are those of SurfaceResults."""

  def __init__(self, task_type="fg_bg", thresholds: Sequence[float] = DEFAULT_SURFACE_THRESHOLDS, level: float = 0.5,
               min_component_voxels: int = 0):
    super().__init__(task_type, thresholds=thresholds, level=level)
    self.kwargs = dict(thresholds=tuple(thresholds), level=level, min_component_voxels=int(min_component_voxels))

  def add_batch(self, pmf: t.Tensor, ex) -> SurfaceRows:
    rows = voxel_surface_metrics_for_batch(pmf, ex, self.task_type, **self.kwargs)
    self.scene_id += rows.scene_id
    self.class_index.append(rows.class_index)
    self.chamfer_l1.append(rows.metrics.chamfer_l1.cpu())
    self.fscore.append(rows.metrics.fscore.cpu())
    return rows


class VisibilityRows(NamedTuple):
  """One row per (scene, foreground class), scene-major, like SurfaceRows."""
  scene_index: t.Tensor                    # i64 [R], host
  class_index: t.Tensor                    # i64 [R], host: 1 .. C - 1
  scene_id: List[str]                      # [R]
  eye: t.Tensor                            # f64 [B, 3], host: the camera of every scene in voxel coordinates
  metrics: "VisibilityIoU"                 # [R, 2] on pmf's device: column 0 what the camera sees, column 1 what is hidden


def visibility_metrics_for_batch(pmf: t.Tensor, ex, task_type, level: float = 0.5) -> VisibilityRows:
  """IoU per (scene, class) split into the part of the grid the camera sees and the part hidden behind the scene
  (corenet_amd.voxel_visibility): the predicted set of (scene b, class k) is pmf[b, k] > level, the ground truth
  ex.grid[b] == k, and a voxel is hidden iff an occupied voxel of the WHOLE scene, ex.grid[b] > 0, lies between its
  centre and the camera -- other objects hide too.  The camera of scene b is the centre of projection of
  ex.camera_transform[b] in the voxel space of view2voxel_matrices(ex.grid_sampling_offset, resolution), where the voxel
  centres are the grid's sample points (ValueError for a camera without one, e.g. an orthographic one).  One occlusion
  call per batch; reading the camera from the device synchronises once.  Rows are those of surface_metrics_for_batch; a
  class absent on both sides of a region gives iou NaN there."""
  from corenet_amd import voxel_visibility as VV
  from corenet_amd.data.batched_example import view2voxel_matrices
  task = _task(task_type)
  if pmf.dim() != 5 or pmf.shape[1] < 2:
    raise ValueError(f"visibility_metrics_for_batch: pmf must be [B, C >= 2, D, H, W], got {tuple(pmf.shape)}")
  dev = pmf.device
  B, C = pmf.shape[:2]
  K = C - 1
  if len(ex.scene_id) != B:
    raise ValueError(f"visibility_metrics_for_batch: pmf has {B} elements, the batch {len(ex.scene_id)}")
  if task == "fg_bg" and K != 1:
    raise ValueError(f"visibility_metrics_for_batch: fg_bg expects 2 classes, pmf has {C}")
  if tuple(ex.grid.shape) != (B,) + tuple(pmf.shape[2:]):
    raise ValueError(f"visibility_metrics_for_batch: ex.grid is {tuple(ex.grid.shape)}, pmf {tuple(pmf.shape)}")
  eye = VV.eye_in_voxel_space(ex.camera_transform, view2voxel_matrices(ex.grid_sampling_offset, tuple(pmf.shape[2:])))
  grid = ex.grid.to(dev)
  hidden = VV.occlusion(grid, eye).occluded                                  # [B, D, H, W]: the whole scene occludes
  shape = (B * K,) + tuple(pmf.shape[2:])
  pred = (pmf[:, 1:] > level).reshape(shape)
  classes = t.arange(1, C, device=dev, dtype=grid.dtype)[None, :, None, None, None]
  gt = (grid[:, None] == classes).reshape(shape)
  metrics = VV._split_iou(pred, gt, hidden[:, None].expand((B, K) + tuple(pmf.shape[2:])).reshape(shape))
  rows = t.arange(B * K)
  return VisibilityRows(rows // K, rows % K + 1, [ex.scene_id[b] for b in range(B) for _ in range(K)], eye, metrics)


class VisibilityResults:
  """Accumulates visibility_metrics_for_batch over an evaluation run, in the manner of VoxelSurfaceResults:
  add_batch(pmf, ex) takes what pipeline.evaluate_batch returns; summary() gives, for the seen and the hidden region,
  the mean IoU over the rows that are not NaN and the IoU of the summed counts, per class and overall."""

  REGIONS = ("visible", "hidden")

  def __init__(self, task_type="fg_bg", level: float = 0.5):
    self.task_type = task_type
    self.level = level
    self.scene_id: List[str] = []
    self.class_index: List[t.Tensor] = []
    self.intersection: List[t.Tensor] = []
    self.union: List[t.Tensor] = []
    self.iou: List[t.Tensor] = []

  def add_batch(self, pmf: t.Tensor, ex) -> VisibilityRows:
    rows = visibility_metrics_for_batch(pmf, ex, self.task_type, level=self.level)
    self.scene_id += rows.scene_id
    self.class_index.append(rows.class_index)
    self.intersection.append(rows.metrics.intersection.cpu())
    self.union.append(rows.metrics.union.cpu())
    self.iou.append(rows.metrics.iou.cpu())
    return rows

  def rows(self) -> Tuple[t.Tensor, t.Tensor, t.Tensor, t.Tensor]:
    """(class_index i64 [R], intersection i64 [R, 2], union i64 [R, 2], iou f64 [R, 2]) of every row added so far."""
    if not self.class_index:
      z = t.zeros((0, 2), dtype=t.int64)
      return t.zeros(0, dtype=t.int64), z, z.clone(), t.zeros((0, 2), dtype=t.float64)
    return t.cat(self.class_index), t.cat(self.intersection), t.cat(self.union), t.cat(self.iou)

  def summary(self) -> Dict:
    cls, inter, union, iou = self.rows()

    def entry(sel):
      i, u = inter[sel].sum(0), union[sel].sum(0)
      pooled = t.where(u > 0, i.to(t.float64) / u.to(t.float64), t.full((), float("nan"), dtype=t.float64))
      mean = _nanmean(iou[sel])
      return {r: {"mean_iou": float(mean[c]), "pooled_iou": float(pooled[c]), "num_rows": int((~t.isnan(iou[sel][:, c])).sum())}
              for c, r in enumerate(self.REGIONS)}
    return {"overall": entry(t.ones_like(cls, dtype=t.bool)),
            "per_class": {int(c): entry(cls == c) for c in sorted(set(cls.tolist()))}}


class ReprojectionRows(NamedTuple):
  """Per scene the silhouette and depth rows; per (scene, foreground class), scene-major like SurfaceRows, the label
  rows.  Tensors are on pmf's device unless noted."""
  scene_id: List[str]                      # [B]
  silhouette: "SilhouetteCounts"           # [B]: covered pixels of prediction and ground truth
  depth: "DepthErrors"                     # [B]: sums over the pixels both cover
  scene_index: t.Tensor                    # i64 [R], host
  class_index: t.Tensor                    # i64 [R], host: 1 .. C - 1
  class_scene_id: List[str]                # [R]
  class_intersection: t.Tensor             # i64 [R]: pixels with the class's label in both label images
  class_union: t.Tensor                    # i64 [R]
  class_iou: t.Tensor                      # f64 [R], NaN where the union is 0


def reprojection_metrics_for_batch(pmf: t.Tensor, ex, task_type, image_size: Optional[Tuple[int, int]] = None,
                                   level: float = 0.5, gt: str = "grid") -> ReprojectionRows:
  """Image-space agreement of prediction and ground truth seen from the input camera (corenet_amd.image_metrics on
  render.render_geometry).

  The prediction is the label grid of extract_labels, emptied where the winning probability is not above level (for
  level >= 0.5 a voxel carries class k iff pmf[b, k] > level, the set the other metrics use), drawn as the exposed faces
  of its voxels (render.voxel_faces through inverse(ex.v2x_transform[b]): view space, as in visualize_output).  The
  ground truth is ex.grid's faces built the same way (gt="grid") or the scene's view-space triangles ex.vertices, a
  pixel's label being the mesh label of its triangle (gt="mesh").  Both are drawn from ex.camera_transform[b] without
  culling in ONE render_geometry call of 2 B images of image_size (default: the input image's (H, W)).  Per scene: the
  silhouette intersection, union and IoU; the depth-error sums over the pixels both sides cover (depth is the distance
  along the view axis); per (scene, foreground class) the intersection, union and IoU of the two label images -- for
  fg_bg the one class is the scene's label as extract_labels defines it, i.e. the silhouette again.  With gt="grid" a
  prediction equal to the ground truth draws the same triangles twice: IoU exactly 1 and every depth sum exactly 0."""
  from corenet_amd import image_metrics as IM
  task = _task(task_type)
  if gt not in ("grid", "mesh"):
    raise ValueError(f"reprojection_metrics_for_batch: gt must be 'grid' or 'mesh', got {gt!r}")
  if pmf.dim() != 5 or pmf.shape[1] < 2:
    raise ValueError(f"reprojection_metrics_for_batch: pmf must be [B, C >= 2, D, H, W], got {tuple(pmf.shape)}")
  dev = pmf.device
  B, C = pmf.shape[:2]
  K = C - 1
  if len(ex.scene_id) != B:
    raise ValueError(f"reprojection_metrics_for_batch: pmf has {B} elements, the batch {len(ex.scene_id)}")
  if task == "fg_bg" and K != 1:
    raise ValueError(f"reprojection_metrics_for_batch: fg_bg expects 2 classes, pmf has {C}")
  if tuple(ex.grid.shape) != (B,) + tuple(pmf.shape[2:]):
    raise ValueError(f"reprojection_metrics_for_batch: ex.grid is {tuple(ex.grid.shape)}, pmf {tuple(pmf.shape)}")
  if image_size is None:
    image_size = tuple(ex.input_image.shape[-2:])
  mesh_labels = [t.as_tensor(v).to(t.int64).cpu().reshape(-1) for v in ex.mesh_labels]
  if task == "fg_bg":
    if any(v.shape != (1,) for v in mesh_labels):
      raise ValueError("reprojection_metrics_for_batch: fg_bg expects one mesh label per scene")
    scene_label = t.cat(mesh_labels)
    num_labels = int(scene_label.max()) + 1
    if int(scene_label.min()) < 1:
      raise ValueError(f"reprojection_metrics_for_batch: mesh labels must be positive, got {scene_label.tolist()}")
  else:
    num_labels = C
  pred_lbl, gt_lbl = extract_labels(pmf, ex, task)
  pred_lbl = pred_lbl * (pmf.amax(dim=1) > level)
  # label 0 is not drawn; what the other labels look like does not matter
  palette = t.zeros((num_labels, 3), dtype=t.float32)
  palette[0] = -1.0
  v2x_inv = [ex.v2x_transform[b].detach().cpu().to(t.float32).inverse() for b in range(B)]
  cams = t.stack([ex.camera_transform[b].detach().cpu().to(t.float32) for b in range(B)])
  if gt == "grid":
    grids = t.cat([pred_lbl, gt_lbl.to(dev, t.int32)], 0)
    faces = render.voxel_faces(grids, palette, t.stack(v2x_inv + v2x_inv))
    tri, tri_label = faces.triangles, faces.material_ids
    counts = faces.num_triangles.cpu()
  else:
    faces = render.voxel_faces(pred_lbl, palette, t.stack(v2x_inv))
    mesh_num_tri = [t.as_tensor(v).to(t.int64).cpu().reshape(-1) for v in ex.mesh_num_tri]
    if any(n.shape != l.shape for n, l in zip(mesh_num_tri, mesh_labels)) or \
        sum(int(n.sum()) for n in mesh_num_tri) != ex.vertices.shape[0]:
      raise ValueError("reprojection_metrics_for_batch: ex.mesh_num_tri, ex.mesh_labels and ex.vertices disagree")
    tri = t.cat([faces.triangles, ex.vertices.to(dev, t.float32)], 0)
    gt_label = t.cat([t.repeat_interleave(l, n) for l, n in zip(mesh_labels, mesh_num_tri)]).to(dev, t.int32)
    tri_label = t.cat([faces.material_ids, gt_label], 0)
    counts = t.cat([faces.num_triangles.cpu(), t.stack([n.sum() for n in mesh_num_tri])])
  start = t.cumsum(counts, 0) - counts
  ranges = t.stack([start, start + counts], 1)
  buffers = render.render_geometry(tri, ranges, t.cat([cams, cams], 0), image_size, cull_back_facing=False,
                                   outputs=("triangle_index", "depth"))
  labels = render.gather_triangle_attribute(buffers, tri_label, 0)
  mask = buffers.mask
  silhouette = IM.silhouette_counts(mask[:B], mask[B:])
  depth = IM.depth_errors(buffers.depth[:B], buffers.depth[B:], mask[:B] & mask[B:])
  table = IM.label_image_overlaps(labels[:B], labels[B:], num_labels)       # [B, pred, gt]
  diag = t.diagonal(table, dim1=1, dim2=2)
  union = table.sum(2) + table.sum(1) - diag                                 # [B, num_labels]
  rows = t.arange(B * K)
  scene_index, class_index = rows // K, rows % K + 1
  label_of_row = (scene_label if task == "fg_bg" else class_index).to(dev)
  inter, union = diag[scene_index.to(dev), label_of_row], union[scene_index.to(dev), label_of_row]
  return ReprojectionRows(list(ex.scene_id), silhouette, depth, scene_index, class_index,
                          [ex.scene_id[b] for b in range(B) for _ in range(K)], inter, union, IM._iou(inter, union))


class ReprojectionResults:
  """Accumulates reprojection_metrics_for_batch over an evaluation run, in the manner of VisibilityResults:
  add_batch(pmf, ex) takes what pipeline.evaluate_batch returns.  summary() gives, for the silhouette and per class,
  the mean IoU over the rows that are not NaN and the IoU of the summed counts, and the depth errors pooled from the
  summed sums: mean_abs, rmse, abs_rel and delta1 (NaN when no pixel is covered on both sides)."""

  def __init__(self, task_type="fg_bg", image_size: Optional[Tuple[int, int]] = None, level: float = 0.5,
               gt: str = "grid"):
    self.task_type, self.image_size, self.level, self.gt = task_type, image_size, level, gt
    self.scene_id: List[str] = []
    self._scene: List[Tuple[t.Tensor, ...]] = []      # silhouette (intersection, union, iou) + the five depth fields
    self._class: List[Tuple[t.Tensor, ...]] = []      # class_index, intersection, union, iou

  def add_batch(self, pmf: t.Tensor, ex) -> ReprojectionRows:
    rows = reprojection_metrics_for_batch(pmf, ex, self.task_type, image_size=self.image_size, level=self.level,
                                          gt=self.gt)
    self.scene_id += rows.scene_id
    self._scene.append(tuple(x.cpu() for x in tuple(rows.silhouette) + tuple(rows.depth)))
    self._class.append((rows.class_index, rows.class_intersection.cpu(), rows.class_union.cpu(), rows.class_iou.cpu()))
    return rows

  def rows(self) -> Dict[str, t.Tensor]:
    """Every row added so far, on the host.  Per scene [S]: intersection, union (i64), iou (f64), depth_count (i64),
    depth_abs_sum, depth_sq_sum, depth_abs_rel_sum (f64), depth_delta1_count (i64); per (scene, class) [R]: class_index,
    class_intersection, class_union (i64), class_iou (f64)."""
    i64, f64 = t.int64, t.float64
    scene = (("intersection", i64), ("union", i64), ("iou", f64), ("depth_count", i64), ("depth_abs_sum", f64),
             ("depth_sq_sum", f64), ("depth_abs_rel_sum", f64), ("depth_delta1_count", i64))
    cls = (("class_index", i64), ("class_intersection", i64), ("class_union", i64), ("class_iou", f64))
    out = {}
    for names, parts in ((scene, self._scene), (cls, self._class)):
      for c, (name, dtype) in enumerate(names):
        out[name] = t.cat([p[c] for p in parts]) if parts else t.zeros(0, dtype=dtype)
    return out

  def summary(self) -> Dict:
    r = self.rows()
    nan = t.full((), float("nan"), dtype=t.float64)

    def entry(inter, union, iou):
      i, u = inter.sum(), union.sum()
      pooled = i.to(t.float64) / u.to(t.float64) if int(u) > 0 else nan
      return {"mean_iou": float(_nanmean(iou)), "pooled_iou": float(pooled),
              "num_rows": int((~t.isnan(iou)).sum())}
    n = r["depth_count"].sum().to(t.float64)
    div = lambda x: float(x.sum().to(t.float64) / n) if float(n) > 0 else float("nan")
    cls = r["class_index"]
    return {"silhouette": entry(r["intersection"], r["union"], r["iou"]),
            "per_class": {int(c): entry(r["class_intersection"][cls == c], r["class_union"][cls == c],
                                        r["class_iou"][cls == c]) for c in sorted(set(cls.tolist()))},
            "depth": {"num_pixels": int(n), "mean_abs": div(r["depth_abs_sum"]),
                      "rmse": div(r["depth_sq_sum"]) ** 0.5, "abs_rel": div(r["depth_abs_rel_sum"]),
                      "delta1": div(r["depth_delta1_count"])}}


class InstanceRows(NamedTuple):
  """Per (scene, class) the panoptic counts, and one row per ground-truth object, scene-major in mesh order."""
  scene_id: List[str]                      # [B]
  counts: "PanopticCounts"                 # tp / fp / fn i64, sum_iou f64 [B, num_classes] on pmf's device
  scene_index: t.Tensor                    # i64 [M], host
  mesh_index: t.Tensor                     # i64 [M], host: the object is mesh mesh_index of its scene
  class_index: t.Tensor                    # i64 [M], host: ex.mesh_labels of the object
  gt_voxels: t.Tensor                      # i64 [M], host: 0 for a mesh that leaves no voxel (still a false negative)
  matched: t.Tensor                        # bool [M], host
  matched_iou: t.Tensor                    # f64 [M], host: the IoU with the matched predicted component, 0 if none
  best_iou: t.Tensor                       # f64 [M], host: the best IoU with a predicted component of the object's class


def instance_metrics_for_batch(pmf: t.Tensor, ex, task_type, connectivity: int = 6, min_component_voxels: int = 0,
                               iou_threshold: float = 0.5, gt_instances: Optional[t.Tensor] = None,
                               **voxelization) -> InstanceRows:
  """Per-object evaluation of a batch (corenet_amd.voxel_overlap): per-object IoU and the counts of
  panoptic / segmentation / recognition quality.

  The predicted instances are the connected components (`connectivity`, per value) of the predicted label grid
  extract_labels(pmf, ex, task_type)[0]; the class of a component is the label it carries.  Components below
  min_component_voxels voxels are folded into the background.  The ground-truth instances are gt_instances (int32
  [B, D, H, W], mesh index + 1, 0 where no mesh is) if given, otherwise batched_example.voxelize(ex, resolution,
  voxel_content_mesh_index, **voxelization) with the keywords of batched_example.voxelize (where meshes overlap, the
  voxel belongs to the one with the highest index); the class of instance i of scene b is ex.mesh_labels[b][i - 1].  A
  predicted component matches an object iff their classes are equal and their IoU exceeds iou_threshold (>= 0.5, so
  matches are unique: match_segments).  A mesh that leaves no voxel counts as a false negative.  Touching objects of one
  class come out as one predicted component, which then matches at most one of them: that is the measurement, not an
  error.  A ground-truth label above the scene's number of meshes raises ValueError.

  Per call: one connected-components call with its statistics, one label_overlaps call, torch on the sparse table."""
  from corenet_amd import voxel_overlap as VO
  from corenet_amd.voxel_components import component_stats, connected_components
  task = _task(task_type)
  if pmf.dim() != 5 or pmf.shape[1] < 2:
    raise ValueError(f"instance_metrics_for_batch: pmf must be [B, C >= 2, D, H, W], got {tuple(pmf.shape)}")
  dev = pmf.device
  B, C = pmf.shape[:2]
  if len(ex.scene_id) != B or len(ex.mesh_labels) != B:
    raise ValueError(f"instance_metrics_for_batch: pmf has {B} elements, the batch {len(ex.scene_id)}")
  mesh_labels = [t.as_tensor(v).to(t.int64).cpu().reshape(-1) for v in ex.mesh_labels]
  if gt_instances is None:
    from corenet_amd.data import batched_example
    gt_instances = batched_example.voxelize(ex, tuple(pmf.shape[2:]), batched_example.voxel_content_mesh_index, **voxelization).grid
  gt_instances = t.as_tensor(gt_instances).to(dev)
  if tuple(gt_instances.shape) != (B,) + tuple(pmf.shape[2:]):
    raise ValueError(f"instance_metrics_for_batch: gt_instances is {tuple(gt_instances.shape)}, pmf {tuple(pmf.shape)}")
  pred = extract_labels(pmf, ex, task)[0]
  comps = connected_components(pred, connectivity, by_value=True)
  stats = component_stats(comps, pred)
  num_meshes = t.tensor([v.numel() for v in mesh_labels], dtype=t.int64)
  ov = VO.label_overlaps(comps.labels, gt_instances, comps.num_components, num_meshes.to(dev))
  if bool(ov.bad.any()):
    raise ValueError(f"instance_metrics_for_batch: gt_instances has labels outside 0 .. number of meshes ({ov.bad.tolist()} voxels)")
  K = stats.size.numel()
  comp_scene = t.repeat_interleave(t.arange(B), stats.offsets[1:] - stats.offsets[:-1], output_size=K).to(dev)
  class_a = t.zeros(K + B, dtype=t.int32, device=dev)                        # a background row in front of every scene
  class_a[t.arange(K, device=dev) + comp_scene + 1] = stats.value
  class_b = t.cat([t.cat([t.zeros(1, dtype=t.int64), v]) for v in mesh_labels]).to(dev, t.int32)
  matches = VO.match_segments(ov, class_a, class_b, iou_threshold=iou_threshold, min_voxels_a=int(min_component_voxels))
  num_classes = max([C] + [int(v.max()) + 1 for v in mesh_labels if v.numel()])
  counts = VO.panoptic_quality(matches, num_classes)
  objects = matches.valid_b.nonzero()[:, 0]                                   # scene-major, mesh order
  return InstanceRows(list(ex.scene_id), counts,
                      t.repeat_interleave(t.arange(B), num_meshes), t.cat([t.arange(int(n)) for n in num_meshes] + [t.zeros(0, dtype=t.int64)]),
                      t.cat(mesh_labels + [t.zeros(0, dtype=t.int64)]), matches.size_b[objects].cpu(),
                      (matches.partner_b[objects] > 0).cpu(), matches.iou_b[objects].cpu(), matches.best_iou_b[objects].cpu())


class InstanceResults:
  """Accumulates instance_metrics_for_batch over an evaluation run, in the manner of VisibilityResults: add_batch(pmf,
  ex) takes what pipeline.evaluate_batch returns (keyword arguments go on to instance_metrics_for_batch, e.g.
  gt_instances); summary() pools the counts over all scenes and gives, per class and overall (the classes summed): PQ,
  SQ, RQ, tp / fp / fn, the mean best_iou per ground-truth object and the number of predicted components per
  ground-truth object, (tp + fp) / (tp + fn)."""

  def __init__(self, task_type="fg_bg", connectivity: int = 6, min_component_voxels: int = 0, iou_threshold: float = 0.5,
               **voxelization):
    self.task_type = task_type
    self.connectivity = connectivity
    self.min_component_voxels = min_component_voxels
    self.iou_threshold = iou_threshold
    self.voxelization = voxelization
    self.scene_id: List[str] = []
    self.counts: List[Tuple[t.Tensor, t.Tensor, t.Tensor, t.Tensor]] = []
    self.class_index: List[t.Tensor] = []
    self.best_iou: List[t.Tensor] = []

  def add_batch(self, pmf: t.Tensor, ex, gt_instances: Optional[t.Tensor] = None) -> InstanceRows:
    rows = instance_metrics_for_batch(pmf, ex, self.task_type, connectivity=self.connectivity,
                                      min_component_voxels=self.min_component_voxels, iou_threshold=self.iou_threshold,
                                      gt_instances=gt_instances, **self.voxelization)
    self.scene_id += rows.scene_id
    self.counts.append(tuple(x.cpu() for x in rows.counts))
    self.class_index.append(rows.class_index)
    self.best_iou.append(rows.best_iou)
    return rows

  def pooled(self) -> Tuple[t.Tensor, t.Tensor, t.Tensor, t.Tensor]:
    """(tp, fp, fn i64 [num_classes], sum_iou f64 [num_classes]) summed over every scene added so far; batches with
    fewer classes are padded."""
    nc = max([c[0].shape[1] for c in self.counts] + [1])
    out = [t.zeros(nc, dtype=t.int64), t.zeros(nc, dtype=t.int64), t.zeros(nc, dtype=t.int64), t.zeros(nc, dtype=t.float64)]
    for c in self.counts:
      for acc, x in zip(out, c):
        acc[:x.shape[1]] += x.sum(0)
    return tuple(out)

  def summary(self) -> Dict:
    from corenet_amd.voxel_overlap import panoptic_scores
    tp, fp, fn, sum_iou = self.pooled()
    cls = t.cat(self.class_index) if self.class_index else t.zeros(0, dtype=t.int64)
    best = t.cat(self.best_iou) if self.best_iou else t.zeros(0, dtype=t.float64)

    def entry(tp, fp, fn, sum_iou, sel):
      pq, sq, rq = panoptic_scores(tp, fp, fn, sum_iou)
      objects = int(tp + fn)
      return {"pq": float(pq), "sq": float(sq), "rq": float(rq), "tp": int(tp), "fp": int(fp), "fn": int(fn),
              "num_objects": objects, "mean_best_iou": float(best[sel].mean()) if objects else float("nan"),
              "components_per_object": float(tp + fp) / objects if objects else float("nan")}
    present = [c for c in range(tp.numel()) if int(tp[c] + fp[c] + fn[c])]
    return {"overall": entry(tp.sum(), fp.sum(), fn.sum(), sum_iou.sum(), t.ones_like(cls, dtype=t.bool)),
            "per_class": {c: entry(tp[c], fp[c], fn[c], sum_iou[c], cls == c) for c in present}}


class TopologyRows(NamedTuple):
  """One row per (scene, class) in which prediction or ground truth has a voxel, scene-major; class 0 is the
  class-agnostic mask (any object).  Everything is on the host."""
  scene_id: List[str]                      # [R]
  scene_index: t.Tensor                    # i64 [R]
  class_index: t.Tensor                    # i64 [R]
  pred: t.Tensor                           # i64 [R, 6]: b0, b1, b2, chi, volume (voxels), exposed_faces
  gt: t.Tensor                             # i64 [R, 6]
  pred_area: t.Tensor                      # f64 [R]: Crofton area in view-space units
  gt_area: t.Tensor                        # f64 [R]


def topology_metrics_for_batch(pmf: t.Tensor, ex, task_type, connectivity: int = 26) -> TopologyRows:
  """Shape type per (scene, class) (corenet_amd.voxel_topology): the Betti numbers b0 (pieces), b1
  (handles), b2 (cavities), the Euler characteristic, the volume, the exposed faces and the Crofton surface area of the
  predicted label grid extract_labels(pmf, ex, task_type)[0] and of the ground truth [1].  Rows: the class-agnostic mask
  (class 0) of every scene, then every label for `semantic`, the scene's mesh label for `fg_bg`; rows empty on both
  sides are left out.  The area is in view-space units (voxel edge from inverse(ex.v2x_transform[b]); ValueError unless
  the voxels are cubic).  A ground-truth label outside 0 .. the number of labels raises ValueError.  The default
  connectivity is 26: thin parts digitised along a diagonal are one piece under it and many under 6.

  Per call: one configuration histogram and three connected-components passes over prediction and ground truth together."""
  from corenet_amd import voxel_topology as VT
  task = _task(task_type)
  if connectivity not in (6, 26):
    raise ValueError(f"topology_metrics_for_batch: connectivity must be 6 or 26, got {connectivity}")
  if pmf.dim() != 5 or pmf.shape[1] < 2:
    raise ValueError(f"topology_metrics_for_batch: pmf must be [B, C >= 2, D, H, W], got {tuple(pmf.shape)}")
  dev = pmf.device
  B, C = pmf.shape[:2]
  if len(ex.scene_id) != B:
    raise ValueError(f"topology_metrics_for_batch: pmf has {B} elements, the batch {len(ex.scene_id)}")
  if tuple(ex.grid.shape) != (B,) + tuple(pmf.shape[2:]):
    raise ValueError(f"topology_metrics_for_batch: ex.grid is {tuple(ex.grid.shape)}, pmf {tuple(pmf.shape)}")
  sizes = _voxel_sizes(ex.v2x_transform).to(t.float64)
  if task == "fg_bg":
    if C != 2:
      raise ValueError(f"topology_metrics_for_batch: fg_bg expects 2 classes, pmf has {C}")
    scene_label = t.cat([t.as_tensor(v).reshape(-1) for v in ex.mesh_labels]).to(t.int64).cpu()
    if scene_label.numel() != B or bool((scene_label < 0).any()):
      raise ValueError(f"topology_metrics_for_batch: fg_bg expects one non-negative mesh label per scene, got {scene_label.tolist()}")
    L = int(scene_label.max()) if B else 0
  else:
    L = C - 1
  pred, gt = extract_labels(pmf, ex, task)
  both = t.cat([pred, t.as_tensor(gt).to(dev, t.int32)])
  grid, L, mask = VT._prepare(both, L, "topology_metrics_for_batch")
  betti, hist = VT._betti(grid, L, mask, connectivity, VT._CHUNK_BYTES)
  if bool(hist.bad[B:].any()):
    raise ValueError(f"topology_metrics_for_batch: ex.grid has labels outside 0 .. {L} ({hist.bad[B:].tolist()} voxels)")
  table = hist.table.cpu()
  ints = t.stack([x.cpu() for x in betti] + [VT.volume(table), VT.exposed_faces(table)], -1)             # [2B, L + 1, 6]
  area = VT.crofton_area(table, t.cat([sizes, sizes])[:, None])                                          # [2B, L + 1]
  keep = (ints[:B, :, 4] > 0) | (ints[B:, :, 4] > 0)
  if task == "fg_bg":
    own = t.zeros_like(keep)
    own[:, 0] = True
    own[t.arange(B), scene_label] = True
    keep &= own
  scene, cls = keep.nonzero(as_tuple=True)
  return TopologyRows([ex.scene_id[int(b)] for b in scene], scene, cls, ints[:B][scene, cls], ints[B:][scene, cls],
                      area[:B][scene, cls], area[B:][scene, cls])


class TopologyResults:
  """Accumulates topology_metrics_for_batch over an evaluation run, in the manner of InstanceResults: add_batch(pmf, ex)
  takes what pipeline.evaluate_batch returns; summary() gives, for the class-agnostic rows (`any_object`), per class and
  `overall` (the rows of all classes together): the mean |b0 - b0'|, |b1 - b1'|, |b2 - b2'| between prediction and ground
  truth, the share of rows with all three equal (`topology_correct`), the pooled volume and area ratios, predicted over
  ground truth (NaN where the ground truth has none), and the number of rows."""

  def __init__(self, task_type="fg_bg", connectivity: int = 26):
    self.task_type = task_type
    self.connectivity = connectivity
    self.batches: List[TopologyRows] = []

  def add_batch(self, pmf: t.Tensor, ex) -> TopologyRows:
    rows = topology_metrics_for_batch(pmf, ex, self.task_type, connectivity=self.connectivity)
    self.batches.append(rows)
    return rows

  def rows(self) -> TopologyRows:
    """Every row added so far; scene_index counts within its batch."""
    if not self.batches:
      z, f = t.zeros(0, dtype=t.int64), t.zeros(0, dtype=t.float64)
      return TopologyRows([], z, z, t.zeros((0, 6), dtype=t.int64), t.zeros((0, 6), dtype=t.int64), f, f)
    return TopologyRows(sum((b.scene_id for b in self.batches), []), *(t.cat(x) for x in list(zip(*self.batches))[1:]))

  def summary(self) -> Dict:
    r = self.rows()
    delta = (r.pred[:, :3] - r.gt[:, :3]).abs()

    def entry(sel):
      n = int(sel.sum())
      nan = float("nan")
      d = delta[sel].to(t.float64)
      gt_volume, gt_area = float(r.gt[sel, 4].sum()), float(r.gt_area[sel].sum())
      return {"mean_abs_delta_b0": float(d[:, 0].mean()) if n else nan, "mean_abs_delta_b1": float(d[:, 1].mean()) if n else nan,
              "mean_abs_delta_b2": float(d[:, 2].mean()) if n else nan,
              "topology_correct": float((d.sum(1) == 0).to(t.float64).mean()) if n else nan,
              "volume_ratio": float(r.pred[sel, 4].sum()) / gt_volume if gt_volume else nan,
              "area_ratio": float(r.pred_area[sel].sum()) / gt_area if gt_area else nan, "num_rows": n}
    cls = r.class_index
    return {"connectivity": self.connectivity, "any_object": entry(cls == 0), "overall": entry(cls > 0),
            "per_class": {int(c): entry(cls == c) for c in sorted(set(cls[cls > 0].tolist()))}}


GLOBAL_CLASS_NAME = "__global__"
METRIC_NAMES = ("iou", "precision", "recall")


class MetricsTable(NamedTuple):
  """The reference's metrics data frame (evaluation_results.py:188-210): one row per metric, one column per class and a
  last column `__global__` with the class-agnostic foreground / background result."""
  rows: Tuple[str, ...]        # ("iou", "precision", "recall")
  columns: Tuple[str, ...]     # class names + ("__global__",)
  values: t.Tensor             # f64 [3, K + 1] on the host; NaN: no true positive

  def row(self, name: str) -> t.Tensor:
    return self.values[self.rows.index(name)]

  def to_csv(self) -> str:
    """Byte for byte what pandas' DataFrame.to_csv gives for the reference's frame: an empty first header cell, floats in
    their shortest round-trip form (repr), NaN as an empty field, minimal quoting, "\n" line ends."""
    out = io.StringIO()
    w = csv.writer(out, lineterminator="\n", quoting=csv.QUOTE_MINIMAL)
    w.writerow(("",) + tuple(self.columns))
    for name, vals in zip(self.rows, self.values.tolist()):
      w.writerow([name] + ["" if v != v else repr(float(v)) for v in vals])
    return out.getvalue()


def compute_voxel_metrics(cm: t.Tensor, classes: Sequence[str]) -> MetricsTable:
  """The metrics table of a confusion matrix [K, K] (ground truth, predicted) over `classes` (K names)
  (evaluation_results.py:188-210)."""
  classes = [str(c) for c in classes]
  cm = t.as_tensor(cm).detach().cpu()
  if cm.dim() != 2 or cm.shape[0] != cm.shape[1] or cm.shape[0] != len(classes):
    raise ValueError(f"compute_voxel_metrics: matrix {tuple(cm.shape)} for {len(classes)} classes")
  per_class = voxel_metrics.compute_voxel_metrics(voxel_metrics.compute_tfpn(cm))
  fg = voxel_metrics.compute_voxel_metrics(voxel_metrics.compute_tfpn_fg(cm))
  values = t.stack([t.cat([getattr(per_class, k), getattr(fg, k).reshape(1)]) for k in METRIC_NAMES])
  return MetricsTable(METRIC_NAMES, tuple(classes) + (GLOBAL_CLASS_NAME,), values)


def scene_classes_of(ex) -> t.Tensor:
  """int32 [B] on the host: the single mesh label of every scene of a batch, the factor fg_bg evaluation scales
  prediction and ground truth with (evaluation_results.py:42-54).  A scene with another number of meshes has no such
  label: ValueError."""
  out = []
  for scene_id, v in zip(ex.scene_id, ex.mesh_labels):
    v = t.as_tensor(v).reshape(-1)
    if v.numel() != 1:
      raise ValueError(f"fg_bg evaluation needs exactly one mesh per scene; scene {scene_id!r} has {v.numel()}")
    out.append(int(v[0]))
  return t.tensor(out, dtype=t.int32)


class QuantitativeResults:
  """Accumulates the confusion matrix of an evaluation run over the dataset's classes and reduces it to the reference's
  table (evaluation_results.py:241-271, without TensorBoard).  The matrix (int64 [K, K]) and the count of voxels whose
  label or prediction fell outside [0, K) live on the device of the first batch; nothing is read back before
  compute_metrics."""

  def __init__(self, classes: Sequence[str], task_type="fg_bg"):
    self.classes = [str(c) for c in classes]
    self.task = _task(task_type)
    self.confusion_matrix: Optional[t.Tensor] = None
    self.bad: Optional[t.Tensor] = None
    self.metrics: Optional[MetricsTable] = None

  def _batch_args(self, ex, dev):
    K = len(self.classes)
    if self.confusion_matrix is None:
      self.confusion_matrix = t.zeros((K, K), dtype=t.int64, device=dev)
      self.bad = t.zeros((1,), dtype=t.int32, device=dev)
    scene = scene_classes_of(ex).to(dev) if self.task == "fg_bg" else None
    return ex.grid.to(dev, t.int32).contiguous(), K, scene

  def add_batch(self, pmf: t.Tensor, ex) -> t.Tensor:
    """Counts a batch from its pmf f32 [B, C, D, H, W] (the reference's contract); returns the predicted labels."""
    gt, K, scene = self._batch_args(ex, pmf.device)
    return voxel_metrics.label_confusion(pmf, gt, K, scene, cm=self.confusion_matrix, bad=self.bad)[0]

  def add_batch_streaming(self, inference, ex) -> t.Tensor:
    """Counts a batch without a pmf: `inference.predict_labels` (SuperResolutionInference) at the resolution of ex.grid,
    the matrix accumulated pass by pass; returns the predicted labels int32 [B, mD, mH, mW]."""
    gt, K, scene = self._batch_args(ex, ex.grid.device)
    with t.no_grad():
      return inference.predict_labels(ex.input_image, ex.camera_transform, ex.v2x_transform, ex.grid_sampling_offset,
                                      tuple(gt.shape[1:]), gt=gt, num_classes=K, scene_classes=scene,
                                      cm=self.confusion_matrix, bad=self.bad)

  def compute_metrics(self, dst: int = 0, group=None) -> Optional[MetricsTable]:
    """Sums the matrix over the ranks onto rank dst (evaluation_results.py:255-260), then reads this rank's out-of-range
    count -- the run's first device -> host synchronisation -- and raises ValueError when it is not 0.  Returns the table
    on rank dst (None elsewhere)."""
    if self.confusion_matrix is None:
      raise ValueError("QuantitativeResults.compute_metrics: no batch was added")
    dist_util.reduce_confusion_matrix(self.confusion_matrix, dst, group)
    bad = int(self.bad.item())
    if bad:
      raise ValueError(f"{bad} voxels had a label or a prediction outside the {len(self.classes)} classes of the dataset")
    if dist_util.dist.is_initialized() and dist_util.dist.get_rank(group) != dst:
      return None                                   # the sum lives on rank dst alone
    self.metrics = compute_voxel_metrics(self.confusion_matrix, self.classes)
    return self.metrics

  def get_mean_iou(self) -> float:
    """Mean IoU over the non-void classes, NaNs skipped, NaN when every class is NaN (evaluation_results.py:262-266)."""
    iou = self.metrics.row("iou")[1:-1]
    keep = ~t.isnan(iou)
    return float(iou[keep].mean()) if bool(keep.any()) else float("nan")

  def write_csv(self, path: str):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w", newline="") as f:
      f.write(self.metrics.to_csv())


def score_metrics_for_batch(pmf: t.Tensor, ex, task_type, nbins: int = 20, num_classes: Optional[int] = None, out=None):
  """Score-level evaluation of a batch (corenet_amd.score_metrics): the ScoreHistogram of pmf f32
  [B, C, D, H, W] against ex.grid, from which the reliability diagram, the calibration errors, the Brier score, the
  threshold curve and average precision follow.  With num_classes (the dataset's class count) an fg_bg batch is scored
  per dataset class, the scene's mesh label scaling label and row as in QuantitativeResults; without it the rows are the
  pmf's own channels.  Accumulates into `out` when given; nothing is read back."""
  from corenet_amd import score_metrics
  task = _task(task_type)
  dev = pmf.device
  scene = scene_classes_of(ex).to(dev) if task == "fg_bg" and num_classes is not None else None
  return score_metrics.score_histogram(pmf, ex.grid.to(dev, t.int32).contiguous(), num_classes, scene, nbins=nbins, out=out)


SCORE_SUMMARY_NAMES = ("ece", "mce", "brier", "ap", "best_threshold", "best_iou", "iou_at_0.5")


class ScoreResults:
  """Accumulates the score histogram of an evaluation run over the dataset's classes (corenet_amd.score_metrics, DESIGN
  section 22) beside QuantitativeResults' confusion matrix: from a pmf, or streamed pass by pass at the resolution of the
  ground truth.  The tables live on the device of the first batch; nothing is read back before compute_metrics."""

  def __init__(self, classes: Sequence[str], task_type="fg_bg", nbins: int = 20):
    from corenet_amd import score_metrics
    self.classes = [str(c) for c in classes]
    self.task = _task(task_type)
    self.nbins = int(nbins)
    if not 1 <= self.nbins <= score_metrics.MAX_NBINS or (len(self.classes) + 1) * self.nbins > score_metrics.MAX_ENTRIES:
      raise ValueError(f"ScoreResults: {self.nbins} bins for {len(self.classes)} classes exceed the table of "
                       f"{score_metrics.MAX_ENTRIES} entries (or the limit of {score_metrics.MAX_NBINS} bins)")
    self.histogram = None
    self.reduced = False

  def ensure_tables(self, dev):
    from corenet_amd import score_metrics
    if self.histogram is None:
      self.histogram = score_metrics.empty_histogram(len(self.classes), self.nbins, dev)

  def _batch_args(self, ex, dev):
    self.ensure_tables(dev)
    scene = scene_classes_of(ex).to(dev) if self.task == "fg_bg" else None
    return ex.grid.to(dev, t.int32).contiguous(), scene

  def add_batch(self, pmf: t.Tensor, ex):
    """Counts a batch from its pmf f32 [B, C, D, H, W]; returns the run's histogram."""
    from corenet_amd import score_metrics
    gt, scene = self._batch_args(ex, pmf.device)
    return score_metrics.score_histogram(pmf, gt, len(self.classes), scene, nbins=self.nbins, out=self.histogram)

  def add_batch_streaming(self, inference, ex):
    """Counts a batch without a pmf: `inference.predict_score_histogram` (SuperResolutionInference) at the resolution of
    ex.grid, the tables accumulated pass by pass; returns the run's histogram."""
    gt, scene = self._batch_args(ex, ex.grid.device)
    with t.no_grad():
      return inference.predict_score_histogram(ex.input_image, ex.camera_transform, ex.v2x_transform, ex.grid_sampling_offset,
                                               tuple(gt.shape[1:]), gt, num_classes=len(self.classes), scene_classes=scene,
                                               nbins=self.nbins, out=self.histogram)

  def compute_metrics(self, dst: int = 0, group=None):
    """Sums the tables over the ranks onto rank dst the way the confusion matrix is summed, then reads this rank's count
    of rejected voxels and raises ValueError when it is not 0.  Returns the histogram on rank dst (None elsewhere)."""
    if self.histogram is None:
      raise ValueError("ScoreResults.compute_metrics: no batch was added")
    h = self.histogram
    dist_util.reduce_confusion_matrix(h.table, dst, group)
    dist_util.reduce_confusion_matrix(h.sq, dst, group)
    bad = int(h.bad.item())
    if bad:
      raise ValueError(f"{bad} voxels had a label outside the {len(self.classes)} classes of the dataset, a scene class that "
                       "does not fit them, or a score that is NaN or outside [0, 1]")
    self.reduced = True
    if dist_util.dist.is_initialized() and dist_util.dist.get_rank(group) != dst:
      return None
    return h

  def _columns(self) -> Tuple[str, ...]:
    return tuple(self.classes) + (GLOBAL_CLASS_NAME,)

  def summary(self) -> Dict:
    """Per class and for the `__global__` row (the class-agnostic foreground): expected and maximum calibration error,
    Brier score, average precision, the first threshold of maximum IoU with that IoU, and the IoU at threshold 0.5
    (the first threshold j / nbins >= 0.5).  NaN where a row has no voxel (or no positive, where positives are needed)."""
    from corenet_amd import score_metrics as SM
    h = self.histogram
    if h is None:
      raise ValueError("ScoreResults.summary: no batch was added")
    thr, best = SM.best_threshold(h)
    half = (self.nbins + 1) // 2
    cols = (SM.expected_calibration_error(h), SM.maximum_calibration_error(h), SM.brier_score(h), SM.average_precision(h),
            thr, best, SM.threshold_curve(h).iou[:, half])
    values = t.stack(cols, 1).cpu().tolist()
    return {name: dict(zip(SCORE_SUMMARY_NAMES, row)) for name, row in zip(self._columns(), values)}

  def write_csv(self, path: str):
    """One line per (class, threshold) with the curve -- kind `threshold`: value j / nbins, tp, fp, fn, iou, precision,
    recall -- and one per (class, bin) with the reliability diagram -- kind `bin`: value the bin's lower edge, count,
    confidence, frequency.  NaN as an empty field, floats in their shortest round-trip form."""
    from corenet_amd import score_metrics as SM
    h = self.histogram
    c, curve, rel = SM.threshold_counts(h), SM.threshold_curve(h), SM.reliability(h)
    tp, fp, fn = (x.cpu().tolist() for x in c)
    iou, prec, rec = (x.cpu().tolist() for x in (curve.iou, curve.precision, curve.recall))
    cnt, conf, freq = (x.cpu().tolist() for x in rel)
    cell = lambda v: "" if v != v else repr(float(v))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w", newline="") as f:
      w = csv.writer(f, lineterminator="\n", quoting=csv.QUOTE_MINIMAL)
      w.writerow(("class", "kind", "value", "tp", "fp", "fn", "iou", "precision", "recall", "count", "confidence", "frequency"))
      for r, name in enumerate(self._columns()):
        for j in range(self.nbins + 1):
          w.writerow([name, "threshold", repr(j / self.nbins), tp[r][j], fp[r][j], fn[r][j], cell(iou[r][j]), cell(prec[r][j]),
                      cell(rec[r][j]), "", "", ""])
        for j in range(self.nbins):
          w.writerow([name, "bin", repr(j / self.nbins), "", "", "", "", "", "", int(cnt[r][j]), cell(conf[r][j]),
                      cell(freq[r][j])])
