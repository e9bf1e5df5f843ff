"""The training / evaluation hot loop around the model (`corenet.pipeline`, pipeline.py:100-242,311-325):
data loader, ground-truth voxelization settings, one training step from a list of dataset elements, and the evaluation
run over a dataset (`EvalPipeline.run_eval`, pipeline.py:292-343).
Configuration objects, TensorBoard, checkpoint management, `DatasetManager` and the progress UI of the reference pipeline
are out of scope; their values arrive here as plain arguments."""
from __future__ import annotations

import os
from typing import List, Optional, Tuple

import torch as t

from corenet_amd import distributed as dist_util
from corenet_amd.data import batched_example, dataset as dataset_lib

LOSS_OF_TASK = {"fg_bg": "iou_fgbg", "semantic": "xent_times_iou_agnostic"}      # pipeline.py:150-154


def create_distributed_loader(dataset, batch_size: int, global_rank: int, global_world_size: int,
                              num_data_workers: int = 0, prefetch_factor: Optional[int] = None,
                              pad_data: bool = False) -> t.utils.data.DataLoader:
  """pipeline.py:100-119: the loader hands over *lists* of elements (`collate_fn=lambda v: v`); `batch`
  runs in the training process, which is where this build sends the geometry to the GPU."""
  sampler = dist_util.DistributedSampler(dataset, global_rank=global_rank, global_world_size=global_world_size,
                                         pad_data=pad_data)
  ctx = t.multiprocessing.get_context("fork") if num_data_workers > 0 else None
  return t.utils.data.DataLoader(
      dataset, batch_size=batch_size, num_workers=num_data_workers, pin_memory=True, collate_fn=_identity,
      sampler=sampler, multiprocessing_context=ctx, drop_last=False,
      prefetch_factor=prefetch_factor if num_data_workers > 0 else None)


def _identity(v):
  return v


def voxelize_batch(b: batched_example.BatchedExample, task_type: str = "fg_bg",
                   resolution: Tuple[int, int, int] = (128, 128, 128), sub_grid_sampling: bool = False,
                   voxelization_image_resolution_multiplier=8, conservative_rasterization: bool = False,
                   voxelization_projection_depth_multiplier: int = 1) -> batched_example.BatchedExample:
  """pipeline.py:122-142 with the fields of `VoxelizationConfig` as arguments (defaults: configs/models/h7.json5)."""
  voxel_content_fn = {"semantic": batched_example.VoxelContentSemanticLabel(b.mesh_labels),
                      "fg_bg": batched_example.voxel_content_1}[task_type]
  return batched_example.voxelize(
      b, resolution=tuple(resolution), voxel_content_fn=voxel_content_fn, sub_grid_sampling=sub_grid_sampling,
      image_resolution_multiplier=voxelization_image_resolution_multiplier,
      conservative_rasterization=conservative_rasterization,
      projection_depth_multiplier=voxelization_projection_depth_multiplier)


def process_batch(model, batch: List[dataset_lib.DatasetElement], task_type: str = "fg_bg", lr: float = 4e-4,
                  adam_eps: float = 1e-4, world_size: int = 1, all_reduce=None, **voxelization) -> t.Tensor:
  """One training step from dataset elements (TrainPipeline._process_batch, pipeline.py:215-242): batch ->
  ground-truth grid -> `v2s = camera @ inverse(v2x)` -> forward, loss, backward, gradient exchange, Adam
  (`CoreNet.train_step`).  Returns the loss as a device tensor (the reference syncs on it every step)."""
  if world_size > 1 and getattr(all_reduce, "engine", None) is not model.engine:
    # DistributedDataParallel(broadcast_buffers=True) semantics (pipeline.py:199): every forward starts from rank
    # 0's BatchRenorm running statistics, which feed the r / d clamps (batch_renorm.py:46-49).  An exchange that was
    # attached to this model (`GradientSync(world).attach(model.engine)`) delivers exactly that on the first gradient
    # bucket of the previous step, without a collective of its own: the blocking broadcast in front of the step is only
    # for exchange objects that do not
    dist_util.broadcast_buffers(model.engine.store)
  ex = batched_example.batch(batch, device=model.engine.device)
  ex = voxelize_batch(ex, task_type, **voxelization)
  # v2s = camera @ inverse(v2x) (pipeline.py:219-221).  v2x is scale(m, m, m) built from the host-side resolution
  # (batched_example.voxelize), so its inverse is taken on the host copy of the same 4x4 and uploaded: no
  # device -> host read-back inside the step
  m = float(max(voxelization.get("resolution", (128, 128, 128))))
  inv_v2x = t.diag(t.tensor([m, m, m, 1.0])).inverse().to(ex.camera_transform.device, non_blocking=True)
  v2s = ex.camera_transform @ inv_v2x
  return model.train_step(ex.input_image, v2s, ex.grid_sampling_offset, ex.grid, LOSS_OF_TASK[task_type],
                          lr=lr, adam_eps=adam_eps, world_size=world_size, all_reduce=all_reduce)


def evaluate_batch(inference_fn, batch: List[dataset_lib.DatasetElement], task_type: str = "fg_bg", device="cuda",
                   **voxelization):
  """The body of EvalPipeline.run_eval's loop (pipeline.py:311-320): returns (pmf, voxelized batch)."""
  ex = batched_example.batch(batch, device=device)
  ex = voxelize_batch(ex, task_type, **voxelization)
  resolution = tuple(ex.grid.shape[1:])
  with t.no_grad():
    pmf = inference_fn(ex.input_image, ex.camera_transform, ex.v2x_transform, ex.grid_sampling_offset, resolution)
  return pmf, ex


def run_eval(inference, dataset, output_dir: str, task_type: str, batch_size: int, global_rank: int = 0,
             global_world_size: int = 1, resolution: Tuple[int, int, int] = (128, 128, 128), qualitative=None,
             num_data_workers: int = 0, device="cuda", scores=None, **voxelization) -> Optional[float]:
  """One evaluation run over this rank's share of `dataset` (EvalPipeline.run_eval, pipeline.py:292-343): per batch the
  ground truth is voxelized at `resolution` and scored into the confusion matrix over dataset.classes; at the end the
  matrix is summed over the ranks and rank 0 writes <output_dir>/voxel_metrics.csv and returns the mean IoU over the
  non-void classes (the other ranks return None).

  inference: called as inference(image, camera_transform, v2x_transform, grid_offsets, resolution) -> pmf, like the
  reference's InferenceFn.  When it also has `predict_labels` (SuperResolutionInference over a CoreNet) the batch is
  scored without a pmf, pass by pass (evaluation_results.QuantitativeResults.add_batch_streaming); the pmf is then
  computed only for the batches a given `qualitative` (evaluation_results.QualitativeResults) wants to draw.  Such a
  batch runs the network twice, encoder and all m^3 decoder passes: once for the pmf to draw and once for the labels.
  device: where the batches and the confusion matrix are put, as in evaluate_batch.
  scores: an evaluation_results.ScoreResults to feed alongside the confusion matrix (score-level evaluation, DESIGN
  section 22): streamed pass by pass when the inference streams (`predict_score_histogram`), from the pmf otherwise.  Its
  tables are summed over the ranks at the end and rank 0 writes <output_dir>/score_metrics.csv.
  voxelization: the keyword arguments of voxelize_batch other than task_type and resolution."""
  from corenet_amd import evaluation_results as results_lib
  loader = create_distributed_loader(dataset, batch_size, global_rank, global_world_size,
                                     num_data_workers=num_data_workers, pad_data=False)
  quantitative = results_lib.QuantitativeResults(dataset.classes, task_type)
  resolution = tuple(int(v) for v in resolution)
  streaming = hasattr(inference, "predict_labels")
  for batch in loader:
    ex = batched_example.batch(batch, device=device)
    ex = voxelize_batch(ex, task_type, resolution=resolution, **voxelization)
    draw = qualitative is not None and qualitative.wants(ex)
    pmf = None
    if draw or not streaming:
      with t.no_grad():
        pmf = inference(ex.input_image, ex.camera_transform, ex.v2x_transform, ex.grid_sampling_offset, resolution)
    if streaming:
      quantitative.add_batch_streaming(inference, ex)
    else:
      quantitative.add_batch(pmf, ex)
    if draw:
      qualitative.add_batch(pmf, ex)
    if scores is not None:
      if streaming and hasattr(inference, "predict_score_histogram"):
        scores.add_batch_streaming(inference, ex)
      else:
        if pmf is None:
          with t.no_grad():
            pmf = inference(ex.input_image, ex.camera_transform, ex.v2x_transform, ex.grid_sampling_offset, resolution)
        scores.add_batch(pmf, ex)
  if quantitative.confusion_matrix is None:           # a rank without a batch still takes part in the sum
    K = len(quantitative.classes)
    quantitative.confusion_matrix = t.zeros((K, K), dtype=t.int64, device=device)
    quantitative.bad = t.zeros((1,), dtype=t.int32, device=device)
  quantitative.compute_metrics()
  if scores is not None:
    if scores.histogram is None:                      # a rank without a batch still takes part in the sum
      scores.ensure_tables(device)
    scores.compute_metrics()
  if global_rank != 0:
    return None
  quantitative.write_csv(os.path.join(output_dir, "voxel_metrics.csv"))
  if scores is not None:
    scores.write_csv(os.path.join(output_dir, "score_metrics.csv"))
  return quantitative.get_mean_iou()
