"""Scenes shared by the renderer tests: the two scenes of the reference's renderer tests (scene_renderer_test.py,
voxel_renderer_test.py), whose GL images are tests/golden/render/*.png, and a synthetic BatchedExample."""
import math
import os

import numpy as np
import PIL.Image
import torch as t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_RENDER = os.path.join(ROOT, "tests", "golden", "render")

CUBE_V = np.array([[0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1], [0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
CUBE_I = np.array([0, 1, 2, 2, 3, 0, 1, 5, 6, 6, 2, 1, 7, 6, 5, 5, 4, 7, 4, 0, 3, 3, 7, 4, 4, 5, 1, 1, 0, 4, 3, 2, 6, 6,
                   7, 3])


def cube_mesh() -> t.Tensor:
  return t.from_numpy(CUBE_V[CUBE_I].reshape(-1, 3, 3))


def golden(name: str) -> np.ndarray:
  return np.array(PIL.Image.open(os.path.join(GOLDEN_RENDER, f"expected_image_{name}.png")))[..., :3]


def mesh_scene(device="cpu") -> t.Tensor:
  from corenet_amd.geometry import transformations as T
  from corenet_amd.visualization import render as R
  cam = t.matmul(T.perspective_rh(70 * math.pi / 180, 1, 0.1, 10.0), T.look_at_rh((-1.2, -1.5, -1), (0, 0, 0), (0, 1, 0)))
  return R.render_scene(cube_mesh().to(device), cam, (256, 256), material_ids=t.zeros(12, dtype=t.int32),
                        diffuse_coefficients=((1.0, 0.0, 0.0),), ambient_coefficients=((0.0, 0.0, 0.0),),
                        ambient_light_color=(0.0, 0.0, 0.0), light_position=(-1.2, -1.5, -1))


VOXEL_GRID = [[[1, 0, 1], [0, 0, 0], [1, 0, 1]], [[0, 0, 0], [0, 1, 0], [0, 0, 0]], [[0, 1, 0], [1, 1, 1], [0, 1, 0]]]


def voxel_scene(device="cpu") -> t.Tensor:
  from corenet_amd.geometry import transformations as T
  from corenet_amd.visualization import render as R
  g = t.tensor(VOXEL_GRID, dtype=t.int32).to(device)
  la = T.look_at_rh((-1.2 + 0.5, -1.5 + 0.5, -0.5 + 0.5), (0.5, 0.5, 0.5), (0, 1, 0))
  mv = t.matmul(T.perspective_rh(70 * math.pi / 180, 1, 0.1, 10.0), la)
  return R.render_voxel_grid(g, mv, (256, 256), T.scale((1.0 / 3,) * 3), ((-1, 0, 0), (1.0, 0, 0)),
                             light_position=(-1.2 + 0.5, -1.5 + 0.5, -1 + 0.5), ambient_light_color=(0.0, 0.0, 0.0))


def golden_stats(image: np.ndarray, name: str):
  """(L1 over RGB, differing pixels, covered pixels of image, covered pixels of the golden image)."""
  exp = golden(name)
  d = np.abs(image.astype(np.int64) - exp.astype(np.int64))
  return int(d.sum()), int((d.sum(-1) > 0).sum()), int(image.any(-1).sum()), int(exp.any(-1).sum())


def synthetic_example(B=2, R=32, seed=0):
  """(pmf f32 [B, 2, R, R, R], BatchedExample) on the host: a sphere of probabilities, a voxel ball as ground truth,
  a scaled cube per element as ground-truth mesh, random input images."""
  from corenet_amd.data.batched_example import BatchedExample
  from corenet_amd.geometry import transformations as T
  from corenet_amd.visualization import camera_util
  g = t.Generator().manual_seed(seed)
  verts = [cube_mesh() * 0.4 + 0.3 + 0.05 * b for b in range(B)]
  z = t.linspace(-1, 1, R)
  rr = (z[:, None, None] ** 2 + z[None, :, None] ** 2 + z[None, None, :] ** 2).sqrt()
  p1 = (1 - rr).clamp(0, 1)[None].expand(B, R, R, R)
  pmf = t.stack([1 - p1, p1], 1).contiguous()
  grid = (rr < 0.6).to(t.int32)[None].expand(B, R, R, R).contiguous()
  cam = t.matmul(camera_util.perspective_projection(), T.look_at_lh((0.5, 0.5, -1.5), (0.5, 0.5, 0.5), (0, 1, 0)))
  ex = BatchedExample(
      vertices=t.cat(verts), view_transform=t.eye(4).expand(B, 4, 4).clone(), camera_transform=cam.expand(B, 4, 4).clone(),
      mesh_num_tri=[t.tensor([12], dtype=t.int32) for _ in range(B)],
      mesh_labels=[t.tensor([1 + b], dtype=t.int32) for b in range(B)],
      input_image=t.randint(0, 256, (B, 3, 64, 48), generator=g, dtype=t.uint8), scene_id=[f"x/s{b}" for b in range(B)],
      grid_sampling_offset=t.full((B, 3), 0.5), v2x_transform=T.scale([float(R)] * 3).expand(B, 4, 4).clone(), grid=grid)
  return pmf, ex


QUALITATIVE_GOLDEN = os.path.join(GOLDEN_RENDER, "qualitative_n2_s0.png")


def fixture_eval_batch(nc=4):
  """(pmf f32 [2, nc, 128, 128, 128] on the GPU, voxelized BatchedExample) of the two fixture scenes (semantic task): a
  pmf near the ground truth, softmax(2 * one-hot + 0.3 * noise), the noise drawn on the host from a fixed seed."""
  from corenet_amd import pipeline
  from corenet_amd.data import batched_example as BE, dataset as D
  root = os.path.join(ROOT, "tests", "golden", "n2_dataset")
  ds = D.CoReNetDatasetImpl(os.path.join(root, "dataset.json"), os.path.join(root, "meshes"))
  ex = pipeline.voxelize_batch(BE.batch([ds[0], ds[1]]), "semantic")
  noise = t.randn((2, nc) + tuple(ex.grid.shape[1:]), generator=t.Generator().manual_seed(7)) * 0.3
  onehot = t.nn.functional.one_hot(ex.grid.to(t.int64).clamp(0, nc - 1), nc).permute(0, 4, 1, 2, 3).float()
  return (noise.to(ex.grid.device) + 2 * onehot).softmax(1), ex


def write_qualitative(pmf, ex, out_dir) -> str:
  """QualitativeResults for the batch's first scene -> the path of the PNG it wrote."""
  from corenet_amd import evaluation_results as ER

  class First:
    def __len__(self):
      return 1

    def __getitem__(self, i):
      return type("El", (), {"scene_id": ex.scene_id[0]})()

  ER.QualitativeResults(First(), out_dir, "semantic", num_qualitative_results=1).add_batch(pmf, ex)
  return os.path.join(out_dir, "img_%s.png" % ex.scene_id[0].replace("/", "_"))
