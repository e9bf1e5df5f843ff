"""Geometry-buffer checks shared by test_render_geometry_cpu.py / _gpu.py and test_reprojection_cpu.py / _gpu.py.

Everything here is float64 numpy written from the contract of render.render_geometry alone; it shares no code with the
product and uses no oracle.

  * restate(): coverage, winner, barycentrics, z_ndc and clip w per pixel of a triangle list, and which pixels are
    DECIDED: in float64 every edge of the nearest and of the second nearest surviving fragment lies farther than
    EDGE_EPS = 1e-3 pixel from the pixel centre, and the z_ndc gap between those two fragments exceeds Z_EPS = 1e-5
    (a z_ndc within Z_EPS of the [-1, 1] limits counts as undecided too).  Undecided pixels are left out of the value
    comparisons; MAX_UNDECIDED caps them at 5 % of the covered pixels of every image of every case.
  * ray_cast_labels(): a brute-force ray caster of a tiny label grid: per pixel centre the eye ray, its nearest entry
    into a drawn voxel cube (slab test), the label and the clip w of the entry point.  No triangles, no bins.
  * cases(): the triangle scenes of the id-colour, restatement and output tests.

Tolerances of the float32 outputs against float64 (TOL): 8 times the largest deviation of the host twin from restate()
over cases(), measured on the host; the kernel is bit-identical to the twin, so the margin only guards a changed scene.
  measured: barycentrics 3.41e-5, depth 3.94e-6 (depths up to 5.2), z_ndc 7.85e-6
  bounds:   barycentrics 2.7e-4,  depth 3.2e-5,                      z_ndc 6.3e-5
The cameras of the scenes go through fixed(), so every machine draws bit-identical inputs: whether a pixel is decided, and
by how much, is then a property of the scene and not of the last bit of a tan or a sqrt of the machine that built it."""
import signal

import numpy as np
import torch as t

EDGE_EPS = 1e-3
Z_EPS = 1e-5
MAX_UNDECIDED = 0.05
TOL = {"barycentrics": 2.7e-4, "depth": 3.2e-5, "z_ndc": 6.3e-5}


class limit:
  """Wall-clock limit of one GPU step (SIGALRM); a step that overruns fails its test instead of hanging the run."""

  def __init__(self, seconds: int):
    self.seconds = seconds

  def __enter__(self):
    def boom(*_):
      raise TimeoutError(f"GPU step exceeded {self.seconds} s")
    self.prev = signal.signal(signal.SIGALRM, boom)
    signal.alarm(self.seconds)

  def __exit__(self, *exc):
    signal.alarm(0)
    signal.signal(signal.SIGALRM, self.prev)
    return False


def gpu_step(fn, seconds=60):
  with limit(seconds):
    out = fn()
    t.cuda.synchronize()
  return out


# ---------------------------------------------------------------- the float64 restatement
def _fragments(tri, vp, H, W, cull):
  """Per (triangle, pixel): survives bool, z_ndc, b [.., 3], w, edge distance in pixels (min over the three edges)."""
  T = tri.shape[0]
  clip = np.concatenate([tri, np.ones((T, 3, 1))], -1) @ vp.T                   # [T, 3, 4]
  w = clip[..., 3]
  X = (clip[..., 0] + w) * (W / 2.0)
  Y = (clip[..., 1] + w) * (H / 2.0)
  V = np.stack([X, Y, w], -1)                                                   # [T, 3, 3] window-scaled vertices
  edges = np.stack([np.cross(V[:, 1], V[:, 2]), np.cross(V[:, 2], V[:, 0]), np.cross(V[:, 0], V[:, 1])], 1)
  det = (edges[:, 0] * V[:, 0]).sum(-1)
  ok = (det != 0) & (w > 0).any(1)
  if cull:
    with np.errstate(divide="ignore", invalid="ignore"):
      ndc = clip[..., :2] / w[..., None]
      a, b = ndc[:, 1] - ndc[:, 0], ndc[:, 2] - ndc[:, 0]
      ok &= (a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]) > 0
  edges = edges * np.sign(np.where(det == 0, 1.0, det))[:, None, None]
  px, py = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
  P = np.stack([px.ravel(), py.ravel(), np.ones(H * W)], 0)                    # [3, HW]
  E = edges @ P                                                                 # [T, 3, HW]
  with np.errstate(divide="ignore", invalid="ignore"):
    dist = E / np.linalg.norm(edges[:, :, :2], axis=-1)[:, :, None]
    s = E.sum(1)
    bary = E / s[:, None]
    wf = (bary * w[:, :, None]).sum(1)
    z = (bary * clip[:, :, 2, None]).sum(1) / wf
  survives = ok[:, None] & (E >= 0).all(1) & (z >= -1) & (z <= 1)
  near_limit = (np.abs(np.abs(z) - 1) <= Z_EPS)
  return survives, z, bary, wf, np.abs(dist).min(1), near_limit


def restate(triangles, ranges, vps, size, cull):
  """-> dict of float64 / int arrays over [I, H, W]: triangle_index (-1: none), barycentrics [.., 3], depth, z_ndc (inf on
  background), covered, decided."""
  H, W = size
  tri = np.asarray(triangles, np.float64)
  I = len(ranges)
  culls = np.broadcast_to(np.asarray(cull, bool), (I,))
  out = {"triangle_index": np.full((I, H * W), -1, np.int64), "barycentrics": np.zeros((I, H * W, 3)),
         "depth": np.full((I, H * W), np.inf), "z_ndc": np.full((I, H * W), np.inf),
         "decided": np.ones((I, H * W), bool)}
  for i, (t0, t1) in enumerate(ranges):
    if t1 <= t0:
      continue
    sv, z, bary, wf, dist, lim = _fragments(tri[t0:t1], np.asarray(vps[i], np.float64), H, W, culls[i])
    ids = np.arange(t1 - t0)[:, None]
    key_z = np.where(sv, z, np.inf)
    # nearest first, the later triangle first on equal z
    order = np.lexsort((-np.broadcast_to(ids, z.shape), key_z), axis=0)
    first, second = order[0], order[1] if t1 - t0 > 1 else order[0]
    col = np.arange(H * W)
    has1 = sv[first, col]
    has2 = sv[second, col] & (t1 - t0 > 1)
    gap = np.where(has2, z[second, col] - z[first, col], np.inf)
    decided = ~(has1 & ((dist[first, col] <= EDGE_EPS) | lim[first, col]))
    decided &= ~(has2 & ((dist[second, col] <= EDGE_EPS) | lim[second, col] | (gap <= Z_EPS)))
    out["triangle_index"][i] = np.where(has1, first + t0, -1)
    out["barycentrics"][i] = np.where(has1[:, None], bary[first, :, col], 0.0)
    out["depth"][i] = np.where(has1, wf[first, col], np.inf)
    out["z_ndc"][i] = np.where(has1, z[first, col], np.inf)
    out["decided"][i] = decided
  out = {k: v.reshape((I, H, W) + v.shape[2:]) for k, v in out.items()}
  out["covered"] = out["triangle_index"] >= 0
  return out


def undecided_fraction(ref):
  """Per image: undecided covered pixels / covered pixels (0 for an empty image)."""
  cov = ref["covered"].reshape(ref["covered"].shape[0], -1)
  und = (~ref["decided"]).reshape(cov.shape) & cov
  return und.sum(1) / np.maximum(cov.sum(1), 1)


def deviations(buffers, ref):
  """Largest |float32 output - float64 restatement| per output over the decided pixels; triangle_index must be equal
  there (asserted)."""
  d = ref["decided"]
  idx = buffers.triangle_index.cpu().numpy()
  assert np.array_equal(idx[d], ref["triangle_index"][d]), int((idx[d] != ref["triangle_index"][d]).sum())
  fg = d & ref["covered"]
  out = {}
  for name in ("barycentrics", "depth", "z_ndc"):
    got = getattr(buffers, name).cpu().numpy().astype(np.float64)
    out[name] = float(np.abs(got[fg] - ref[name][fg]).max()) if fg.any() else 0.0
    bg = d & ~ref["covered"]
    assert np.array_equal(got[bg], ref[name][bg]), name                       # 0 / +inf on background, exactly
  return out


# ---------------------------------------------------------------- brute-force ray caster of a label grid
def ray_cast_labels(labels, voxel_to_view, vp, size):
  """labels int [D, H, W] (0: empty), voxel_to_view and vp 4 x 4 (voxel_to_view affine) -> (label int64 [H, W], 0 where
  the ray meets no drawn voxel, depth float64 [H, W], the clip w of the entry point, inf there)."""
  Hi, Wi = size
  g = np.asarray(labels)
  M = np.asarray(voxel_to_view, np.float64)
  vp = np.asarray(vp, np.float64)
  to_voxel = np.linalg.inv(vp @ M)                                              # clip -> voxel coordinates
  x = (np.arange(Wi) + 0.5) / Wi * 2 - 1
  y = (np.arange(Hi) + 0.5) / Hi * 2 - 1
  X, Y = np.meshgrid(x, y)

  def unproject(zn):
    h = np.stack([X.ravel(), Y.ravel(), np.full(Hi * Wi, zn), np.ones(Hi * Wi)], -1) @ to_voxel.T
    return h[:, :3] / h[:, 3:]
  o = unproject(-1.0)
  d = unproject(1.0) - o                                                        # the eye ray, near to far plane
  zz, yy, xx = np.nonzero(g)
  lo = np.stack([xx, yy, zz], -1).astype(np.float64)                            # [V, 3] cubes [lo, lo + 1]
  with np.errstate(divide="ignore", invalid="ignore"):
    t0 = (lo[None] - o[:, None]) / d[:, None]
    t1 = (lo[None] + 1 - o[:, None]) / d[:, None]
  tin = np.minimum(t0, t1).max(-1)                                              # [P, V]
  tout = np.maximum(t0, t1).min(-1)
  hit = (tin < tout) & (tin >= 0) & (tin <= 1)
  tin = np.where(hit, tin, np.inf)
  k = tin.argmin(1)
  any_hit = hit.any(1)
  tk = tin[np.arange(len(k)), k]
  point = o + np.where(any_hit, tk, 0.0)[:, None] * d
  clip = np.concatenate([point, np.ones((len(k), 1))], -1) @ (vp @ M).T
  label = np.where(any_hit, g[zz[k], yy[k], xx[k]], 0).astype(np.int64)
  depth = np.where(any_hit, clip[:, 3], np.inf)
  return label.reshape(Hi, Wi), depth.reshape(Hi, Wi)


# ---------------------------------------------------------------- scenes
def perspective_vp():
  from corenet_amd.visualization import camera_util as C
  return C.perspective_projection(1.0, znear=0.1, zfar=10)          # eye at the origin, looking along +z, fovy 60


def fixed(m):
  """m rounded to multiples of 2^-12: the same float32 matrix on every machine, whatever the last bits of its tan and
  sqrt are, so a scene checked on one machine is the same scene on another."""
  return t.round(t.as_tensor(m, dtype=t.float32) * 4096) / 4096


def _look(eye, at=(0.0, 0.0, 2.5)):
  from corenet_amd.geometry import transformations as T
  return fixed(t.matmul(perspective_vp(), T.look_at_lh(eye, at, (0, 1, 0))))


def soup_case():
  """I = 4 images of 29 x 37 (no multiple of the 16-pixel tile) of one soup: random triangles of both windings in front
  of the eye, two coincident triangles (the later one wins), a triangle with one vertex behind the eye, a triangle
  wholly beyond z_ndc = 1; ranges with t0 > 0 and an empty one, three cameras, culling on and off."""
  rng = np.random.RandomState(11)
  tri = (rng.rand(40, 3, 3) - 0.5) * 2.4
  tri[:, :, 2] = tri[:, :, 2] * 0.5 + 2.5
  big = np.array([[-0.35, -0.3, 2.1], [0.3, -0.3, 2.0], [0.0, 0.35, 2.2]])
  special = np.stack([big, big,                                                  # coincident: 41 wins over 40
                      [[0.3, -0.5, 1.5], [0.9, -0.4, 1.2], [0.6, 0.0, -0.5]],   # one vertex behind the eye
                      [[-3.0, -3.0, 12.0], [3.0, -3.0, 12.0], [0.0, 3.0, 12.0]]])  # beyond the far plane (zfar = 10)
  tri = t.from_numpy(np.concatenate([tri, special]).astype(np.float32))
  T_ = tri.shape[0]
  ranges = [[0, T_], [5, T_ - 1], [7, 7], [0, T_]]
  vps = t.stack([_look((0.0, 0.0, 0.0)), _look((0.5, 0.3, -0.2)), _look((-1.0, 2.0, 0.5)), _look((0.0, 0.0, 0.0))])
  return dict(triangles=tri, ranges=ranges, vps=vps, size=(29, 37), cull=[False, True, False, True])


def receding_case():
  """render_tex_check.receding_quad() under its perspective_vp(): clip w varies 5.5 x across the image."""
  import render_tex_check as X
  corners, uvs = X.receding_quad()
  tri, _ = X.quad(corners, uvs)
  return dict(triangles=tri, ranges=[[0, 2]], vps=X.perspective_vp()[None], size=(29, 37), cull=[False])


def cases():
  return {"soup": soup_case(), "receding": receding_case()}


def render_case(R, case, device="cpu", **kw):
  return R.render_geometry(case["triangles"].to(device), case["ranges"], case["vps"], case["size"], case["cull"], **kw)


def restate_case(case):
  return restate(case["triangles"].numpy(), case["ranges"], case["vps"].numpy(), case["size"], case["cull"])


def id_colour_image(R, case, device="cpu"):
  """The case drawn by render_batch with one material per triangle whose ambient colour is the three bytes of its index
  (diffuse and specular 0) and a white clear colour, decoded back -> int64 [I, H, W], -1 on background (index 2^24 - 1
  is no triangle)."""
  T_ = case["triangles"].shape[0]
  ids = np.arange(T_)
  mats = t.zeros(T_, 10)
  mats[:, :3] = t.from_numpy(np.stack([ids & 255, (ids >> 8) & 255, (ids >> 16) & 255], -1).astype(np.float32)) / 255
  mats[:, 9] = 1.0
  img = R.render_batch(case["triangles"].to(device), t.arange(T_, dtype=t.int32).to(device), mats.to(device), case["ranges"],
                       case["vps"], case["size"], clear_colors=(1.0, 1.0, 1.0), cull_back_facing=case["cull"])
  c = img.cpu().numpy().astype(np.int64)
  dec = c[..., 0] + 256 * c[..., 1] + 65536 * c[..., 2]
  return np.where(dec == (1 << 24) - 1, -1, dec)


def long_list_soup():
  """2 images of 48 x 80 (3 x 5 tiles) of 3000 small triangles that all land in a few tiles around the image centre:
  per-tile lists of hundreds to thousands of records (several staged chunks and a partial last one), and empty tiles."""
  rng = np.random.RandomState(5)
  T_ = 3000
  tri = (rng.rand(T_, 3, 3).astype(np.float32) - 0.5) * 1.2
  tri[:, :, 2] = tri[:, :, 2] * 0.5 + 2.5
  tri[T_ // 2:T_ // 2 + T_ // 8] = tri[:T_ // 8]                      # coplanar duplicates: ties on z
  vp = fixed(perspective_vp())
  return dict(triangles=t.from_numpy(tri), ranges=[[0, T_], [100, 1125]], vps=t.stack([vp, vp]), size=(48, 80),
              cull=[False, True])


def label_grid_case():
  """A 12 x 10 x 9 (D, H, W) grid with three labels in view space (1 / 12 per voxel) seen from two cameras at 40 x 56."""
  rng = np.random.RandomState(3)
  g = np.zeros((12, 10, 9), np.int32)
  g[2:9, 2:8, 1:7] = 1
  g[4:11, 1:5, 3:9] = 2
  g[1:5, 5:9, 4:8] = 3
  g[rng.rand(*g.shape) < 0.15] = 0
  from corenet_amd.geometry import transformations as T
  m = T.scale([1 / 12.0] * 3)
  vps = t.stack([_look((1.2, 1.0, -0.7), (0.4, 0.4, 0.5)), _look((-0.4, 0.25, -0.9), (0.4, 0.4, 0.5))])
  return t.from_numpy(g), m, vps, (40, 56)


def check_label_grid(R, device):
  """voxel_faces of the label grid through render_geometry against the ray caster: the label image
  material_ids[triangle_index] and the depth at decided pixels."""
  g, m, vps, size = label_grid_case()
  pal = t.zeros(4, 3)
  pal[0] = -1.0
  f = R.voxel_faces(g[None].to(device), pal, m)
  T_ = f.triangles.shape[0]
  buf = R.render_geometry(f.triangles, [[0, T_], [0, T_]], vps, size)
  labels = R.gather_triangle_attribute(buf, f.material_ids, 0).cpu().numpy()
  ref = restate(f.triangles.cpu().numpy(), [[0, T_], [0, T_]], vps.numpy(), size, False)
  assert (undecided_fraction(ref) <= MAX_UNDECIDED).all(), undecided_fraction(ref)
  for i in range(2):
    lab, dep = ray_cast_labels(g.numpy(), m.numpy(), vps[i].numpy(), size)
    d = ref["decided"][i]
    assert (lab > 0).sum() > 300
    assert np.array_equal(buf.triangle_index[i].cpu().numpy()[d], ref["triangle_index"][i][d])
    assert np.array_equal(labels[i][d], lab[d]), (i, int((labels[i][d] != lab[d]).sum()))
    fg = d & (lab > 0)
    err = np.abs(buf.depth[i].cpu().numpy().astype(np.float64)[fg] - dep[fg]).max()
    assert err <= TOL["depth"], (i, err)
  return buf


# ---------------------------------------------------------------- batches of the reprojection tests
def fixture_elements():
  import os
  from corenet_amd.data import dataset as D
  root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "n2_dataset")
  ds = D.CoReNetDatasetImpl(os.path.join(root, "dataset.json"), os.path.join(root, "meshes"))
  return [ds[0], ds[1]]


def host_fixture_batch(res=32):
  """The two fixture scenes as a BatchedExample on the host: their cameras, images, labels and view-space meshes
  (transformed with torch), and -- the voxelizer being a GPU kernel -- a ground-truth grid of res^3 in which mesh k fills
  the voxels whose centres lie in its view-space bounding box (later meshes on top)."""
  from corenet_amd.data.batched_example import BatchedExample
  from corenet_amd.geometry import transformations as T
  els = fixture_elements()
  verts, grids = [], []
  c = (t.arange(res, dtype=t.float32) + 0.5) / res
  for e in els:
    g = t.zeros(res, res, res, dtype=t.int32)
    ends = t.cumsum(e.mesh_num_tri.to(t.int64), 0)
    for k, (a, b) in enumerate(zip((ends - e.mesh_num_tri).tolist(), ends.tolist())):
      v = T.transform_mesh(e.mesh_vertices[a:b], t.matmul(e.view_transform, e.o2w_transforms[k]))
      verts.append(v)
      lo, hi = v.reshape(-1, 3).min(0)[0], v.reshape(-1, 3).max(0)[0]
      inside = [(c >= lo[q]) & (c <= hi[q]) for q in range(3)]              # x, y, z
      g[inside[2][:, None, None] & inside[1][None, :, None] & inside[0][None, None, :]] = int(e.mesh_labels[k])
    grids.append(g)
  B = len(els)
  return BatchedExample(
      vertices=t.cat(verts), view_transform=t.stack([e.view_transform for e in els]),
      camera_transform=t.stack([e.camera_transform for e in els]), mesh_num_tri=[e.mesh_num_tri for e in els],
      mesh_labels=[e.mesh_labels for e in els], input_image=t.stack([e.input_image for e in els]),
      scene_id=[e.scene_id for e in els], grid_sampling_offset=t.full((B, 3), 0.5),
      v2x_transform=t.diag(t.tensor([float(res)] * 3 + [1.0])).expand(B, 4, 4).clone(), grid=t.stack(grids))


def one_hot_pmf(grid, C):
  return t.nn.functional.one_hot(grid.to(t.int64).clamp(0, C - 1), C).permute(0, 4, 1, 2, 3).float()


def shifted_example():
  """(pmf f32 [1, 3, 8, 8, 8], BatchedExample, predicted grid): one scene, an 8^3 grid with two labels in the unit cube,
  a 24 x 20 input image, and a prediction that is the ground truth moved by one voxel along x."""
  from corenet_amd.data.batched_example import BatchedExample
  from corenet_amd.geometry import transformations as T
  g = t.zeros(8, 8, 8, dtype=t.int32)
  g[2:6, 1:5, 2:5] = 1
  g[3:7, 4:7, 4:7] = 2
  pred = t.zeros_like(g)
  pred[:, :, 1:] = g[:, :, :-1]
  cam = _look((1.37, 1.21, -1.29), (0.5, 0.45, 0.55))
  ex = BatchedExample(
      vertices=t.zeros(0, 3, 3), view_transform=t.eye(4)[None], camera_transform=cam[None],
      mesh_num_tri=[t.tensor([0, 0], dtype=t.int32)], mesh_labels=[t.tensor([1, 2], dtype=t.int32)],
      input_image=t.zeros(1, 3, 24, 20, dtype=t.uint8), scene_id=["synthetic/shifted"],
      grid_sampling_offset=t.full((1, 3), 0.5), v2x_transform=T.scale([8.0] * 3)[None], grid=g[None])
  return one_hot_pmf(pred[None], 3), ex, pred


def reprojection_reference(pred, gt, voxel_to_view, cam, size, C):
  """The rows reprojection_metrics_for_batch should give for one scene, from the ray caster's label and depth images."""
  pl, pd = ray_cast_labels(pred.numpy(), voxel_to_view, cam, size)
  gl, gd = ray_cast_labels(gt.numpy(), voxel_to_view, cam, size)
  pm, gm = pl > 0, gl > 0
  both = pm & gm
  err = np.abs(pd[both] - gd[both])
  ratio = np.maximum(pd[both] / gd[both], gd[both] / pd[both])
  assert (np.abs(ratio - 1.25) > 1e-3).all()
  table = np.zeros((C, C), np.int64)
  np.add.at(table, (pl.ravel(), gl.ravel()), 1)
  return dict(intersection=int(both.sum()), union=int((pm | gm).sum()), count=int(both.sum()), abs_sum=err.sum(),
              sq_sum=(err ** 2).sum(), abs_rel_sum=(err / gd[both]).sum(), delta1_count=int((ratio < 1.25).sum()),
              table=table)


def all_decided(R, grid, voxel_to_view, cam, size):
  """Whether every pixel of the grid's face image is decided (restate on the faces voxel_faces emits)."""
  pal = t.zeros(int(grid.max()) + 1, 3)
  pal[0] = -1.0
  f = R.voxel_faces(grid[None], pal, t.as_tensor(voxel_to_view, dtype=t.float32))
  T_ = f.triangles.shape[0]
  return bool(restate(f.triangles.numpy(), [[0, T_]], np.asarray(cam)[None], size, False)["decided"].all())


def check_shifted_example(ER, R, device):
  """The shifted example on device against the ray caster: counts and tables exact (every pixel is decided), the depth
  sums within TOL["depth"] times the pixel count.  Returns the rows."""
  pmf, ex, pred = shifted_example()
  cam, size = ex.camera_transform[0].numpy(), (24, 20)
  m = np.diag([1 / 8.0] * 3 + [1.0])
  assert all_decided(R, pred, m, cam, size) and all_decided(R, ex.grid[0], m, cam, size)
  ref = reprojection_reference(pred, ex.grid[0], m, cam, size, 3)
  assert ref["intersection"] >= 25 and ref["union"] > ref["intersection"]     # the shift shows
  rows = ER.reprojection_metrics_for_batch(pmf.to(device), ex.to(device), "semantic")
  s, d = rows.silhouette, rows.depth
  assert s.intersection.tolist() == [ref["intersection"]] and s.union.tolist() == [ref["union"]]
  assert abs(float(s.iou) - ref["intersection"] / ref["union"]) < 1e-15
  assert d.count.tolist() == [ref["count"]] and d.delta1_count.tolist() == [ref["delta1_count"]]
  for name in ("abs_sum", "sq_sum", "abs_rel_sum"):
    got = float(getattr(d, name))
    print(name, got, float(ref[name]))
    assert abs(got - float(ref[name])) <= TOL["depth"] * ref["count"], name
  table = ref["table"]
  inter = [int(table[k, k]) for k in (1, 2)]
  union = [int(table[k].sum() + table[:, k].sum() - table[k, k]) for k in (1, 2)]
  assert rows.class_index.tolist() == [1, 2] and rows.scene_index.tolist() == [0, 0]
  assert rows.class_intersection.tolist() == inter and rows.class_union.tolist() == union
  return rows


def rows_equal(a, b):
  """Two ReprojectionRows with the same values bit for bit (NaN == NaN), wherever their tensors live."""
  def same(x, y):
    x, y = x.cpu(), y.cpu()
    return x.dtype == y.dtype and x.shape == y.shape and t.equal(t.nan_to_num(x.double(), nan=-1.0),
                                                                 t.nan_to_num(y.double(), nan=-1.0))
  assert a.scene_id == b.scene_id and a.class_scene_id == b.class_scene_id
  for name in ("scene_index", "class_index", "class_intersection", "class_union", "class_iou"):
    assert same(getattr(a, name), getattr(b, name)), name
  for x, y, name in zip(tuple(a.silhouette) + tuple(a.depth), tuple(b.silhouette) + tuple(b.depth),
                        a.silhouette._fields + a.depth._fields):
    assert same(x, y), name


def check_identity_rows(rows, B):
  """A prediction equal to the ground truth with gt="grid": IoU exactly 1, every depth sum exactly 0, delta_1 exactly 1."""
  s, d = rows.silhouette, rows.depth
  assert bool((s.intersection == s.union).all()) and bool((s.union > 50).all()) and s.iou.tolist() == [1.0] * B
  assert d.abs_sum.tolist() == [0.0] * B and d.sq_sum.tolist() == [0.0] * B and d.abs_rel_sum.tolist() == [0.0] * B
  assert t.equal(d.count.cpu(), s.intersection.cpu()) and t.equal(d.delta1_count.cpu(), d.count.cpu())
  seen = rows.class_union.cpu() > 0
  assert bool(seen.any()) and t.equal(rows.class_intersection.cpu(), rows.class_union.cpu())
  assert bool((rows.class_iou.cpu()[seen] == 1.0).all()) and bool(t.isnan(rows.class_iou.cpu()[~seen]).all())
