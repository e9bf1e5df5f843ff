"""Textured rendering on the MI355X: every case of render_tex_check.py on the HIP kernel, each image also compared with
the library's host twin bit for bit (no material has a specular term)."""
import signal

import pytest
import torch as t

import render_tex_check as X

pytestmark = pytest.mark.gpu
_DEVICE_KEYS = ("normals", "tex_coords", "textures")


@pytest.fixture(scope="module")
def R():
  from corenet_amd.visualization import render as R
  return R


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


def _gpu(fn, seconds=120):
  with limit(seconds):
    out = fn()
    t.cuda.synchronize()
  return out


@pytest.fixture(scope="module")
def render(R):
  """render_batch on the GPU for host tensors -> host image, asserted equal to the host twin's."""
  def both(tri, mids, mats, ranges, vps, size, **kw):
    dkw = {k: (v.cuda() if k in _DEVICE_KEYS and v is not None else v) for k, v in kw.items()}
    g = _gpu(lambda: R.render_batch(tri.cuda(), mids.cuda(), mats.cuda(), ranges, vps, size, **dkw))
    c = R.render_batch(tri, mids, mats, ranges, vps, size, **kw)
    assert g.device.type == "cuda" and g.dtype == t.uint8
    assert t.equal(g.cpu(), c), int((g.cpu() != c).any(-1).sum())
    return c
  return both


@pytest.mark.parametrize("kind", ["random", "checker"])
@pytest.mark.parametrize("uv_range", list(X.UV_RANGES))
@pytest.mark.parametrize("tex_size", X.TEX_SIZES, ids=lambda s: "%dx%d" % s)
def test_orthographic_against_float64(render, tex_size, uv_range, kind):
  X.case_orthographic(render, tex_size, uv_range, kind)


def test_perspective_against_float64(render):
  X.case_perspective(render)


def test_row_orientation(render):
  X.case_row_orientation(render)


def test_layers_and_materials(render):
  X.case_layers_and_materials(render)


@pytest.mark.parametrize("normals", [True, False], ids=["normals", "geometric"])
def test_bit_exact_identities(render, normals):
  X.case_identities(render, normals)


def test_non_finite_and_huge_coordinates(render):
  X.case_non_finite(render)


def test_batching(render):
  X.case_batching(render)


def test_validation_raises_before_any_launch(R, monkeypatch):
  """Every ValueError comes before the library is touched: with it taken away, the errors are still ValueErrors."""
  def no_library():
    raise AssertionError("the library was reached before the arguments were checked")

  def gpu_only(tri, mids, mats, ranges, vps, size, **kw):
    dkw = {k: (v.cuda() if k in _DEVICE_KEYS and v is not None else v) for k, v in kw.items()}
    return _gpu(lambda: R.render_batch(tri.cuda(), mids.cuda(), mats.cuda(), ranges, vps, size, **dkw))
  tri, uv = X.quad(X.rect(-2, 2, -2, 2), X.rect_uv(0, 1, 0, 1))
  with monkeypatch.context() as m:
    m.setattr(R, "_lib", no_library)
    with pytest.raises(AssertionError):                              # a valid call does reach it
      gpu_only(tri, t.zeros(2, dtype=t.int32), X.flat_materials([X.DIFFUSE]), [[0, 2]], t.eye(4)[None], (8, 8),
               tex_coords=uv, textures=t.zeros((1, 2, 2, 3), dtype=t.uint8), texture_indices=t.tensor([0]))

    def checked(*a, **kw):
      if "tex_coords" in kw and "textures" in kw and kw["texture_indices"].tolist() == [0, 1]:
        return None                                                  # case_validation's closing valid call
      return gpu_only(*a, **kw)
    X.case_validation(checked)
  X.case_validation(gpu_only)


def test_render_scenes(R, render):
  X.case_render_scenes(R, "cuda", render)
