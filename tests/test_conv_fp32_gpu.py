"""The fp32 convolution engine (csrc/conv_igemm.hip, csrc/conv_kernels.h: crn_conv_fwd, crn_conv_wgrad) on the GPU, every row of
tests/conv_fp32_cases.py against a float64 reference: torch's conv3d / conv_transpose3d on the case's inputs as doubles, the
fused transform applied in float64, autograd in float64 for the weight gradient.  Bars: 3e-5 of max|reference| forward and data
gradient, 5e-5 weight gradient (tests/test_conv_plan_cpu.py shows that the references leave two thirds of them to the kernel and
that ten kernel bugs miss them by 10x or more).  Every output buffer starts at a sentinel or at random contents; whatever the
output view does not address -- neighbouring channels of a concat buffer, pad elements of a strided buffer -- must come back
bit-identical.  Which kernel ran is asked of the plan query on the very views of the launch."""
import functools
import os
import time

import pytest
import torch as t

import conv_fp32_cases as K
from conv_fp32_cases import CASES, BAR_FWD, BAR_WGRAD, SENTINEL
from kernel_contract_emu import EmuBackend

pytestmark = pytest.mark.gpu

EMU = EmuBackend()
# CRN_TEST_SELFCHECK=1 runs the test LOGIC against the contract emulator on CPU (as tests/test_kernels_gpu.py does)
_SELF = os.environ.get("CRN_TEST_SELFCHECK") == "1"
DEV = "cpu" if _SELF else "cuda"
_DET_ENV = os.environ.get("CRN_DETERMINISTIC", "0") == "1"
FWD = [c.name for c in CASES if c.op == "fwd"]
WGRAD = [c.name for c in CASES if c.op == "wgrad"]
MAXERR = {}          # path -> (largest error / bar seen, case)


@pytest.fixture(scope="module")
def be():
  t0 = time.time()
  if _SELF:
    yield EMU
  else:
    from corenet_amd.backend import HipBackend
    assert t.cuda.is_available(), "gpu tests need an MI355X"
    yield HipBackend()
  print("\nfp32 conv engine, largest error per path (in units of max|float64 reference|):")
  for path in sorted(MAXERR):
    err, name = MAXERR[path]
    print(f"  {path:24s} {err:.2e}  ({name})")
  print(f"  module wall time {time.time() - t0:.1f} s")


@functools.lru_cache(maxsize=None)
def built(name):
  return K.build(K.BY_NAME[name])


@functools.lru_cache(maxsize=None)
def ref_of(name):
  b = built(name)
  return K.FwdRef(b) if b.case.op == "fwd" else K.WgradRef(b)


def _plan(be, b):
  """The plan of the case's launch on device storages, checked against the row (None under the emulator)."""
  if _SELF:
    return None
  c = b.case
  ys = (b.y0 if c.op == "fwd" else b.dys).to(DEV)
  p = K.query_plan(be, b, b.xs.to(DEV), ys, b.wp.to(DEV), None if c.op == "fwd" else b.dw0.to(DEV))
  want = {k: v for k, v in c.expect.items() if not (_DET_ENV and k == "splits")}
  assert {k: p[k] for k in want} == want, f"{c.name}: on the device's views the plan is {p}"
  return p


def _note(path, err, bar, name):
  if path not in MAXERR or err > MAXERR[path][0]:
    MAXERR[path] = (err, name)
  print(f"{name}: {path} max error {err:.2e} of the range (bar {bar:.0e})")


def _path_name(c, p):
  if p is None: return c.op + " " + c.expect["path"]
  if p["path"] != "generic": return c.op + " " + p["path"]
  return f"{c.op} generic x{p['xstage']}" + (f" dy{p['dystage']}" if c.op == "wgrad" else "")


@pytest.mark.parametrize("name", FWD)
def test_forward_case(be, name):
  b, r = built(name), ref_of(name)
  c = b.case
  p = _plan(be, b)
  y = K.run_fwd(be, b, DEV)
  err, outside = r.check(b, y)
  _note(_path_name(c, p), err, BAR_FWD, name)
  assert outside, f"{name}: elements outside the output view changed"
  assert err <= BAR_FWD, f"{name}: {err:.3e} of max|ref| > {BAR_FWD}"
  splits = c.expect.get("splits", 1) if p is None else p["splits"]
  if splits > 1 and c.expect["path"] in ("generic", "pointwise"):
    # the same call armed with crn_splitk_defer: the sum stays pending (or is reduced at once when y cannot take it) until an
    # unrelated entry of the library flushes it -- the same bits either way
    other = t.ones(8, device=DEV)
    be.splitk_defer(True)
    y2 = K.run_fwd(be, b, DEV)
    be.zero(other)
    assert t.equal(y2.view(t.int32), y.view(t.int32)), f"{name}: armed with crn_splitk_defer the result differs"
    assert float(other.abs().max()) == 0.0


@pytest.mark.parametrize("name", WGRAD)
def test_wgrad_case(be, name):
  b, r = built(name), ref_of(name)
  c = b.case
  if c.deterministic: be.set_deterministic(True)
  try:
    p = _plan(be, b)
    dw = K.run_wgrad(be, b, DEV)
    err, pad_ok = r.check(b, dw)
    _note(_path_name(c, p), err, BAR_WGRAD, name)
    assert pad_ok, f"{name}: columns past Cout of an accumulating call changed"
    assert err <= BAR_WGRAD, f"{name}: {err:.3e} of max|ref| > {BAR_WGRAD}"
    if c.deterministic:                       # one workgroup per dw element, a fixed order: the same bits again
      assert t.equal(K.run_wgrad(be, b, DEV).view(t.int32), dw.view(t.int32))
  finally:
    if c.deterministic: be.set_deterministic(_DET_ENV)


def test_split_by_atomics_under_graph_capture(be):
  """Mode 2 of the generic forward kernel: a stream under capture that was given no scratch (no crn_splitk_reserve) cannot
  grow one, so the launch zeroes y and adds its splits with atomics.  Captured on a fresh stream, replayed once."""
  # Mode 2 is inferred, not observed: it rests on crn_splitk_scratch (csrc/splitk.hip) returning nullptr for a stream whose
  # slot is too small while hipStreamIsCapturing says it is being captured ("if (cap != hipStreamCaptureStatusNone) return
  # nullptr;").  Should a capture stream ever be given a slot lazily, this test would run mode 3 instead.
  name = "s_auto_x0_b"
  b, r = built(name), ref_of(name)
  if _SELF:
    y = K.run_fwd(be, b, DEV)
  else:
    assert _plan(be, b)["splits"] > 1
    K.run_fwd(be, b, DEV); K.run_fwd(be, built("d_cols_1024"), DEV)     # code objects load outside the capture
    xs, wp, bp = b.xs.to(DEV), b.wp.to(DEV), b.bp.to(DEV)
    y = b.y0.to(DEV).clone()
    xv, yv, tr = K.xview(b, xs), K.yview(b, y), K.transform_of(b, DEV)
    t.cuda.synchronize()
    side = t.cuda.Stream()
    graph = t.cuda.CUDAGraph()
    try:
      with t.cuda.stream(side):
        with t.cuda.graph(graph, stream=side):
          be.conv_fwd(xv, tr, wp, b.npad, bp, 0, yv, b.window, b.pad_lo, 0, False)
      t.cuda.synchronize()
      assert float((y - b.y0.to(DEV)).abs().max()) == 0.0          # captured, not run
      graph.replay()
      t.cuda.synchronize()
    finally:
      del graph
      be.splitk_release(side)
  err, outside = r.check(b, y)
  _note("fwd generic atomics", err, BAR_FWD, name)
  assert outside and err <= BAR_FWD, f"{err:.3e}"


def test_rejected_calls_launch_nothing(be):
  """CRN_EINVAL before anything is written: the output keeps its sentinel."""
  if _SELF:
    return                      # (the plan queries' statuses for the same calls: tests/test_conv_plan_cpu.py)
  import ctypes as C
  from corenet_amd import _lib
  from corenet_amd.backend import _cview
  L = be.lib
  B, cin, cout, dims = 2, 8, 16, (2, 4, 8)
  S = dims[0] * dims[1] * dims[2]
  xs = t.randn(B * cin * S, device=DEV); w = t.randn(cin * 512 * 32, device=DEV)
  ys = t.full((3 * 17 * S,), SENTINEL, device=DEV); dw = t.full((cin * 576 * 16,), SENTINEL, device=DEV)
  view = lambda st, b_, cn: C.byref(_cview(K.make_view("plain", st, b_, cn, dims)))
  st = _lib.stream()
  def fwd(x=None, y=None, npad=16, k=(3, 3, 3), boxes=None):
    return L._crn_conv_fwd(x or view(xs, B, cin), None, w.data_ptr(), npad, None, 0, y or view(ys, B, cout), *k, 1, 1, 1, 0, 0, boxes, st)
  def wg(x=None, dy=None, npad=16, k=(3, 3, 3)):
    return L._crn_conv_wgrad(x or view(xs, B, cin), None, dy or view(ys, B, cout), dw.data_ptr(), npad, *k, 1, 1, 1, 1, None, st)
  assert fwd(npad=24) == -1 and wg(npad=24) == -1
  assert fwd(y=view(ys, B, 17)) == -1
  assert fwd(y=view(ys, 3, cout)) == -1 and wg(dy=view(ys, 3, cout)) == -1
  for n, cg in ((9, 0), (0, 9), (-1, 0)):
    tb = _lib.CrnTapBoxes(); tb.n_groups, tb.c_groups = n, cg
    assert fwd(boxes=C.cast(C.pointer(tb), C.c_void_p)) == -1
  assert fwd(k=(6, 6, 6)) == -1
  assert wg(k=(8, 8, 9)) == -1
  t.cuda.synchronize()
  assert float((ys - SENTINEL).abs().max()) == 0.0 and float((dw - SENTINEL).abs().max()) == 0.0
