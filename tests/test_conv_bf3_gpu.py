"""The split-bf16 convolution engine (csrc/conv_bf3.hip: crn_conv_fwd_bf3, crn_conv_fwd_bf3_slabs and its two fused BatchRenorm
epilogues, crn_conv_wgrad_bf3_boxes) on the GPU, every row of tests/conv_bf3_cases.py against a float64 reference: torch's conv3d /
conv_transpose3d on the case's inputs as doubles, the fused transform applied in float64, autograd in float64 for the gradients.
Two bars per row: the project's 2e-5 of max|reference| against float64 (tests/test_conv_bf3_plan_cpu.py shows that the operand
split itself takes at most half of it and that eight kernel bugs miss it by 10x or more), and SPLIT_BAR against the split model --
the same products summed in float64 -- from which only the order of the float32 sums separates the kernel.  Every output buffer
starts at a sentinel or at random contents; whatever the output view does not address must come back bit-identical.  Which kernel
ran is asked of the plan query on the very views of the launch."""
import ctypes as C
import functools
import os
import time

import pytest
import torch as t

import conv_bf3_cases as K
import conv_fp32_cases as K32
from conv_bf3_cases import CASES, BAR, SPLIT_BAR, SENTINEL
from conv_bf3_cases import rejections

pytestmark = pytest.mark.gpu

DEV = "cuda"
_DET_ENV = os.environ.get("CRN_DETERMINISTIC", "0") == "1"
FWD = [c.name for c in CASES if c.op == "fwd" and not c.fuse]
FUSE = [c.name for c in CASES if c.fuse]
WGRAD = [c.name for c in CASES if c.op == "wgrad"]
MAXERR = {}          # kernel family -> [largest error against float64, against the split model] in units of max|reference|
WS_SENT = -7.25


@pytest.fixture(scope="module")
def be():
  t0 = time.time()
  from corenet_amd.backend import HipBackend
  assert t.cuda.is_available(), "gpu tests need an MI355X"
  yield HipBackend()
  print("\nsplit-bf16 conv engine, largest error per kernel family (of max|float64 reference|): against float64, against the split model")
  for fam in sorted(MAXERR):
    print(f"  {fam:28s} {MAXERR[fam][0]:.2e}  {MAXERR[fam][1]:.2e}")
  print(f"  module wall time {time.time() - t0:.1f} s")


@functools.lru_cache(maxsize=None)
def built(name):
  return K.build(K.BY_NAME[name])


@functools.lru_cache(maxsize=None)
def ref_of(name):
  return K.make_ref(built(name))


def _plan(be, b, fuse=None):
  """The plan of the case's launch on device storages, checked against the row."""
  c = b.case
  ys = (b.y0 if c.op == "fwd" else b.dys).to(DEV)
  p = K.query_plan(be, b, b.xs.to(DEV), ys, b.wp.to(DEV), None if c.op == "fwd" else b.dw0.to(DEV),
                   slab=b.slab.to(DEV) if c.slabs else None, fuse=fuse)
  want = {k: v for k, v in c.expect.items() if not (_DET_ENV and k in ("splits", "per_split"))}
  assert {k: p[k] for k in want} == want, f"{c.name}: on the device's views the plan is {p}"
  return p


def _family(c, p):
  if c.op == "wgrad": return f"wgrad tpw{p['tpw']} dy{p['dmode']} w{p['twt']}"
  return f"fwd {p['kind']} x{p['xmode']} ng{p['ng']}" + (" split" if p["splits"] > 1 else "")


def _note(fam, e64, esp, name):
  m = MAXERR.setdefault(fam, [0.0, 0.0])
  m[0], m[1] = max(m[0], e64), max(m[1], esp)
  print(f"{name}: {fam}: {e64:.2e} of the range against float64 (bar {BAR:.0e}), {esp:.2e} against the split model (bar {SPLIT_BAR:.1e})")


@pytest.mark.parametrize("name", FWD)
def test_forward_case(be, name):
  b, r = built(name), ref_of(name)
  c = b.case
  p = _plan(be, b)
  y = K.run_fwd(be, b, DEV)
  e64, esp, outside = r.check(b, y)
  _note(_family(c, p), e64, esp, name)
  assert outside, f"{name}: elements outside the output view changed"
  assert e64 <= BAR, f"{name}: {e64:.3e} of max|ref| > {BAR}"
  assert esp <= SPLIT_BAR, f"{name}: {esp:.3e} of max|ref| from the split model > {SPLIT_BAR}"
  # the other form of the weights (staged fp32 / pre-arranged slabs) multiplies the same operands in the same order -- the
  # wave-specialised kernel, which exists for slabs only, included: the same bits
  y2 = K.run_fwd(be, b, DEV, slabs=not c.slabs)
  assert t.equal(y2.view(t.int32), y.view(t.int32)), f"{name}: the staged-weights and the slab form differ"
  if p["splits"] > 1:
    # armed with crn_splitk_defer: the sum stays pending (or is reduced at once when y cannot take it) until an unrelated entry
    # of the library flushes it -- the same bits either way
    other = t.ones(8, device=DEV)
    be.splitk_defer(True)
    y3 = K.run_fwd(be, b, DEV)
    be.zero(other)
    assert t.equal(y3.view(t.int32), y.view(t.int32)), f"{name}: armed with crn_splitk_defer the result differs"
    assert float(other.abs().max()) == 0.0


@pytest.mark.parametrize("name", WGRAD)
def test_wgrad_case(be, name):
  b, r = built(name), ref_of(name)
  c = b.case
  if c.deterministic: be.set_deterministic(True)
  try:
    p = _plan(be, b)
    dw = K.run_wgrad(be, b, DEV)
    e64, esp, pad_ok = r.check(b, dw)
    _note(_family(c, p), e64, esp, name)
    assert pad_ok, f"{name}: entries that hold no tap (columns past dy->C included) are not what the contract says"
    assert e64 <= BAR, f"{name}: {e64:.3e} of max|ref| > {BAR}"
    assert esp <= SPLIT_BAR, f"{name}: {esp:.3e} of max|ref| from the split model > {SPLIT_BAR}"
    if c.deterministic:                       # one workgroup per dw element, a fixed order: the same bits again
      assert p["splits"] == 1
      assert t.equal(K.run_wgrad(be, b, DEV).view(t.int32), dw.view(t.int32))
  finally:
    if c.deterministic: be.set_deterministic(_DET_ENV)


def _raw_fwd_args(b, xs, slab, bp, y):
  from corenet_amd.backend import _cview, _ctr, _ctapboxes
  c = b.case
  return (C.byref(_cview(K.xview(b, xs))), _ctr(K.transform_of(b, DEV)), slab.data_ptr(), b.npad, None if bp is None else bp.data_ptr(),
          b.bias_sB, C.byref(_cview(K.yview(b, y))), *b.window, *b.pad_lo, int(c.accumulate), _ctapboxes(b.boxes))


@pytest.mark.parametrize("name", FUSE)
def test_fused_epilogue_case(be, name):
  """crn_conv_fwd_bf3_slabs_stats / _bnbwd at partial tiles: y bit-identical to the plain call's, the parts of the launch summed in
  float64 equal to float64 sums over the launch's own y (3e-6 / 2e-5 of the largest sum, the bars of the model-shape tests), the
  workspace beyond the parts untouched; a declining launch (nparts == 0) writes y all the same and leaves the workspace alone."""
  from corenet_amd import _lib
  b, r = built(name), ref_of(name)
  c = b.case
  S = c.odims[0] * c.odims[1] * c.odims[2]
  Cn = b.ycout
  y_plain = K.run_fwd(be, b, DEV)
  e64, esp, outside = r.check(b, y_plain)
  assert outside and e64 <= BAR and esp <= SPLIT_BAR, (name, e64, esp, outside)
  ws = t.full((K.WS_BYTES(b) // 8,), WS_SENT, dtype=t.float64, device=DEV)
  dsum = t.full((600,), WS_SENT, device=DEV)
  xs, slab = b.xs.to(DEV), b.slab.to(DEV)
  bp = None if b.bp is None else b.bp.to(DEV)
  y = b.y0.to(DEV).clone()
  bn_x = b.bn_x.to(DEV) if c.fuse == "bnbwd" else None
  saved = b.bn_saved.to(DEV) if c.fuse == "bnbwd" else None
  f = K.fuse_request(b, ws, dsum, bn_x, saved)
  p = _plan(be, b, fuse=f)
  args = _raw_fwd_args(b, xs, slab, bp, y)
  if c.fuse == "stats":
    n = C.c_int(-1)
    be.lib.crn_conv_fwd_bf3_slabs_stats(*args, 1, f.ws, f.ws_bytes, C.byref(n), _lib.stream())
    nparts = n.value
  else:
    be.lib.crn_conv_fwd_bf3_slabs_bnbwd(*args, C.byref(f), _lib.stream())
    nparts = f.nparts
  want_parts = c.expect["nparts"]
  assert nparts == want_parts == p["nparts"], (name, nparts, want_parts, p["nparts"])
  assert t.equal(y.view(t.int32), y_plain.view(t.int32)), f"{name}: y differs from the plain call's"
  wsc, dsc = ws.cpu(), dsum.cpu()
  if nparts == 0:
    assert bool((wsc == WS_SENT).all()) and bool((dsc == WS_SENT).all()), f"{name}: a declining launch wrote its workspace"
    return
  assert nparts == K.parts_of(c)
  assert bool((wsc[Cn * nparts * 2:] == WS_SENT).all()), f"{name}: workspace written past the parts"
  got = wsc[:Cn * nparts * 2].view(Cn, nparts, 2).sum(1)                       # float64
  yk = K.logical(K.yview(b, y.cpu().double()))                                # the launch's own y, [B, Cn, D, H, W]
  if c.fuse == "stats":
    yr = yk.relu()
    want = t.stack([yr.sum((0, 2, 3, 4)), (yr * yr).sum((0, 2, 3, 4))], 1)
    bar = 3e-6
    assert bool((dsc == WS_SENT).all())
  else:
    xn = b.bn_x[:c.B * Cn * S].double().view(c.B, Cn, *c.odims).relu()
    mu, rstd = b.bn_saved[:Cn].double().view(1, -1, 1, 1, 1), b.bn_saved[Cn:2 * Cn].double().view(1, -1, 1, 1, 1)
    want = t.stack([yk.sum((0, 2, 3, 4)), (yk * ((xn - mu) * rstd)).sum((0, 2, 3, 4))], 1)
    bar = 2e-5
    assert bool((dsc[:K.NDSUM] == 0).all()) and bool((dsc[K.NDSUM:] == WS_SENT).all()), f"{name}: dsum[:ndsum] zeroed, the rest untouched"
  for j, nm in enumerate(("first sum", "second sum")):
    e = float((got[:, j] - want[:, j]).abs().max() / want[:, j].abs().max())
    print(f"{name}: {c.fuse} {nm}: {e:.2e} of the largest (bar {bar:.0e})")
    assert e <= bar, (name, nm, e)


def test_rejected_calls_write_nothing(be):
  """Every rejection of the two entries (the list of tests/test_conv_bf3_plan_cpu.py, built from the code): the plan query and the
  launch both return CRN_EINVAL on the device's views, and y / dw keep their sentinel -- the zero_first memset of the weight
  gradient included (it used to run before the last two rejections).  Not checked: the split-K scratch.  The library owns it and
  exports no way to read it; that a rejected forward call does not touch the split-K state is shown by the arming test below, and
  bf3_fwd_select, which holds every rejection, makes no HIP call at all."""
  from corenet_amd import _lib
  st = _lib.stream()
  out = _lib.CrnBf3Plan()
  keep = []
  for name, op, mk in rejections():
    a = mk(DEV)
    keep.append(a)
    if op == "fwd":
      rq = be.lib._crn_conv_fwd_bf3_plan(*a["args"][:2], a["w"], None, *a["args"][2:], None, C.byref(out))
      assert rq == -1, (name, "query", rq)
      rc = be.lib._crn_conv_fwd_bf3(*a["args"][:2], a["w"], *a["args"][2:], st)
    else:
      rq = be.lib._crn_conv_wgrad_bf3_plan(*a["args"], C.byref(out))
      assert rq == -1, (name, "query", rq)
      rc = be.lib._crn_conv_wgrad_bf3_boxes(*a["args"], st)
    assert rc == -1, (name, "launch", rc)
  t.cuda.synchronize()
  for (name, op, _), a in zip(rejections(), keep):
    assert bool((a["out"] == SENTINEL).all()), f"{name}: a rejected call wrote its output"


def test_rejected_call_keeps_the_arming_of_splitk_defer(be):
  """A caller arms crn_splitk_defer, the split-bf16 entry rejects the shape, the caller falls back to the fp32 engine: that call
  must still find the arming (crn_conv_fwd_bf3 used to consume it before its rejections).  Seen from outside: the dense output
  of the armed fp32 split launch is untouched until another entry of the library flushes the pending sum."""
  from corenet_amd import _lib
  b32 = K32.build(K32.BY_NAME["s_auto_b"])                   # fp32 table: splits its channels, dense y, no accumulation
  y_ref = K32.run_fwd(be, b32, DEV)
  name, op, mk = [r for r in rejections() if r[0] == "fwd: window planes of 9 taps"][0]
  a = mk(DEV)
  other = t.ones(8, device=DEV)
  be.splitk_defer(True)
  assert be.lib._crn_conv_fwd_bf3(*a["args"][:2], a["w"], *a["args"][2:], _lib.stream()) == -1
  y = K32.run_fwd(be, b32, DEV)
  t.cuda.synchronize()
  pending = float((y - SENTINEL).abs().max()) == 0.0
  be.zero(other)
  assert t.equal(y.view(t.int32), y_ref.view(t.int32))
  assert pending, "the rejected call consumed the arming: the fp32 fall-back reduced its sum at once"
