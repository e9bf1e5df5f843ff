"""The encoder convolution engine (csrc/conv_e2d.hip: crn_conv2d_bf3, crn_conv_wgrad_2d_bf3, crn_bf3_operands) on the GPU, every row
of tests/conv_e2d_cases.py against a float64 reference: torch's conv3d on the case's inputs as doubles, the fused transform applied
in float64, autograd in float64 for the gradients.  Two bars per row: the project's 2e-5 of max|reference| against float64
(tests/test_conv_e2d_plan_cpu.py shows that the operand split itself takes at most half of it and which kernel bugs miss it by 10x
or more), and SPLIT_BAR against the split model -- the same products summed in float64 -- from which only the order of the float32
sums separates the kernel.  Every output buffer starts at a sentinel or at random contents; whatever the output view does not
address must come back bit-identical.  Which kernel ran is asked of the plan query on the very views of the launch."""
import ctypes as C
import functools
import os
import time

import pytest
import torch as t

import conv_e2d_cases as K
import conv_fp32_cases as K32
from conv_e2d_cases import CASES, BAR, SPLIT_BAR, SENTINEL, rejections

pytestmark = pytest.mark.gpu

DEV = "cuda"
_DET_ENV = os.environ.get("CRN_DETERMINISTIC", "0") == "1"
FWD = [c.name for c in CASES if c.op == "fwd"]
WGRAD = [c.name for c in CASES if c.op == "wgrad"]
MAXERR = {}          # kernel family -> [largest error against float64, against the split model] in units of max|reference|


@pytest.fixture(scope="module")
def be():
  t0 = time.time()
  from corenet_amd.backend import HipBackend
  assert t.cuda.is_available(), "gpu tests need an MI355X"
  yield HipBackend()
  print("\nencoder conv engine, largest error per kernel family (of max|float64 reference|): against float64, against the split model")
  for fam in sorted(MAXERR):
    print(f"  {fam:28s} {MAXERR[fam][0]:.2e}  {MAXERR[fam][1]:.2e}")
  print(f"  module wall time {time.time() - t0:.1f} s")


@functools.lru_cache(maxsize=None)
def built(name):
  return K.build(K.BY_NAME[name])


@functools.lru_cache(maxsize=None)
def ref_of(name):
  return K.make_ref(built(name))


def _plan(be, b):
  """The plan of the case's launch on device storages, checked against the row."""
  c = b.case
  if c.op == "fwd":
    p = K.query_plan(be, b, b.xs.to(DEV), b.y0.to(DEV), b.wop.to(DEV))
  else:
    p = K.query_plan(be, b, b.xs.to(DEV), b.dys.to(DEV), dw=b.dw0.to(DEV))
  want = {k: v for k, v in c.expect.items() if not (_DET_ENV and c.op == "wgrad" and k in K.DET_FIELDS)}
  assert {k: p[k] for k in want} == want, f"{c.name}: on the device's views the plan is {p}"
  return p


def _family(p):
  if p["kernel"] in ("wg1", "wg3"): return f"wgrad {p['kernel']}" + (" split" if p["splits"] > 1 else "")
  return f"fwd {p['kernel']} mode {p['mode']}"


def _note(fam, e64, esp, name):
  m = MAXERR.setdefault(fam, [0.0, 0.0])
  m[0], m[1] = max(m[0], e64), max(m[1], esp)
  print(f"{name}: {fam}: {e64:.2e} of the range against float64 (bar {BAR:.0e}), {esp:.2e} against the split model (bar {SPLIT_BAR:.1e})")


@pytest.mark.parametrize("name", FWD)
def test_forward_case(be, name):
  b, r = built(name), ref_of(name)
  p = _plan(be, b)
  y = K.run_fwd(be, b, DEV)
  e64, esp, outside = r.check(b, y)
  _note(_family(p), e64, esp, name)
  assert outside, f"{name}: elements outside the output view changed"
  assert e64 <= BAR, f"{name}: {e64:.3e} of max|ref| > {BAR}"
  assert esp <= SPLIT_BAR, f"{name}: {esp:.3e} of max|ref| from the split model > {SPLIT_BAR}"
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
    _note(_family(p), e64, esp, name)
    assert pad_ok, f"{name}: columns dy->C .. Npad are not what the contract says (zero after zero_first, untouched otherwise)"
    assert e64 <= BAR, f"{name}: {e64:.3e} of max|ref| > {BAR}"
    assert esp <= SPLIT_BAR, f"{name}: {esp:.3e} of max|ref| from the split model > {SPLIT_BAR}"
    if c.deterministic:                       # one workgroup per dw element, a fixed order: the same bits again
      assert p["splits"] == 1
      assert t.equal(K.run_wgrad(be, b, DEV).view(t.int32), dw.view(t.int32))
  finally:
    if c.deterministic: be.set_deterministic(_DET_ENV)


def test_wgrad_writes_nothing_behind_dw(be):
  """Rows of the last row tile past C (and columns of the last column tile past N) are computed and must not be stored: dw sits in
  a larger buffer full of SENTINEL, behind and in front."""
  for name in ("g1_c67_n12_k1", "g1_c35_n40_k5", "g3_4x8_c5_k1", "g3_8x8_c11"):
    b = built(name)
    c = b.case
    n, guard = b.dw0.numel(), 64 * 9 * b.npad
    buf = t.full((n + 2 * guard,), SENTINEL, device=DEV)
    dw = buf[guard:guard + n]
    be.conv_wgrad(K.xview(b, b.xs.to(DEV)), K.transform_of(b, DEV), K.yview(b, b.dys.to(DEV)), dw, b.npad, b.window, b.pad_lo,
                  True, math="bf16x3_2d")
    t.cuda.synchronize()
    assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + n:] == SENTINEL).all()), name
    assert not bool((dw == SENTINEL).any()), name


def test_operand_table(be):
  """crn_bf3_operands over five layers in one launch (encoder order at Npad 16 / 48 with 9 taps / 64 / 128, slab order), out of
  size order in the table and in the output: bit-identical to the contract emulator, the bytes behind the last entry untouched."""
  packed, desc, blocks, nbytes = K.operand_layers()
  want = t.full((nbytes + K.OPERAND_SLACK,), K.OPERAND_SENTINEL, dtype=t.uint8)
  K._EMU.bf3_operands(packed, (t.as_tensor(desc), blocks), want)
  got = t.full((nbytes + K.OPERAND_SLACK,), K.OPERAND_SENTINEL, dtype=t.uint8, device=DEV)
  be.bf3_operands(packed.to(DEV), (t.as_tensor(desc).to(DEV), blocks), got)
  got = got.cpu()
  assert bool((got[nbytes:] == K.OPERAND_SENTINEL).all()), "bytes behind the last entry were written"
  assert t.equal(got, want)


def _launch(be, op, a):
  from corenet_amd import _lib
  fn = be.lib._crn_conv2d_bf3 if op == "fwd" else be.lib._crn_conv_wgrad_2d_bf3
  return fn(*a["args"], _lib.stream())


def test_rejected_calls_write_nothing(be):
  """Every rejection of the two entries (the list of tests/test_conv_e2d_plan_cpu.py, built from the code): the plan query and the
  launch both return CRN_EINVAL on the device's views, and y / dw keep their sentinel -- the zero_first memset of the weight gradient
  included.  The query-only rows (views far larger than their storage) are not launched."""
  from corenet_amd import _lib
  out = _lib.CrnE2dPlan()
  keep = []
  for name, op, mk, launch in rejections():
    a = mk(DEV)
    keep.append(a)
    q = be.lib._crn_conv2d_bf3_plan if op == "fwd" else be.lib._crn_conv_wgrad_2d_bf3_plan
    assert q(*a["args"], C.byref(out)) == -1, (name, "query")
    if launch:
      assert _launch(be, op, a) == -1, (name, "launch")
  t.cuda.synchronize()
  for (name, op, _, _), a in zip(rejections(), keep):
    assert bool((a["out"] == SENTINEL).all()), f"{name}: a rejected call wrote its output"


def test_rejected_call_keeps_the_arming_of_splitk_defer(be):
  """A caller arms crn_splitk_defer, the encoder engine rejects the shape (a 14 x 16 map: H is no multiple of the tile height, one of
  the rejections that used to sit behind crn_splitk_begin), the caller falls back to the fp32 engine: that call must still find the
  arming.  Seen from outside: the dense output of the armed fp32 split launch is untouched until another entry of the library
  flushes the pending sum."""
  b32 = K32.build(K32.BY_NAME["s_auto_b"])                   # fp32 table: splits its channels, dense y, no accumulation
  y_ref = K32.run_fwd(be, b32, DEV)
  name, op, mk, _ = [r for r in rejections() if r[0] == "fwd: 3x3 on 14 x 16: H % 4"][0]
  a = mk(DEV)
  other = t.ones(8, device=DEV)
  be.splitk_defer(True)
  assert _launch(be, op, a) == -1
  y = K32.run_fwd(be, b32, DEV)
  t.cuda.synchronize()
  pending = float((y - SENTINEL).abs().max()) == 0.0
  be.zero(other)
  assert t.equal(y.view(t.int32), y_ref.view(t.int32))
  assert pending, "the rejected call consumed the arming: the fp32 fall-back reduced its sum at once"
