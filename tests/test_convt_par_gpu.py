"""The parity-walk kernels of decoder stage_6.t1 (csrc/convt_par.hip: crn_convt_s2k7_{fwd,dgrad,c2_fwd,c2_dgrad,wgrad}_bf3 and
crn_convt_s2k7_ximage) on the GPU, every row of tests/convt_par_cases.py against a float64 reference: torch's conv_transpose3d on
T(x) as doubles, its adjoint, autograd in float64 for the weight gradient.  Two bars per row: the project's 2e-5 of max|reference|
against float64 (tests/test_convt_par_model_cpu.py shows that the operand split itself takes less than half of it and that eight
kernel bugs miss it by 10x or more), and SPLIT_BAR against the walk model -- the same products summed in float64 -- from which only
the order of the float32 sums separates the kernel.  Inputs hold NaN wherever their view does not reach, outputs start at a sentinel
or at random contents: no NaN may appear, and whatever the output view does not address must come back bit-identical.  The weight
images are gathered on the GPU and must equal the contract emulator's bit for bit."""
import functools
import os
import time

import pytest
import torch as t

import convt_par_cases as K
from convt_par_cases import CASES, BAR, SPLIT_BAR

pytestmark = pytest.mark.gpu

DEV = "cuda"
_DET_ENV = os.environ.get("CRN_DETERMINISTIC", "0") == "1"
names = lambda op, det=False: [c.name for c in CASES if c.op == op and c.deterministic == det]
MAXERR = {}          # kernel family -> [largest error against float64, against the walk model] in units of max|reference|
PAIR_CLASS = ("36-tap pair", "48-tap pairs", "64-tap pair")


@pytest.fixture(scope="module")
def be():
  t0 = time.time()
  from corenet_amd.backend import HipBackend
  assert t.cuda.is_available(), "gpu tests need an MI355X"
  yield HipBackend()
  print("\nparity-walk kernels, largest error per kernel family (of max|float64 reference|): against float64, against the walk model")
  for fam in sorted(MAXERR):
    print(f"  {fam:36s} {MAXERR[fam][0]:.2e}  {MAXERR[fam][1]:.2e}")
  print(f"  module wall time {time.time() - t0:.1f} s")


@functools.lru_cache(maxsize=None)
def built(name):
  return K.build(K.BY_NAME[name])


@functools.lru_cache(maxsize=None)
def ref_of(name):
  return K.Ref(built(name))


def _note(fam, e64, esp, name):
  m = MAXERR.setdefault(fam, [0.0, 0.0])
  m[0], m[1] = max(m[0], e64), max(m[1], esp)
  print(f"{name}: {fam}: {e64:.2e} of the range against float64 (bar {BAR:.0e}), {esp:.2e} against the walk model (bar {SPLIT_BAR:.1e})")


def _image(be, b, r):
  """The row's weight image gathered on the GPU from the parameter slab: bit-equal to the contract emulator's."""
  img = t.zeros(r.img.numel(), dtype=t.uint8, device=DEV)
  be.bf3_gather_image(b.params.to(DEV), t.as_tensor(r.tab).to(DEV), img)
  assert t.equal(img.cpu(), r.img), f"{b.case.name}: the weight image differs from the emulator's"
  return img


def _fwd_or_dgrad(be, name):
  b, r = built(name), ref_of(name)
  c = b.case
  img = _image(be, b, r)
  out = (K.run_fwd if c.op == "fwd" else K.run_dgrad)(be, b, DEV, img)
  e64, esp, nan_free, outside = r.check(b, out)
  _note(("resident " if c.resident else "walk ") + c.op, e64, esp, name)
  assert nan_free, f"{name}: a NaN from outside the input views reached the output"
  assert outside, f"{name}: elements outside the output view changed"
  assert e64 <= BAR, f"{name}: {e64:.3e} of max|ref| > {BAR}"
  assert esp <= SPLIT_BAR, f"{name}: {esp:.3e} of max|ref| from the walk model > {SPLIT_BAR}"


@pytest.mark.parametrize("name", names("fwd"))
def test_forward_case(be, name):
  _fwd_or_dgrad(be, name)


@pytest.mark.parametrize("name", names("dgrad"))
def test_dgrad_case(be, name):
  _fwd_or_dgrad(be, name)


@pytest.mark.parametrize("name", names("wgrad"))
def test_wgrad_case(be, name):
  b, r = built(name), ref_of(name)
  c = b.case
  if _DET_ENV: be.set_deterministic(False)          # (the rows here are about the kernel; g_det is the deterministic one)
  try:
    dw = K.run_wgrad(be, b, DEV)
  finally:
    if _DET_ENV: be.set_deterministic(True)
  e64, emod, nan_free, rest_ok = r.check_wgrad(b, dw)
  for k, e in emod.items():
    _note(f"wgrad {PAIR_CLASS[k]}, T(x) {c.ximg}", e64, e, name)
  assert nan_free, f"{name}: a NaN from outside the input views reached the gradient"
  assert rest_ok, f"{name}: entries that hold no tap (columns past 8 cout included) are not what the contract says"
  assert e64 <= BAR, f"{name}: {e64:.3e} of max|ref| > {BAR}"
  assert max(emod.values()) <= SPLIT_BAR, f"{name}: {max(emod.values()):.3e} of max|ref| from the walk model > {SPLIT_BAR}"


@pytest.mark.parametrize("name", names("wgrad", det=True))
def test_wgrad_steps_aside_in_deterministic_mode(be, name):
  """The entry returns CRN_EINVAL and writes nothing; conv_wgrad(math="ct_par") then lands on the generic split-bf16 engine, within
  the same bars."""
  b, r = built(name), ref_of(name)
  be.set_deterministic(True)
  try:
    dw = K.run_wgrad(be, b, DEV, want_rc=-1)
    assert t.equal(dw.cpu().view(t.int32), b.dw0.view(t.int32)), f"{name}: the rejected call wrote"
    dw = K.run_wgrad_dispatch(be, b, DEV)
  finally:
    be.set_deterministic(_DET_ENV)
  e64, emod, nan_free, rest_ok = r.check_wgrad(b, dw, real_only=True)
  _note("wgrad deterministic (generic engine)", e64, max(emod.values()), name)
  assert nan_free and rest_ok, name
  assert e64 <= BAR, f"{name}: {e64:.3e} of max|ref| > {BAR}"
  assert max(emod.values()) <= SPLIT_BAR, f"{name}: {max(emod.values()):.3e} of max|ref| from the walk model > {SPLIT_BAR}"


@pytest.mark.parametrize("name", names("ximage"))
def test_ximage_case(be, name):
  """The operand image bit for bit: bf16 hi / lo of the float32 T(x); the bytes behind crn_convt_s2k7_ximage_bytes untouched."""
  b = built(name)
  img, nb = K.run_ximage(be, b, DEV)
  img = img.cpu()
  want = K.ref_ximage(b)
  assert nb == want.numel() * 2
  assert t.equal(img[:nb].view(t.int16).view(want.shape), want), f"{name}: the operand image differs from bf16 hi / lo of T(x)"
  assert bool((img[nb:] == 0xA5).all()), f"{name}: bytes behind the image were written"
