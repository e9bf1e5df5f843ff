"""GPU tests of csrc/batch_renorm.hip: every kernel its host code can choose -- the five register instantiations of the
channel-owner form, the owner form that is not register-resident, the two-pass form at 3, 4, 8, 32 and 64 slices, the
big_dec switch, the scalar fall-backs behind vec_ok, crn_batch_renorm_finalize on both sides of its narrow / wide switch,
eval mode, the deterministic sum(dx), the take-over of a pending split-K sum, and the two elementwise block-tail kernels --
against float64 references written here.

The forward reference is the header contract of include/corenet_hip.h (and oracle.corenet_oracle.batch_renorm) on the
float32 inputs cast to float64; the backward reference is the header's formula in float64 on the float32 scale / shift /
saved of the FORWARD REFERENCE (never of the statistics kernel: a backward failure points at the backward kernel).
Tolerances are the project's: 2e-5 of max-abs-err / max-abs-reference, |dsum - ref| <= 2e-5 * max_c sum|dx|, copies,
masks and sentinels bit-exact, the elementwise kernels 1e-6 of range.

The post-ReLU mask x' * scale + shift > 0 is discontinuous: every post_relu input is built so that no element of the
float64 y lies within 1e-4 * max|y| of zero (asserted on the host before any GPU call), so the float32 FMA and the float64
reference agree on every element and none is left out of a comparison.

CRN_TEST_SELFCHECK=1 runs the same assertions against the contract emulator on a CPU (error returns, alignment cases,
the route probe, bit-for-bit comparisons of two kernels and the split-K tests are then left out)."""
import os

import numpy as np
import pytest
import torch as t

from oracle import corenet_oracle as O
from kernel_contract_emu import EmuBackend

pytestmark = pytest.mark.gpu

_SELF = os.environ.get("CRN_TEST_SELFCHECK") == "1"
DEV = "cpu" if _SELF else "cuda"

EPS = float(np.float32(1e-3))       # the kernels take eps and momentum as float32
MOM = float(np.float32(0.1))        # (0.1: a second update of the running statistics is far outside the tolerance)
TOL = 2e-5
SENT = -7.0
_DET0 = os.environ.get("CRN_DETERMINISTIC", "0") not in ("", "0")       # the library's mode outside the tests that switch it


@pytest.fixture(scope="module")
def be():
  if _SELF:
    return EmuBackend()
  from corenet_amd.backend import HipBackend
  assert t.cuda.is_available(), "gpu tests need an MI355X"
  return HipBackend()


def _hip_error():
  from corenet_amd._lib import HipError
  return HipError


def _sync():
  if not _SELF:
    t.cuda.synchronize()


def dev(x):
  """A copy on the device under test, for a tensor the call writes (under the emulator .to() alone would alias it)."""
  return x.clone().to(DEV)


def close(a, b, rtol, name=""):
  a = a.detach().cpu().double(); b = b.detach().cpu().double()
  den = float(b.abs().max()) + 1e-30
  err = float((a - b).abs().max()) / den
  assert err <= rtol, f"{name}: max-abs-err/max = {err:.3e} > {rtol}"
  return err


def exact(a, want, name=""):
  """a (device) equals the reference cast to its dtype, bit for bit."""
  assert t.equal(a.detach().cpu(), want.cpu().to(a.dtype)), name


def all_sentinel(a, name=""):
  a = a.detach().cpu()
  assert bool((a == SENT).all()), f"{name}: sentinel overwritten"


# ------------------------------------------------------------------ float64 references
def sched(nbt):
  """r_max, 1 / r_max, d_max in float32 arithmetic from num_batches_tracked (batch_renorm.py:41-42, bn_finalize_channel)."""
  nt = t.tensor([nbt], dtype=t.int64).to(t.float32)
  d_max = (5.0 * (nt - 5000.0) / (25000.0 - 5000.0)).clamp(0.0, 5.0)
  r_max = 1.0 + (2.0 * (nt - 5000.0) / (40000.0 - 5000.0)).clamp(0.0, 2.0)
  assert d_max.dtype == t.float32 and r_max.dtype == t.float32
  return float(r_max), float(1.0 / r_max), float(d_max)


def finalize_ref(mean, var, C, gamma, beta, rm, rv, nbt):
  """float64 mean / biased variance [C] -> dict of float64 scale, shift, saved [4, C], running_mean, running_var and the
  raw (unclamped) r, d."""
  g, bt, rm, rv = gamma.double(), beta.double(), rm.double(), rv.double()
  r_max, r_min, d_max = sched(nbt)
  b_std = (var + EPS).sqrt(); run_std = (rv + EPS).sqrt()
  r_raw = b_std / run_std; d_raw = (mean - rm) / run_std
  r = r_raw.clamp(r_min, r_max); d = d_raw.clamp(-d_max, d_max)
  rstd = 1.0 / b_std
  unbiased = var * C / t.tensor(float(C - 1), dtype=t.float64)          # (C = 1: inf / nan, as the reference project)
  return dict(scale=g * r * rstd, shift=bt + g * (d - mean * r * rstd), saved=t.stack([mean, rstd, r, d]),
              running_mean=rm + MOM * (mean - rm), running_var=rv + MOM * (unbiased - rv), r_raw=r_raw, d_raw=d_raw,
              r_lim=(r_min, r_max), d_max=d_max)


def fwd_ref(x, pre, gamma, beta, rm, rv, nbt):
  """x: float32 [B, C, S]."""
  v = x.double()
  if pre: v = v.clamp(min=0)
  mean = v.mean((0, 2))
  var = ((v - mean.view(1, -1, 1)) ** 2).mean((0, 2))
  return finalize_ref(mean, var, x.shape[1], gamma, beta, rm, rv, nbt)


def out_ref(x, pre, scale32, shift32):
  """y = x' * scale + shift in float64 on the float32 scale / shift."""
  v = x.double()
  if pre: v = v.clamp(min=0)
  return v * scale32.double().view(1, -1, 1) + shift32.double().view(1, -1, 1)


def bwd_ref(x, dy, pre, post, gamma, scale32, shift32, saved32):
  """The backward formula of include/corenet_hip.h in float64 -> dx [B, C, S], dgamma, dbeta, dsum [C]."""
  B, C, S = x.shape
  xd = x.double()
  v = xd.clamp(min=0) if pre else xd
  mu, rstd, r, d = [u.double().view(1, C, 1) for u in saved32.view(4, C)]
  g = dy.double()
  if post:
    g = g * (out_ref(x, pre, scale32, shift32) > 0)
  xn = (v - mu) * rstd
  s1 = g.sum((0, 2)); s2 = (g * xn).sum((0, 2))
  n = float(B * S)
  dx = gamma.double().view(1, C, 1) * r * rstd * (g - (s1 / n).view(1, C, 1) - xn * (s2 / n).view(1, C, 1))
  if pre:
    dx = dx * (xd > 0)
  return dict(dx=dx, dgamma=r.view(-1) * s2 + d.view(-1) * s1, dbeta=s1, dsum=dx.sum((0, 2)))


def f32(ref):
  return {k: v.to(t.float32) for k, v in ref.items() if k in ("scale", "shift", "saved", "running_mean", "running_var")}


MASK_MARGIN = 1e-4


def mask_margin(x, pre, scale32, shift32):
  """min |y| / max |y| of the float64 y."""
  y = out_ref(x, pre, scale32, shift32).abs()
  return float(y.min()) / float(y.max())


def clear_of_mask(x, pre, gamma, beta, rm, rv, nbt):
  """Moves the elements of x whose float64 y = x' * scale + shift lies within MASK_MARGIN * max|y| of zero away from the
  crossing (the statistics move with them, hence the rounds: at most 8); asserts the margin holds on return."""
  x = x.clone()
  for _ in range(8):
    ref = f32(fwd_ref(x, pre, gamma, beta, rm, rv, nbt))
    y = out_ref(x, pre, ref["scale"], ref["shift"])
    lim = MASK_MARGIN * float(y.abs().max())
    bad = y.abs() < lim
    if not bool(bad.any()):
      break
    sgn = t.where(y >= 0, 1.0, -1.0).double()
    step = sgn * (3.0 * lim) / ref["scale"].double().view(1, -1, 1)       # y moves by 3 * lim away from zero
    x = t.where(bad, (x.double() + step).to(t.float32), x)
  ref = f32(fwd_ref(x, pre, gamma, beta, rm, rv, nbt))
  assert mask_margin(x, pre, ref["scale"], ref["shift"]) >= MASK_MARGIN, "post-ReLU mask margin not reached in 8 rounds"
  return x


# ------------------------------------------------------------------ the dispatch, as csrc/batch_renorm.hip words it
def owner_form(B, C, S):
  return C >= 64 and B * S <= 65536 and (B * S <= 16384 or C >= 256)


def stats_two_pass(B, C, S):
  return not owner_form(B, C, S)


def bwd_two_pass(B, C, S, pre):
  return not (owner_form(B, C, S) and not (pre and B * S > 8192))


def nsplit_for(S, C, B):
  return min(max(1, 2048 // max(1, C * B)), max(1, S // 4096), 64)


class Probe:
  """Did the call go through the two-pass kernels?  Their first pass leaves partial sums at the head of the BatchRenorm
  workspace; the owner kernels never touch it."""

  def __init__(self, be, C):
    self.ws = None if _SELF else be._bn_ws(C, t.empty(0, device=DEV).device)[0]
    if self.ws is not None:
      self.ws[:16].fill_(0xFF)

  def two_pass(self):
    return bool((self.ws[:16].cpu() != 0xFF).any())

  def check(self, want, name):
    if self.ws is not None:
      _sync()
      assert self.two_pass() == want, f"{name}: expected the {'two-pass' if want else 'channel-owner'} form"


# ------------------------------------------------------------------ one shape through statistics and backward
def make_case(B, C, S, pre, post, nbt=12000, seed=0, x=None, plant=True):
  g = t.Generator().manual_seed(1000 * B + 7 * C + S + seed)
  if x is None:
    x = t.randn(B, C, S, generator=g) * 2 + 0.4
  if plant and S >= 3:                  # the `> 0` side of the input masks: exact zeros of both signs
    x[:, :, 0] = 0.0; x[:, :, 1] = -0.0; x[-1, :, S - 1] = 0.0
  gamma = t.rand(C, generator=g) + 0.5; beta = t.randn(C, generator=g)
  rm = t.randn(C, generator=g); rv = t.rand(C, generator=g) * 3 + 0.1
  dy = t.randn(B, C, S, generator=g)
  if post:
    x = clear_of_mask(x, pre, gamma, beta, rm, rv, nbt)
  return dict(B=B, C=C, S=S, pre=pre, post=post, nbt=nbt, x=x, dy=dy, gamma=gamma, beta=beta, rm=rm, rv=rv, g=g)


def wide(x, lead=1, extra=2, fill=SENT):
  """x [B, C, S] as the channel slice [lead, lead + C) of a device buffer `extra` channels wider -> (buffer, slice, batch stride)."""
  B, C, S = x.shape
  buf = t.full((B, C + extra, S), fill, dtype=x.dtype)
  buf[:, lead:lead + C] = x
  buf = buf.to(DEV) if not _SELF else buf
  return buf, buf[:, lead:lead + C], (C + extra) * S


def neighbours_untouched(buf, C, name, lead=1):
  all_sentinel(buf[:, :lead], name + " channel before"); all_sentinel(buf[:, lead + C:], name + " channels after")


def run_stats(be, cs, name, xs=None, sB=None, check_route=True):
  B, C, S, pre = cs["B"], cs["C"], cs["S"], cs["pre"]
  ref = fwd_ref(cs["x"], pre, cs["gamma"], cs["beta"], cs["rm"], cs["rv"], cs["nbt"])
  once = ref["running_mean"]                       # "updated exactly once": a second update would be far outside the tolerance
  assert float((MOM * (ref["saved"][0] - once)).abs().max()) > 10 * TOL * float(once.abs().max())
  if xs is None:
    xbuf, xs, sB = wide(cs["x"])
  rm, rv = dev(cs["rm"]), dev(cs["rv"])
  sc, sh, sv = [t.full((n,), SENT, device=DEV) for n in (C, C, 4 * C)]
  probe = Probe(be, C)
  be.bn_stats(xs, B, C, S, sB, pre, cs["gamma"].to(DEV), cs["beta"].to(DEV), rm, rv,
              t.tensor([cs["nbt"]], dtype=t.int64).to(DEV), EPS, MOM, True, sc, sh, sv)
  if check_route:
    probe.check(stats_two_pass(B, C, S), name + " stats")
  errs = {}
  for nm, got in (("scale", sc), ("shift", sh), ("running_mean", rm), ("running_var", rv)):
    errs[nm] = close(got, ref[nm], TOL, f"{name} {nm}")
  for i, nm in enumerate(("mu", "rstd", "r", "d")):
    errs[nm] = close(sv.view(4, C)[i], ref["saved"][i], TOL, f"{name} saved {nm}")
  print(f"[batch_renorm] {name} stats ({'two-pass' if stats_two_pass(B, C, S) else 'owner'}): " +
        " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
  return ref


def run_bwd(be, cs, name, ref=None, xs=None, sB_x=None, dy_dev=None, sB_dy=None, dx_pair=None, check_route=True):
  """bn_bwd twice (accumulate off, then on) on the float32 scale / shift / saved of the forward reference."""
  B, C, S, pre, post = cs["B"], cs["C"], cs["S"], cs["pre"], cs["post"]
  if ref is None:
    ref = fwd_ref(cs["x"], pre, cs["gamma"], cs["beta"], cs["rm"], cs["rv"], cs["nbt"])
  r32 = f32(ref)
  if post:
    assert mask_margin(cs["x"], pre, r32["scale"], r32["shift"]) >= MASK_MARGIN
  want = bwd_ref(cs["x"], cs["dy"], pre, post, cs["gamma"], r32["scale"], r32["shift"], r32["saved"])
  if xs is None:
    xbuf, xs, sB_x = wide(cs["x"])
  if dy_dev is None:
    dy_dev, sB_dy = cs["dy"].to(DEV), C * S
  gm, sc, sh, sv = [v.to(DEV) for v in (cs["gamma"], r32["scale"], r32["shift"], r32["saved"].reshape(-1))]
  nds = max(1, C - 2)
  dsum_bar = TOL * (float(want["dx"].abs().sum((0, 2)).max()) + 1e-30)
  dg0 = t.randn(C, generator=cs["g"]) * 10; db0 = t.randn(C, generator=cs["g"]) * 10
  for acc in (False, True):
    if dx_pair is None:
      dxbuf, dxs, sB_dx = wide(t.full((B, C, S), SENT))
    else:
      dxbuf, dxs, sB_dx = dx_pair()
    dg, db = (dev(dg0), dev(db0)) if acc else (t.full((C,), SENT, device=DEV), t.full((C,), SENT, device=DEV))
    ds = t.full((C,), SENT, device=DEV)
    probe = Probe(be, C)
    be.bn_bwd(xs, sB_x, dy_dev, sB_dy, B, C, S, pre, post, gm, sc, sh, sv, dxs, sB_dx, dg, db, acc, ds, nds)
    if check_route:
      probe.check(bwd_two_pass(B, C, S, pre), name + " backward")
    e = {"dx": close(dxs, want["dx"], TOL, f"{name} dx (accumulate={acc})"),
         "dgamma": close(dg, want["dgamma"] + (dg0.double() if acc else 0), TOL, f"{name} dgamma (accumulate={acc})"),
         "dbeta": close(db, want["dbeta"] + (db0.double() if acc else 0), TOL, f"{name} dbeta (accumulate={acc})")}
    dse = float((ds.cpu().double()[:nds] - want["dsum"][:nds]).abs().max())
    assert dse <= dsum_bar, f"{name} dsum (accumulate={acc}): {dse:.3e} > {dsum_bar:.3e}"
    e["dsum/bar"] = dse / dsum_bar
    all_sentinel(ds[nds:], name + " dsum tail")
    if dx_pair is None:
      neighbours_untouched(dxbuf, C, name + " dx")
    print(f"[batch_renorm] {name} backward ({'two-pass' if bwd_two_pass(B, C, S, pre) else 'owner'}, accumulate={int(acc)}): " +
          " ".join(f"{k} {v:.1e}" for k, v in e.items()))
  return want


MODES = [(False, False), (True, False), (False, True)]
MODE_IDS = ["plain", "pre_relu", "post_relu"]

REG_SHAPES = [(1, 64, 1024), (3, 64, 344), (2, 64, 1024), (3, 65, 1028), (2, 64, 4096), (5, 64, 1028), (1, 64, 16384),
              (3, 64, 4100)]
OWNER_SHAPES = [(1, 256, 16388), (17, 256, 964), (1, 256, 16387), (4, 256, 16384), (1, 256, 65540), (1, 64, 16388)]
# (32, 2, 131072): 32 slices x 32 samples = 1024 parts per channel, every part loop takes many trips
TWO_PASS_SHAPES = [(1, 2, 12293), (2, 3, 12296), (1, 2, 262148), (32, 2, 131072)]


def _ids(shapes):
  return ["x".join(map(str, s)) for s in shapes]


def test_shape_tables_reach_their_paths():
  """The shapes above reach the kernels they are there for (the host code of csrc/batch_renorm.hip, restated)."""
  per = lambda B, C, S: -(-(B * S // 4) // 256)
  assert [per(*s) for s in REG_SHAPES] == [1, 2, 2, 4, 8, 6, 16, 13]
  for B, C, S in REG_SHAPES:
    assert owner_form(B, C, S) and B * S <= 16384 and S % 4 == 0
  assert [bwd_two_pass(B, C, S, True) for B, C, S in REG_SHAPES] == [False] * 6 + [True, True]        # big_dec
  assert not any(bwd_two_pass(B, C, S, False) for B, C, S in REG_SHAPES)
  assert [owner_form(*s) for s in OWNER_SHAPES] == [True, True, True, True, False, False]
  assert all(B * S > 16384 for B, C, S in OWNER_SHAPES)
  assert nsplit_for(65540, 256, 1) == 8 and nsplit_for(16388, 64, 1) == 4
  assert [nsplit_for(S, C, B) for B, C, S in TWO_PASS_SHAPES] == [3, 3, 64, 32]
  assert not any(owner_form(*s) for s in TWO_PASS_SHAPES)


@pytest.mark.parametrize("pre,post", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("B,C,S", REG_SHAPES, ids=_ids(REG_SHAPES))
def test_register_form(be, B, C, S, pre, post):
  """bn_owner_stats_reg_kernel / bn_owner_bwd_reg_kernel at NV = 1, 2, 4, 8, 16, full and ragged; from 8192 elements per
  channel on a pre-ReLU backward takes the two-pass kernels instead (big_dec) and matches the same reference."""
  cs = make_case(B, C, S, pre, post)
  name = f"reg {B}x{C}x{S} {MODE_IDS[MODES.index((pre, post))]}"
  ref = run_stats(be, cs, name)
  run_bwd(be, cs, name, ref)


@pytest.mark.parametrize("pre,post", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("B,C,S", OWNER_SHAPES, ids=_ids(OWNER_SHAPES))
def test_owner_form(be, B, C, S, pre, post):
  """bn_owner_stats_kernel / bn_owner_bwd_kernel, vectorised and scalar, at both ends of 16384 < B*S <= 65536, and the
  two shapes just outside (too large; too few channels), which fall to the two-pass kernels."""
  cs = make_case(B, C, S, pre, post)
  name = f"owner {B}x{C}x{S} {MODE_IDS[MODES.index((pre, post))]}"
  ref = run_stats(be, cs, name)
  run_bwd(be, cs, name, ref)


@pytest.mark.parametrize("pre,post", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("B,C,S", TWO_PASS_SHAPES, ids=_ids(TWO_PASS_SHAPES))
def test_two_pass_form(be, B, C, S, pre, post):
  """bn_partial / bn_finalize / bn_bwd_partial / bn_bwd_apply with 3 slices (scalar with a ragged last slice; vectorised
  with the slice length rounded up to 4), at the 64-slice cap, and with 1024 parts per channel."""
  cs = make_case(B, C, S, pre, post)
  name = f"two-pass {B}x{C}x{S} {MODE_IDS[MODES.index((pre, post))]}"
  ref = run_stats(be, cs, name)
  run_bwd(be, cs, name, ref)


# ------------------------------------------------------------------ vec_ok fall-backs with S % 4 == 0
def off_by_one_float(x):
  """x [B, C, S] dense at a device address 4 bytes off 16-byte alignment -> (tensor, batch stride)."""
  B, C, S = x.shape
  buf = t.full((B * C * S + 4,), SENT, dtype=x.dtype).to(DEV)
  v = buf[1:1 + B * C * S].view(B, C, S)
  v.copy_(x)
  if not _SELF:
    assert v.data_ptr() % 16 == 4
  return buf, v, C * S


def odd_batch_stride(x):
  """x [B, C, S] with a batch stride that is 2 mod 4 (16-byte aligned base) -> (tensor, batch stride)."""
  B, C, S = x.shape
  sB = C * S + 2
  buf = t.full((B, sB), SENT, dtype=x.dtype).to(DEV)
  v = buf[:, :C * S].view(B, C, S)
  v.copy_(x)
  assert sB % 4 == 2
  return buf, v, sB


LAYOUTS = {"base+4B": off_by_one_float, "sB=2mod4": odd_batch_stride}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("which", ["x", "dy", "dx"])
@pytest.mark.parametrize("pre,post", MODES, ids=MODE_IDS)
def test_scalar_fallbacks(be, which, layout, pre, post):
  """S % 4 == 0 but one tensor is not float4-addressable: the scalar kernels are chosen and give the reference's values;
  the padding between the samples stays untouched."""
  B, C, S = 2, 64, 256
  cs = make_case(B, C, S, pre, post, seed=3)
  name = f"scalar {which} {layout} {MODE_IDS[MODES.index((pre, post))]}"
  mk = LAYOUTS[layout]
  ref = None
  kw = {}
  if which == "x":
    xbuf, xs, sB = mk(cs["x"])
    ref = run_stats(be, cs, name, xs, sB)
    kw = dict(xs=xs, sB_x=sB)
  elif which == "dy":
    dbuf, dys, sB = mk(cs["dy"])
    kw = dict(dy_dev=dys, sB_dy=sB)
  bufs = []
  if which == "dx":
    def pair():
      buf, v, sB = mk(t.full((B, C, S), SENT))
      bufs.append(buf)
      return buf, v, sB
    kw = dict(dx_pair=pair)
  run_bwd(be, cs, name, ref, **kw)
  if which == "dx" and layout == "sB=2mod4":
    for buf in bufs:
      all_sentinel(buf[:, C * S:], name + " padding between samples")
  if which == "dx" and layout == "base+4B":
    for buf in bufs:
      all_sentinel(buf[:1], name); all_sentinel(buf[1 + B * C * S:], name)


# ------------------------------------------------------------------ elementwise references
def affine_ref(x, scale, shift, r, rscale, rshift):
  C = x.shape[1]
  one, zero = t.ones(C, dtype=t.float64), t.zeros(C, dtype=t.float64)
  v = lambda p, dflt: (p.double() if p is not None else dflt).view(1, C, 1)
  o = x.double() * v(scale, one) + v(shift, zero)
  if r is not None:
    o = o + r.double() * v(rscale, one) + v(rshift, zero)
  return o


def relu_bwd_ref(dy, act, dy2):
  o = t.zeros(act.shape, dtype=t.float64)
  if dy is not None:
    o = dy.double() * (act > 0)
  if dy2 is not None:
    o = o + dy2.double()
  return o


def _opt(x):
  return None if x is None else x.to(DEV)


def elementwise_inputs(B, C, S, seed):
  g = t.Generator().manual_seed(seed)
  x = t.randn(B, C, S, generator=g); r = t.randn(B, C, S, generator=g)
  for v in (x, r):
    v[:, :, 0] = 0.0; v[0, :, S - 1] = -0.0
  sc, sh, rsc, rsh = [t.randn(C, generator=g) for _ in range(4)]
  return x, r, sc, sh, rsc, rsh, g


@pytest.mark.parametrize("tensor", ["r", "y_pre", "y"])
def test_tail_with_one_misaligned_buffer(be, tensor):
  """crn_batch_renorm_stats_tail where only a tail-side buffer is 4 bytes off: the statistics still run in the register form
  and the tail falls to its own (scalar) launch; both against float64."""
  B, C, S = 2, 64, 256
  cs = make_case(B, C, S, False, False, seed=11)
  x, r, _, _, rsc, rsh, _ = elementwise_inputs(B, C, S, 12)
  ref = fwd_ref(cs["x"], False, cs["gamma"], cs["beta"], cs["rm"], cs["rv"], cs["nbt"])
  xg = cs["x"].to(DEV)
  rbuf, rg, _ = off_by_one_float(r) if tensor == "r" else (None, r.to(DEV), 0)
  pbuf, yp, _ = off_by_one_float(t.full((B, C, S), SENT)) if tensor == "y_pre" else (None, t.full((B, C, S), SENT, device=DEV), 0)
  ybuf, y, _ = off_by_one_float(t.full((B, C, S), SENT)) if tensor == "y" else (None, t.full((B, C, S), SENT, device=DEV), 0)
  rm, rv = dev(cs["rm"]), dev(cs["rv"])
  sc, sh, sv = [t.full((n,), SENT, device=DEV) for n in (C, C, 4 * C)]
  be.bn_stats_tail(xg, B, C, S, C * S, cs["gamma"].to(DEV), cs["beta"].to(DEV), rm, rv, t.tensor([cs["nbt"]], dtype=t.int64).to(DEV),
                   EPS, MOM, True, sc, sh, sv, rg, rsc.to(DEV), rsh.to(DEV), C * S, yp, C * S, y, C * S, True)
  for nm, got in (("scale", sc), ("shift", sh), ("running_mean", rm), ("running_var", rv)):
    close(got, ref[nm], TOL, f"tail {tensor} {nm}")
  close(sv.view(4, C), ref["saved"], TOL, f"tail {tensor} saved")
  # the tail on the scale / shift the call itself produced: one FMA against multiply-add is the only difference
  want = affine_ref(cs["x"], sc.cpu(), sh.cpu(), r, rsc, rsh)
  close(yp, want, 1e-6, f"tail {tensor} y_pre"); close(y, want.clamp(min=0), 1e-6, f"tail {tensor} y")
  exact(y, yp.cpu().clamp(min=0), f"tail {tensor} y = relu(y_pre)")
  for buf in (pbuf, ybuf):
    if buf is not None:
      all_sentinel(buf[:1]); all_sentinel(buf[1 + B * C * S:])


@pytest.mark.parametrize("tensor", ["g", "act", "g2"])
def test_head_with_one_misaligned_buffer(be, tensor):
  """crn_batch_renorm_bwd_head where only a head-side buffer is 4 bytes off: dy is formed by the scalar crn_relu_bwd_add
  launch (exact) and the norm's backward runs in the register form on it."""
  B, C, S = 2, 64, 256
  cs = make_case(B, C, S, False, False, seed=13)
  g = cs["g"]
  gg, act, g2 = t.randn(B, C, S, generator=g), t.randn(B, C, S, generator=g), t.randn(B, C, S, generator=g)
  act[:, :, 0] = 0.0; act[:, :, 1] = -0.0
  cs["dy"] = gg * (act > 0) + g2                          # float32, as the kernel forms and stores it
  r32 = f32(fwd_ref(cs["x"], False, cs["gamma"], cs["beta"], cs["rm"], cs["rv"], cs["nbt"]))
  want = bwd_ref(cs["x"], cs["dy"], False, False, cs["gamma"], r32["scale"], r32["shift"], r32["saved"])
  dv = {}
  for nm, v in (("g", gg), ("act", act), ("g2", g2)):
    dv[nm] = off_by_one_float(v)[1] if nm == tensor else v.to(DEV)
  dyg = t.full((B, C, S), SENT, device=DEV)
  dxbuf, dxs, sB_dx = wide(t.full((B, C, S), SENT))
  dg, db, ds = [t.full((C,), SENT, device=DEV) for _ in range(3)]
  be.bn_bwd_head(cs["x"].to(DEV), C * S, dyg, C * S, dv["g"], C * S, dv["act"], C * S, dv["g2"], C * S, B, C, S,
                 cs["gamma"].to(DEV), r32["scale"].to(DEV), r32["shift"].to(DEV), r32["saved"].reshape(-1).to(DEV),
                 dxs, sB_dx, dg, db, False, ds, C - 2)
  exact(dyg, cs["dy"], f"head {tensor} dy")
  close(dxs, want["dx"], TOL, f"head {tensor} dx"); close(dg, want["dgamma"], TOL, f"head {tensor} dgamma")
  close(db, want["dbeta"], TOL, f"head {tensor} dbeta")
  assert float((ds.cpu().double()[:C - 2] - want["dsum"][:C - 2]).abs().max()) <= TOL * float(want["dx"].abs().sum((0, 2)).max())
  all_sentinel(ds[C - 2:]); neighbours_untouched(dxbuf, C, f"head {tensor} dx")


# ------------------------------------------------------------------ numerics
@pytest.mark.parametrize("B,C,S", [(2, 64, 1024), (1, 256, 16388), (2, 3, 12296)], ids=["register", "owner", "two-pass"])
def test_large_offset_needs_float64_sums(be, B, C, S):
  """x = 300 + 0.05 * randn: sum(x^2) / n - mean^2 cancels seven digits, which float64 sums carry and float32 sums do not.
  num_batches_tracked = 0 (r = 1, d = 0): every compared quantity is then well conditioned in the float32 mean and
  variance the contract hands on."""
  g = t.Generator().manual_seed(S)
  x = 300.0 + 0.05 * t.randn(B, C, S, generator=g)
  cs = make_case(B, C, S, False, False, nbt=0, x=x, plant=False)
  cs["rm"] = 300.0 + t.randn(C, generator=g); cs["rv"] = t.rand(C, generator=g) * 0.01 + 0.001
  run_stats(be, cs, f"offset-300 {B}x{C}x{S}")


@pytest.mark.parametrize("B,C,S", [(2, 64, 1024), (2, 3, 12296)], ids=["register", "two-pass"])
def test_constant_and_all_negative_channels(be, B, C, S):
  """A constant channel has variance exactly 0 (the clamp at 0 applies: rstd = 1 / sqrt(eps)); an all-negative channel
  under pre_relu is the constant 0, and its dx is all zeros."""
  for pre in (False, True):
    cs = make_case(B, C, S, pre, False, seed=17, plant=False)
    cs["x"][:, 0] = 1.7
    cs["x"][:, 1] = -cs["x"][:, 1].abs() - 0.5 if pre else 0.1
    ref = run_stats(be, cs, f"constant {B}x{C}x{S} pre={int(pre)}")
    rstd0 = 1.0 / np.sqrt(EPS)
    assert abs(float(ref["saved"][1, 0]) - rstd0) <= 1e-6 * rstd0 and abs(float(ref["saved"][1, 1]) - rstd0) <= 1e-6 * rstd0
    want = run_bwd(be, cs, f"constant {B}x{C}x{S} pre={int(pre)}", ref)
    if pre:
      assert float(want["dx"][:, 1].abs().max()) == 0.0


NBTS = [0, 5000, 5001, 25000, 40000, 10 ** 7, 2 ** 40]


@pytest.mark.parametrize("nbt", NBTS)
def test_num_batches_tracked_schedule(be, nbt):
  """The r_max / d_max schedule at both ends of both ramps and far beyond, with running statistics that clamp r at both ends,
  d at both signs, and one channel where neither clamps."""
  B, C, S = 3, 8, 40
  cs = make_case(B, C, S, False, False, nbt=nbt, seed=nbt % 1000, plant=False)
  x = cs["x"]
  x[:, 4] -= x[:, 4].double().mean().float()                  # channel 4: mean ~ 0, so that d there is not at the mercy of
  v = x.double()                                              # the float32 rounding of the mean
  mean = v.mean((0, 2)); std = (((v - mean.view(1, -1, 1)) ** 2).mean((0, 2)) + EPS).sqrt()
  r_max, r_min, d_max = sched(nbt)
  ratio = t.tensor([0.1, 10.0, 0.2, 5.0, 1.0, 1.0, 4.0, 0.25], dtype=t.float64)      # b_std / running_std
  dval = t.tensor([-20.0, 20.0, 7.0, -7.0, 0.4 * d_max, 30.0, 0.0, -30.0], dtype=t.float64)
  run_std = std / ratio
  cs["rv"] = (run_std ** 2 - EPS).float()
  cs["rm"] = (mean - dval * run_std).float()
  ref = fwd_ref(x, False, cs["gamma"], cs["beta"], cs["rm"], cs["rv"], nbt)
  rr, dr = ref["r_raw"], ref["d_raw"]
  assert bool((rr < r_min).any()) and bool((rr > r_max).any()) and bool((dr < -d_max).any()) and bool((dr > d_max).any())
  if nbt > 5000:
    free = (rr > r_min) & (rr < r_max) & (dr > -d_max) & (dr < d_max) & (dr.abs() > 0.1 * d_max)
    assert bool(free[4]), "no channel with r and d both inside their clamps"
  want = {0: (1.0, 0.0), 5000: (1.0, 0.0), 25000: (1.0 + 2.0 * 20000 / 35000, 5.0), 40000: (3.0, 5.0), 10 ** 7: (3.0, 5.0),
          2 ** 40: (3.0, 5.0)}
  if nbt in want:
    assert abs(r_max - want[nbt][0]) < 1e-6 and d_max == want[nbt][1]
  run_stats(be, cs, f"nbt={nbt}")
  run_bwd(be, cs, f"nbt={nbt}", ref)


def test_one_channel_matches_the_oracle(be):
  """C = 1 divides by C - 1 as the reference project does: running_var turns inf (nan for a constant channel), scale and
  shift stay finite."""
  B, C, S = 2, 1, 50
  for const in (False, True):
    cs = make_case(B, C, S, False, False, seed=int(const), plant=False)
    if const:
      cs["x"][:] = 0.25
    sd = {"weight": cs["gamma"].clone(), "bias": cs["beta"].clone(), "running_mean": cs["rm"].clone(),
          "running_var": cs["rv"].clone(), "num_batches_tracked": t.tensor(cs["nbt"])}
    O.batch_renorm(cs["x"], sd, "", True, eps=EPS, momentum=MOM)
    ref = fwd_ref(cs["x"], False, cs["gamma"], cs["beta"], cs["rm"], cs["rv"], cs["nbt"])
    rm, rv = dev(cs["rm"]), dev(cs["rv"])
    sc, sh, sv = [t.full((n,), SENT, device=DEV) for n in (C, C, 4 * C)]
    be.bn_stats(cs["x"].to(DEV), B, C, S, C * S, False, cs["gamma"].to(DEV), cs["beta"].to(DEV), rm, rv,
                t.tensor([cs["nbt"]], dtype=t.int64).to(DEV), EPS, MOM, True, sc, sh, sv)
    rvh = rv.cpu()
    assert bool(t.isnan(rvh).all()) if const else bool(t.isinf(rvh).all() and (rvh > 0).all()), rvh
    assert t.equal(t.isnan(rvh), t.isnan(sd["running_var"])) and t.equal(t.isinf(rvh), t.isinf(sd["running_var"]))
    assert bool(t.isfinite(sc.cpu()).all() and t.isfinite(sh.cpu()).all())
    close(sc, ref["scale"], TOL, "C=1 scale"); close(sh, ref["shift"], TOL, "C=1 shift")
    close(rm, sd["running_mean"], TOL, "C=1 running_mean vs oracle")


# ------------------------------------------------------------------ crn_batch_renorm_finalize on given parts
def synthetic_parts(C, nparts, seed):
  """float64 [C, nparts, 2] = (sum x, sum x^2) of parts of 1000 elements each, magnitudes over six decades."""
  g = t.Generator().manual_seed(seed)
  mag = 10.0 ** (t.rand(C, nparts, generator=g, dtype=t.float64) * 6 - 3)
  s1 = t.randn(C, nparts, generator=g, dtype=t.float64) * mag
  s2 = s1 * s1 / 1000.0 * (1.0 + 2.0 * t.rand(C, nparts, generator=g, dtype=t.float64)) + t.rand(C, nparts, generator=g, dtype=t.float64) * 1000
  return t.stack([s1, s2], dim=-1).contiguous()


def finalize_case(C, nparts, seed):
  parts = synthetic_parts(C, nparts, seed)
  count = 1000.0 * nparts
  g = t.Generator().manual_seed(seed + 1)
  gamma = t.rand(C, generator=g) + 0.5; beta = t.randn(C, generator=g)
  s = parts.sum(1)
  mean = s[:, 0] / count; var = (s[:, 1] / count - mean * mean).clamp(min=0)
  rm = (mean + t.randn(C, generator=g, dtype=t.float64) * var.sqrt()).float()
  rv = (var * (0.5 + t.rand(C, generator=g, dtype=t.float64))).float()
  return parts, count, gamma, beta, rm, rv, finalize_ref(mean, var, C, gamma, beta, rm, rv, 30000)


def check_finalize(got, ref, name):
  sc, sh, sv, rm, rv = got
  C = sc.numel()
  errs = [close(sc, ref["scale"], TOL, name + " scale"), close(sh, ref["shift"], TOL, name + " shift"),
          close(rm, ref["running_mean"], TOL, name + " running_mean"), close(rv, ref["running_var"], TOL, name + " running_var")]
  errs += [close(sv.view(4, C)[i], ref["saved"][i], TOL, f"{name} saved[{i}]") for i in range(4)]
  return max(errs)


@pytest.mark.parametrize("C", [13, 5, 64])
@pytest.mark.parametrize("nparts", [1, 63, 64, 65, 511, 512, 513, 4096])
def test_finalize_from_given_parts(be, nparts, C):
  """The wave-per-channel kernel below 512 parts and the workgroup-per-channel kernel from 512 on, with a ragged last
  workgroup of channels, against the float64 sum of the parts."""
  parts, count, gamma, beta, rm0, rv0, ref = finalize_case(C, nparts, 100 * C + nparts)
  ws, _ = be._bn_ws(C, t.empty(0, device=DEV).device)
  ws[:C * nparts * 16].view(t.float64).copy_(parts.reshape(-1))
  rm, rv = dev(rm0), dev(rv0)
  sc, sh, sv = [t.full((n,), SENT, device=DEV) for n in (C, C, 4 * C)]
  be.bn_finalize(nparts, C, count, gamma.to(DEV), beta.to(DEV), rm, rv, t.tensor([30000], dtype=t.int64).to(DEV), EPS, MOM, sc, sh, sv)
  e = check_finalize((sc, sh, sv, rm, rv), ref, f"finalize C={C} nparts={nparts}")
  print(f"[batch_renorm] finalize C={C} nparts={nparts} ({'wide' if nparts >= 512 else 'narrow'}): max {e:.1e}")


def _finalize_direct(be, wsp, nparts, C, count, gamma, beta, rm, rv, sc, sh, sv):
  from corenet_amd._lib import ptr, stream
  be.lib.crn_batch_renorm_finalize(wsp, nparts, C, float(count), ptr(gamma), ptr(beta), ptr(rm), ptr(rv),
                                   ptr(t.tensor([30000], dtype=t.int64, device=DEV)), EPS, MOM, ptr(sc), ptr(sh), ptr(sv), stream())


def test_finalize_workspace_off_16_bytes(be):
  """512 parts in a workspace 8 bytes off 16-byte alignment: the wide kernel's 16-byte loads are not possible, the narrow
  kernel gives the same answer."""
  if _SELF:
    pytest.skip("alignment is the library's")
  C, nparts = 5, 512
  parts, count, gamma, beta, rm0, rv0, ref = finalize_case(C, nparts, 77)
  buf = t.zeros(C * nparts * 2 + 1, dtype=t.float64, device=DEV)
  buf[1:].copy_(parts.reshape(-1))
  assert (buf.data_ptr() + 8) % 16 == 8
  rm, rv = dev(rm0), dev(rv0)
  sc, sh, sv = [t.full((n,), SENT, device=DEV) for n in (C, C, 4 * C)]
  _finalize_direct(be, buf.data_ptr() + 8, nparts, C, count, gamma.to(DEV), beta.to(DEV), rm, rv, sc, sh, sv)
  _sync()
  check_finalize((sc, sh, sv, rm, rv), ref, "finalize off-16")


def test_finalize_rejections(be):
  if _SELF:
    pytest.skip("error returns are the library's")
  C = 5
  parts, count, gamma, beta, rm0, rv0, ref = finalize_case(C, 8, 78)
  buf = t.zeros(C * 4097 * 2, dtype=t.float64, device=DEV)
  rm, rv = dev(rm0), dev(rv0)
  sc, sh, sv = [t.full((n,), SENT, device=DEV) for n in (C, C, 4 * C)]
  for nparts, cnt in ((4097, 4097000.0), (0, 1000.0), (8, 0.5)):
    with pytest.raises(_hip_error(), match="status -1"):
      _finalize_direct(be, buf.data_ptr(), nparts, C, cnt, gamma.to(DEV), beta.to(DEV), rm, rv, sc, sh, sv)
  _sync()
  for v in (sc, sh, sv):
    all_sentinel(v, "finalize rejection")
  exact(rm, rm0); exact(rv, rv0)


# ------------------------------------------------------------------ elementwise kernels
ELT_SHAPES = [(2, 6, 100), (1, 2, 12293), (2, 3, 12296), (2, 5, 37)]
AFFINE_VARIANTS = ["all", "no_r", "r_plain", "y_pre_only", "y_only", "no_relu", "no_affine"]


@pytest.mark.parametrize("variant", AFFINE_VARIANTS)
@pytest.mark.parametrize("B,C,S", ELT_SHAPES + [(2, 6, 100)], ids=_ids(ELT_SHAPES) + ["2x6x100+4B"])
def test_affine_add_relu_variants(be, B, C, S, variant, request):
  mis = "+4B" in request.node.callspec.id
  x, r, sc, sh, rsc, rsh, _ = elementwise_inputs(B, C, S, S + len(variant))
  if variant == "no_r": r = rsc = rsh = None
  if variant == "r_plain": rsc = rsh = None
  if variant == "no_affine": sc = sh = None
  relu = variant != "no_relu"
  want = affine_ref(x, sc, sh, r, rsc, rsh)
  if mis:
    xbuf, xs, sBx = off_by_one_float(x)
  else:
    xbuf, xs, sBx = wide(x)
  rs, sBr = (None, 0)
  if r is not None:
    _, rs, sBr = wide(r, lead=0, extra=1)
  pbuf, yp, sBp = wide(t.full((B, C, S), SENT)) if variant != "y_only" else (None, None, 0)
  ybuf, y, sBy = wide(t.full((B, C, S), SENT), lead=2, extra=3) if variant != "y_pre_only" else (None, None, 0)
  be.affine_add_relu(xs, _opt(sc), _opt(sh), rs, _opt(rsc), _opt(rsh), B, C, S, sBx, sBr, yp, sBp, y, sBy, relu)
  if yp is not None:
    close(yp, want, 1e-6, f"affine {variant} y_pre"); neighbours_untouched(pbuf, C, "y_pre")
  if y is not None:
    close(y, want.clamp(min=0) if relu else want, 1e-6, f"affine {variant} y"); neighbours_untouched(ybuf, C, "y", lead=2)
  if y is not None and yp is not None:
    exact(y, yp.cpu().clamp(min=0) if relu else yp.cpu(), "y = relu(y_pre)")


@pytest.mark.parametrize("variant", ["all", "no_dy", "no_dy2"])
@pytest.mark.parametrize("B,C,S", ELT_SHAPES + [(2, 6, 100)], ids=_ids(ELT_SHAPES) + ["2x6x100+4B"])
def test_relu_bwd_add_variants(be, B, C, S, variant, request):
  mis = "+4B" in request.node.callspec.id
  g = t.Generator().manual_seed(S + len(variant))
  dy, act, dy2 = [t.randn(B, C, S, generator=g) for _ in range(3)]
  act[:, :, 0] = 0.0; act[:, :, 1] = -0.0
  if variant == "no_dy": dy = None
  if variant == "no_dy2": dy2 = None
  want = relu_bwd_ref(dy, act, dy2)
  abuf, acts, sBa = off_by_one_float(act) if mis else wide(act)
  dys, sBd = (None, 0) if dy is None else wide(dy, lead=0, extra=1)[1:]
  d2s, sB2 = (None, 0) if dy2 is None else wide(dy2, lead=2, extra=2)[1:]
  dxbuf, dxs, sBx = wide(t.full((B, C, S), SENT))
  be.relu_bwd_add(dys, acts, d2s, B, C, S, sBd, sBa, sB2, dxs, sBx)
  exact(dxs, want, f"relu_bwd_add {variant}")
  neighbours_untouched(dxbuf, C, "relu_bwd_add dx")


# ------------------------------------------------------------------ rejections
def test_batch_of_65_is_rejected(be):
  if _SELF:
    pytest.skip("error returns are the library's")
  B, C, S = 65, 2, 8
  HipError = _hip_error()
  z = lambda *s: t.full(s, SENT, device=DEV)
  x, dy, gg, act = [t.randn(B, C, S, device=DEV) for _ in range(4)]
  gamma, beta, rm, rv = [t.rand(C, device=DEV) + 0.5 for _ in range(4)]
  rm0, rv0 = rm.clone(), rv.clone()
  nbt = t.tensor([0], dtype=t.int64, device=DEV)
  sc, sh, sv, dg, db, ds = z(C), z(C), z(4 * C), z(C), z(C), z(C)
  y, yp, dx, dyo = z(B, C, S), z(B, C, S), z(B, C, S), z(B, C, S)
  n = C * S
  with pytest.raises(HipError, match="status -1"):
    be.bn_stats(x, B, C, S, n, False, gamma, beta, rm, rv, nbt, EPS, MOM, True, sc, sh, sv)
  with pytest.raises(HipError, match="status -1"):
    be.bn_stats_tail(x, B, C, S, n, gamma, beta, rm, rv, nbt, EPS, MOM, True, sc, sh, sv, None, None, None, 0, yp, n, y, n, True)
  one = t.ones(C, device=DEV); sv1 = t.ones(4 * C, device=DEV)
  with pytest.raises(HipError, match="status -1"):
    be.bn_bwd(x, n, dy, n, B, C, S, False, False, gamma, one, one, sv1, dx, n, dg, db, False, ds, C)
  with pytest.raises(HipError, match="status -1"):
    be.bn_bwd_head(x, n, dyo, n, gg, n, act, n, None, 0, B, C, S, gamma, one, one, sv1, dx, n, dg, db, False, ds, C)
  _sync()
  for v in (sc, sh, sv, dg, db, ds, y, yp, dx, dyo):
    all_sentinel(v, "B = 65")
  assert t.equal(rm, rm0) and t.equal(rv, rv0)


def test_short_workspace_is_rejected_before_any_launch(be):
  """The two-pass forms with a workspace one byte short: CRN_ENOMEM and nothing written -- in the forward, in the backward,
  and in crn_batch_renorm_bwd_apply's deterministic sum(dx), whose second use of the workspace can be the larger one."""
  if _SELF:
    pytest.skip("error returns are the library's")
  from corenet_amd._lib import ptr, stream
  B, C, S = 2, 3, 12296
  need = C * nsplit_for(S, C, B) * B * 16
  z = lambda *s: t.full(s, SENT, device=DEV)
  x, dy = t.randn(B, C, S, device=DEV), t.randn(B, C, S, device=DEV)
  gamma, beta, rm, rv = [t.rand(C, device=DEV) + 0.5 for _ in range(4)]
  rm0, rv0 = rm.clone(), rv.clone()
  nbt = t.tensor([0], dtype=t.int64, device=DEV)
  sc, sh, sv, dg, db, ds, dx = z(C), z(C), z(4 * C), z(C), z(C), z(C), z(B, C, S)
  ws = t.full((need + 64,), 0x5A, dtype=t.uint8, device=DEV)
  one = t.ones(C, device=DEV); sv1 = t.ones(4 * C, device=DEV)
  n = C * S
  with pytest.raises(_hip_error(), match="status -2"):
    be.lib.crn_batch_renorm_stats(ptr(x), B, C, S, n, 0, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(nbt), EPS, MOM, 1,
                                  ptr(sc), ptr(sh), ptr(sv), ptr(ws), need - 1, stream())
  with pytest.raises(_hip_error(), match="status -2"):
    be.lib.crn_batch_renorm_bwd(ptr(x), n, ptr(dy), n, B, C, S, 0, 0, ptr(gamma), ptr(one), ptr(one), ptr(sv1), ptr(dx), n,
                                ptr(dg), ptr(db), 0, ptr(ds), C, ptr(ws), need - 1, stream())
  # crn_batch_renorm_bwd_apply with one part per channel given: C * 1 * 16 bytes hold the sums, the ordered sum(dx) of
  # deterministic mode needs ndsum * nsplit * B * 8
  be.set_deterministic(True)
  try:
    det_need = C * nsplit_for(S, C, B) * B * 8
    assert C * 16 < det_need
    with pytest.raises(_hip_error(), match="status -2"):
      be.lib.crn_batch_renorm_bwd_apply(ptr(x), n, ptr(dy), n, B, C, S, 0, ptr(gamma), ptr(one), ptr(one), ptr(sv1), ptr(dx), n,
                                        ptr(dg), ptr(db), 0, ptr(ds), C, ptr(ws), det_need - 1, 1, stream())
  finally:
    be.set_deterministic(_DET0)
  _sync()
  for v in (sc, sh, sv, dg, db, ds, dx):
    all_sentinel(v, "short workspace")
  assert t.equal(rm, rm0) and t.equal(rv, rv0)
  assert bool((ws.cpu() == 0x5A).all())


def test_null_pointers_are_rejected(be):
  """A NULL where the contract needs a tensor is CRN_EINVAL, not a launch on address 0."""
  if _SELF:
    pytest.skip("error returns are the library's")
  from corenet_amd._lib import ptr, stream
  B, C, S = 2, 3, 16
  z = lambda *s: t.full(s, SENT, device=DEV)
  x, dy = t.randn(B, C, S, device=DEV), t.randn(B, C, S, device=DEV)
  gamma, beta, rm, rv = [t.rand(C, device=DEV) + 0.5 for _ in range(4)]
  nbt = t.tensor([0], dtype=t.int64, device=DEV)
  n = C * S
  ws, wsn = be._bn_ws(C, x.device)
  P = lambda a: [ptr(v) if (v is None or isinstance(v, t.Tensor)) else v for v in a]
  # (through be.lib: the backend's own methods ask a tensor for its device before they reach the library)
  stats = [x, B, C, S, n, 0, gamma, beta, rm, rv, nbt, EPS, MOM, 1, z(C), z(C), z(4 * C), ws, wsn]
  for i in (0, 6, 7, 8, 9, 10, 14, 15, 16):
    a = list(stats); a[i] = None
    with pytest.raises(_hip_error(), match="status -1"):
      be.lib.crn_batch_renorm_stats(*P(a), stream())
  one = t.ones(C, device=DEV); sv1 = t.ones(4 * C, device=DEV)
  bwd = [x, n, dy, n, B, C, S, 0, 0, gamma, one, one, sv1, z(B, C, S), n, z(C), z(C), 0, None, 0, ws, wsn]
  for i in (0, 2, 9, 10, 11, 12, 13, 15, 16):
    a = list(bwd); a[i] = None
    with pytest.raises(_hip_error(), match="status -1"):
      be.lib.crn_batch_renorm_bwd(*P(a), stream())
  _sync()
  for v in stats[14:17] + [bwd[13], bwd[15], bwd[16]]:
    all_sentinel(v, "NULL argument")


# ------------------------------------------------------------------ eval mode, deterministic mode
def eval_ref(gamma, beta, rm, rv):
  rstd = 1.0 / (rv.double() + EPS).sqrt()
  return gamma.double() * rstd, beta.double() - gamma.double() * rm.double() * rstd


@pytest.mark.parametrize("B,C,S", [(2, 5, 24), (2, 64, 1024), (2, 3, 12296)])
def test_eval_mode(be, B, C, S):
  """training = 0: scale / shift from the running statistics; running statistics and saved untouched; the tail entry
  equals eval statistics followed by crn_affine_add_relu, bit for bit."""
  cs = make_case(B, C, S, False, False, seed=23)
  x, r, _, _, rsc, rsh, _ = elementwise_inputs(B, C, S, 24)
  wsc, wsh = eval_ref(cs["gamma"], cs["beta"], cs["rm"], cs["rv"])
  rm, rv = dev(cs["rm"]), dev(cs["rv"])
  nbt = t.tensor([cs["nbt"]], dtype=t.int64).to(DEV)
  sc, sh, sv = [t.full((n,), SENT, device=DEV) for n in (C, C, 4 * C)]
  xg = cs["x"].to(DEV)
  be.bn_stats(xg, B, C, S, C * S, False, cs["gamma"].to(DEV), cs["beta"].to(DEV), rm, rv, nbt, EPS, MOM, False, sc, sh, sv)
  close(sc, wsc, TOL, "eval scale"); close(sh, wsh, TOL, "eval shift")
  all_sentinel(sv, "eval saved"); exact(rm, cs["rm"]); exact(rv, cs["rv"])
  y0, p0 = t.full((B, C, S), SENT, device=DEV), t.full((B, C, S), SENT, device=DEV)
  be.affine_add_relu(xg, sc, sh, r.to(DEV), rsc.to(DEV), rsh.to(DEV), B, C, S, C * S, C * S, p0, C * S, y0, C * S, True)
  sc2, sh2, sv2 = [t.full((n,), SENT, device=DEV) for n in (C, C, 4 * C)]
  y1, p1 = t.full((B, C, S), SENT, device=DEV), t.full((B, C, S), SENT, device=DEV)
  be.bn_stats_tail(xg, B, C, S, C * S, cs["gamma"].to(DEV), cs["beta"].to(DEV), rm, rv, nbt, EPS, MOM, False, sc2, sh2, sv2,
                   r.to(DEV), rsc.to(DEV), rsh.to(DEV), C * S, p1, C * S, y1, C * S, True)
  for a, b in ((sc2, sc), (sh2, sh), (y1, y0), (p1, p0)):
    assert t.equal(a, b)
  all_sentinel(sv2, "eval tail saved"); exact(rm, cs["rm"]); exact(rv, cs["rv"])
  close(p1, affine_ref(cs["x"], sc.cpu(), sh.cpu(), r, rsc, rsh), 1e-6, "eval tail y_pre")


@pytest.mark.parametrize("n", [0, 1, 256, 257])
def test_eval_affine_table(be, n):
  """crn_batch_renorm_eval_affine with shuffled table rows: one block, exactly one block, one more; n = 0 returns cleanly."""
  g = t.Generator().manual_seed(n)
  m = max(n, 1)
  params = t.randn(2 * m + 3, generator=g); buffers = t.cat([t.randn(m + 2, generator=g), t.rand(m + 1, generator=g) * 3 + 0.1])
  perm = lambda k: t.randperm(k, generator=g)[:n]
  ig, ib, im, iv, io = perm(m), m + perm(m) + 3, perm(m) + 2, m + 2 + perm(m), perm(m + 2)
  table = t.stack([ig, ib, im, iv, io], dim=1).to(t.int32).contiguous().view(n, 5)
  sc, sh = t.full((m + 2,), SENT, device=DEV), t.full((m + 2,), SENT, device=DEV)
  be.bn_eval_affine(params.to(DEV), buffers.to(DEV), table.to(DEV), EPS, sc, sh)
  _sync()
  wsc = t.full((m + 2,), SENT, dtype=t.float64); wsh = wsc.clone()
  if n:
    a, b = eval_ref(params[ig.long()], params[ib.long()], buffers[im.long()], buffers[iv.long()])
    wsc[io.long()] = a; wsh[io.long()] = b
  close(sc, wsc, TOL, "eval_affine scale"); close(sh, wsh, TOL, "eval_affine shift")
  untouched = t.ones(m + 2, dtype=t.bool); untouched[io.long()] = False
  all_sentinel(sc[untouched.to(DEV)]); all_sentinel(sh[untouched.to(DEV)])


@pytest.mark.parametrize("B,C,S", [(1, 64, 16388), (2, 3, 12296)])
def test_deterministic_dsum(be, B, C, S):
  """crn_set_deterministic: sum(dx) of the two-pass backward by an ordered reduction over dx that re-uses the workspace --
  within tolerance of float64, bit-identical run to run, and nothing else changes."""
  cs = make_case(B, C, S, True, False, seed=29)
  r32 = f32(fwd_ref(cs["x"], True, cs["gamma"], cs["beta"], cs["rm"], cs["rv"], cs["nbt"]))
  want = bwd_ref(cs["x"], cs["dy"], True, False, cs["gamma"], r32["scale"], r32["shift"], r32["saved"])
  xbuf, xs, sB = wide(cs["x"])
  args = [v.to(DEV) for v in (cs["gamma"], r32["scale"], r32["shift"], r32["saved"].reshape(-1))]
  dyg = cs["dy"].to(DEV)
  nds = max(1, C - 2)

  def run():
    dxbuf, dxs, sBdx = wide(t.full((B, C, S), SENT))
    dg, db, ds = [t.full((C,), SENT, device=DEV) for _ in range(3)]
    be.bn_bwd(xs, sB, dyg, C * S, B, C, S, True, False, *args, dxs, sBdx, dg, db, False, ds, nds)
    _sync()
    return [v.cpu().clone() for v in (dxbuf, dg, db, ds)]
  try:
    be.set_deterministic(False)
    plain = run()
    be.set_deterministic(True)
    det = [run(), run()]
  finally:
    be.set_deterministic(_DET0)
  bar = TOL * float(want["dx"].abs().sum((0, 2)).max())
  for d in det:
    e = float((d[3][:nds].double() - want["dsum"][:nds]).abs().max())
    assert e <= bar, f"deterministic dsum: {e:.3e} > {bar:.3e}"
    all_sentinel(d[3][nds:])
    for a, b, nm in zip(d[:3], plain[:3], ("dx", "dgamma", "dbeta")):
      assert t.equal(a, b), nm
  assert t.equal(det[0][3], det[1][3])
  close(plain[0][:, 1:C + 1], want["dx"], TOL, "dx")
  print(f"[batch_renorm] deterministic dsum {B}x{C}x{S}: {e / bar:.1e} of the bar")


# ------------------------------------------------------------------ split-K take-over
def test_stats_take_over_a_pending_splitk_sum(be):
  """crn_splitk_defer + a crn_conv2d_bf3 launch that splits leave the sum pending (the output keeps its sentinel); the
  statistics launch over that output adds the partial sums up, stores x and takes its statistics from the registers --
  x equals the un-deferred convolution and the statistics equal those over it, bit for bit.  A statistics call on another
  tensor flushes the pending sum instead."""
  if _SELF:
    pytest.skip("the emulator has no split-K")
  from corenet_amd import views as V
  from corenet_amd.model import conv_geometry as G
  EMU = EmuBackend()
  wshape, (H, W), B = (64, 192, 1, 1), (8, 8), 1          # one tile, two channel chunks: the launch splits in two
  cout, cin = wshape[:2]
  S = H * W
  g = t.Generator().manual_seed(41)
  w = t.randn(wshape, generator=g) / np.sqrt(cin)
  fwd = G.conv_fwd(wshape, 0)
  assert G.operand_eligible(fwd)
  idx = t.as_tensor(fwd.index); wf = t.zeros(idx.numel()); EMU.gather(w.reshape(-1), idx, wf)
  nf = G.operand_entries(fwd)
  desc, blocks = G.operand_table([(0, 0, fwd)])
  wop = t.zeros(nf * 32, dtype=t.uint8, device=DEV)
  be.bf3_operands(wf.to(DEV), (t.as_tensor(desc).to(DEV), blocks), wop)
  x = t.randn(B, cin, H, W, generator=g).to(DEV)
  conv = lambda y: be.conv2d_bf3(V.view_of(x), None, wop, fwd.npad, None, 0, V.view_of(y), fwd.window, fwd.pad_lo)
  y_ref = t.full((B, cout, H, W), SENT, device=DEV)
  conv(y_ref)
  _sync()
  assert not bool((y_ref == SENT).any())
  C = cout
  gamma, beta = (t.rand(C, generator=g) + 0.5).to(DEV), t.randn(C, generator=g).to(DEV)
  rm0, rv0 = t.randn(C, generator=g), t.rand(C, generator=g) * 3 + 0.1
  nbt = t.tensor([12000], dtype=t.int64, device=DEV)

  def stats(y):
    rm, rv = dev(rm0), dev(rv0)
    sc, sh, sv = [t.full((n,), SENT, device=DEV) for n in (C, C, 4 * C)]
    be.bn_stats(y, B, C, S, C * S, False, gamma, beta, rm, rv, nbt, EPS, MOM, True, sc, sh, sv)
    _sync()
    return sc, sh, sv, rm, rv
  want = stats(y_ref)
  y = t.full((B, cout, H, W), SENT, device=DEV)
  be.splitk_defer()
  conv(y)
  _sync()
  all_sentinel(y, "the split-K sum was not left pending: the test would prove nothing")
  got = stats(y)
  assert t.equal(y, y_ref)
  for a, b, nm in zip(got, want, ("scale", "shift", "saved", "running_mean", "running_var")):
    assert t.equal(a, b), nm
  # the statistics call is for another tensor: the pending sum is flushed
  y2 = t.full((B, cout, H, W), SENT, device=DEV)
  be.splitk_defer()
  conv(y2)
  _sync()
  all_sentinel(y2, "the split-K sum was not left pending")
  other = stats(y_ref.clone())
  assert t.equal(y2, y_ref)
  for a, b in zip(other, want):
    assert t.equal(a, b)


def test_backward_takes_over_a_pending_splitk_sum(be):
  """The same on the backward side: the deferred convolution's output is the `dy` of a BatchRenorm backward (a data gradient
  in the engine).  The backward launch adds the partial sums up while it loads them and does NOT store dy (it is the only
  reader): dx, dgamma, dbeta and dsum equal those over the un-deferred convolution bit for bit and dy keeps its sentinel.
  A backward call on another dy flushes the pending sum instead."""
  if _SELF:
    pytest.skip("the emulator has no split-K")
  from corenet_amd import views as V
  from corenet_amd.model import conv_geometry as G
  EMU = EmuBackend()
  wshape, (H, W), B = (64, 192, 1, 1), (8, 8), 1          # the forward test's shape: two splits, the NV = 1 register kernel
  C, cin = wshape[:2]
  S = H * W
  g = t.Generator().manual_seed(43)
  w = t.randn(wshape, generator=g) / np.sqrt(cin)
  fwd = G.conv_fwd(wshape, 0)
  assert G.operand_eligible(fwd)
  idx = t.as_tensor(fwd.index); wf = t.zeros(idx.numel()); EMU.gather(w.reshape(-1), idx, wf)
  desc, blocks = G.operand_table([(0, 0, fwd)])
  wop = t.zeros(G.operand_entries(fwd) * 32, dtype=t.uint8, device=DEV)
  be.bf3_operands(wf.to(DEV), (t.as_tensor(desc).to(DEV), blocks), wop)
  a = t.randn(B, cin, H, W, generator=g).to(DEV)
  conv = lambda y: be.conv2d_bf3(V.view_of(a), None, wop, fwd.npad, None, 0, V.view_of(y), fwd.window, fwd.pad_lo)
  dy_ref = t.full((B, C, H, W), SENT, device=DEV)
  conv(dy_ref)
  _sync()
  assert not bool((dy_ref == SENT).any())
  x = t.randn(B, C, S, generator=g) * 2 + 0.4
  gamma, beta = t.rand(C, generator=g) + 0.5, t.randn(C, generator=g)
  r32 = f32(fwd_ref(x, False, gamma, beta, t.randn(C, generator=g), t.rand(C, generator=g) * 3 + 0.1, 12000))
  xd = x.to(DEV)
  args = [v.to(DEV) for v in (gamma, r32["scale"], r32["shift"], r32["saved"].reshape(-1))]
  nds = C - 2

  def bwd(dy):
    dx = t.full((B, C, S), SENT, device=DEV)
    dg, db, ds = [t.full((C,), SENT, device=DEV) for _ in range(3)]
    be.bn_bwd(xd, C * S, dy, C * S, B, C, S, False, False, *args, dx, C * S, dg, db, False, ds, nds)
    _sync()
    return dx, dg, db, ds
  names = ("dx", "dgamma", "dbeta", "dsum")
  want = bwd(dy_ref)
  assert not bool((want[0] == SENT).any()) and not bool((want[3][:nds] == SENT).any())
  all_sentinel(want[3][nds:], "dsum tail")
  dy = t.full((B, C, H, W), SENT, device=DEV)
  be.splitk_defer()
  conv(dy)
  _sync()
  all_sentinel(dy, "the split-K sum was not left pending: the test would prove nothing")
  got = bwd(dy)
  for p, q, nm in zip(got, want, names):
    assert t.equal(p, q), nm
  all_sentinel(dy, "dy is not written by the take-over")
  # the backward call is for another dy: the pending sum is flushed
  dy2 = t.full((B, C, H, W), SENT, device=DEV)
  be.splitk_defer()
  conv(dy2)
  _sync()
  all_sentinel(dy2, "the split-K sum was not left pending")
  other = bwd(dy_ref.clone())
  assert t.equal(dy2, dy_ref)
  for p, q, nm in zip(other, want, names):
    assert t.equal(p, q), nm


def _packed(w, geom):
  idx = t.as_tensor(geom.index); out = t.zeros(idx.numel())
  EmuBackend().gather(w.reshape(-1), idx, out)
  return out


def _stats_after_a_deferred_conv(be, conv, yshape, pre_relu, seed):
  """The steps of test_stats_take_over_a_pending_splitk_sum for any producer: conv(y) runs the convolution into y.  All four
  producers end in crn_splitk_finish, so each is held to the same bit-for-bit result whether the statistics launch takes the
  sum over (its register form) or flushes it first."""
  B, C = yshape[:2]
  S = int(np.prod(yshape[2:]))
  g = t.Generator().manual_seed(seed)
  y_ref = t.full(yshape, SENT, device=DEV)
  conv(y_ref)
  _sync()
  assert not bool((y_ref == SENT).any())
  gamma, beta = (t.rand(C, generator=g) + 0.5).to(DEV), t.randn(C, generator=g).to(DEV)
  rm0, rv0 = t.randn(C, generator=g), t.rand(C, generator=g) * 3 + 0.1
  nbt = t.tensor([12000], dtype=t.int64, device=DEV)

  def stats(y):
    rm, rv = dev(rm0), dev(rv0)
    sc, sh, sv = [t.full((n,), SENT, device=DEV) for n in (C, C, 4 * C)]
    be.bn_stats(y, B, C, S, C * S, pre_relu, gamma, beta, rm, rv, nbt, EPS, MOM, True, sc, sh, sv)
    _sync()
    return sc, sh, sv, rm, rv
  names = ("scale", "shift", "saved", "running_mean", "running_var")
  want = stats(y_ref)
  y = t.full(yshape, SENT, device=DEV)
  be.splitk_defer()
  conv(y)
  _sync()
  all_sentinel(y, "the split-K sum was not left pending: the test would prove nothing")
  got = stats(y)
  assert t.equal(y, y_ref)
  for a, b, nm in zip(got, want, names):
    assert t.equal(a, b), nm
  # the statistics call is for another tensor: the pending sum is flushed
  y2 = t.full(yshape, SENT, device=DEV)
  be.splitk_defer()
  conv(y2)
  _sync()
  all_sentinel(y2, "the split-K sum was not left pending")
  other = stats(y_ref.clone())
  assert t.equal(y2, y_ref)
  for a, b, nm in zip(other, want, names):
    assert t.equal(a, b), nm


def _fp32_conv(be, wshape, pad, hw, seed):
  """crn_conv_fwd with splits = 0 (the engine's value: the backend's default of 1 disables the automatic split) on one sample."""
  from corenet_amd import views as V
  from corenet_amd.model import conv_geometry as G
  g = t.Generator().manual_seed(seed)
  w = t.randn(wshape, generator=g) / np.sqrt(np.prod(wshape[1:]))
  fwd = G.conv_fwd(wshape, pad)
  wf = _packed(w, fwd).to(DEV)
  x = t.randn((1, wshape[1]) + hw, generator=g).to(DEV)
  def conv(y, accumulate=False):
    be.conv_fwd(V.view_of(x), None, wf, fwd.npad, None, 0, V.view_of(y), fwd.window, fwd.pad_lo, 0, accumulate, math="fp32")
  return conv


def test_stats_after_a_deferred_pointwise_conv(be):
  """The fp32 pointwise path of crn_conv_fwd: weight (64, 256, 1, 1) on one 8 x 8 map is 2 workgroups and 256 / 128 = 2
  channel slices, so the dispatch computes 2 splits."""
  if _SELF:
    pytest.skip("the emulator has no split-K")
  _stats_after_a_deferred_conv(be, _fp32_conv(be, (64, 256, 1, 1), 0, (8, 8), 45), (1, 64, 8, 8), False, 46)


def test_stats_after_a_deferred_generic_fp32_conv(be):
  """The generic fp32 engine of crn_conv_fwd: weight (128, 256, 3, 3) on one 8 x 8 map.  Every tile configuration covers the
  map with one position tile (at most 8 workgroups over the 128 columns) and needs at least four channel chunks, so the cost
  model's split penalty (20000 cycles) is far below the chunks a split saves each workgroup: 256 input channels already
  split (the sentinel assertion says so on the GPU), the encoder's own 512 -> 512 is not needed."""
  if _SELF:
    pytest.skip("the emulator has no split-K")
  _stats_after_a_deferred_conv(be, _fp32_conv(be, (128, 256, 3, 3), 1, (8, 8), 47), (1, 128, 8, 8), False, 48)


def test_stats_after_a_deferred_bf16x3_conv(be):
  """The split-bf16 decoder engine (crn_conv_fwd_bf3_slabs): weight (16, 64, 5, 5, 5) on one 8^3 sample is one tile and one
  column block, which cannot fill the chip, so the launch splits over its channel chunks.  The statistics are the decoder's
  (pre_relu); 16 channels are below the channel-owner form, so here the statistics call flushes the pending sum itself."""
  if _SELF:
    pytest.skip("the emulator has no split-K")
  from corenet_amd import views as V
  from corenet_amd.model import conv_geometry as G
  wshape, dims = (16, 64, 5, 5, 5), (8, 8, 8)
  g = t.Generator().manual_seed(49)
  w = t.randn(wshape, generator=g) / np.sqrt(np.prod(wshape[1:]))
  fwd = G.conv_fwd(wshape, 2)
  desc, blocks = G.operand_table([(0, 0, fwd, True)])
  slab = t.zeros(G.slab_entries(fwd) * 32, dtype=t.uint8, device=DEV)
  be.bf3_operands(_packed(w, fwd).to(DEV), (t.as_tensor(desc).to(DEV), blocks), slab)
  x = t.randn((1, wshape[1]) + dims, generator=g).to(DEV)
  conv = lambda y: be.conv_fwd(V.view_of(x), None, None, fwd.npad, None, 0, V.view_of(y), fwd.window, fwd.pad_lo, 0,
                               math="bf16x3", wslab=slab)
  _stats_after_a_deferred_conv(be, conv, (1, wshape[0]) + dims, True, 50)


def test_an_accumulating_conv_is_never_left_pending(be):
  """accumulate with the arming set (the pointwise producer's shape): the sum is reduced at once -- y is written when the call
  returns -- and equals the un-armed accumulating call bit for bit.  Both equal prior + the plain result exactly: the reduction
  adds the splits up in the plain call's order (split 0 first, from zero) and then adds that float32 sum to y once."""
  if _SELF:
    pytest.skip("the emulator has no split-K")
  conv = _fp32_conv(be, (64, 256, 1, 1), 0, (8, 8), 45)
  y_ref = t.full((1, 64, 8, 8), SENT, device=DEV)
  be.splitk_defer()
  conv(y_ref)
  _sync()
  all_sentinel(y_ref, "the launch does not split: the test would prove nothing")
  prior = t.randn(1, 64, 8, 8, generator=t.Generator().manual_seed(51)).to(DEV)
  conv(y_ref.clone())                                      # (flushes the sum left pending for y_ref)
  _sync()
  assert not bool((y_ref == SENT).any())
  y_a = prior.clone()
  conv(y_a, accumulate=True)
  _sync()
  y_b = prior.clone()
  be.splitk_defer()
  conv(y_b, accumulate=True)
  _sync()
  assert not t.equal(y_b, prior), "the accumulating sum was left pending"
  assert t.equal(y_b, y_a)
  assert t.equal(y_a, prior + y_ref)


# ------------------------------------------------------------------ the formula itself
@pytest.mark.parametrize("pre,post", [(False, False), (True, False), (False, True), (True, True)])
def test_backward_formula_is_autograd_of_the_oracle(pre, post):
  """The float64 references of this module (forward contract + backward formula of include/corenet_hip.h) against autograd
  through oracle.corenet_oracle.batch_renorm on .double() inputs, to 1e-10.  CPU only."""
  B, C, S, nbt = 3, 6, 50, 30000
  cs = make_case(B, C, S, pre, post, nbt=nbt, seed=31)
  x64 = cs["x"].double()
  sd = {"weight": cs["gamma"].double().requires_grad_(True), "bias": cs["beta"].double().requires_grad_(True),
        "running_mean": cs["rm"].double(), "running_var": cs["rv"].double(), "num_batches_tracked": t.tensor(nbt)}
  xi = x64.clone().requires_grad_(True)
  y = O.batch_renorm(xi.relu() if pre else xi, sd, "", True, eps=EPS, momentum=MOM)
  if post: y = y.relu()
  y.backward(cs["dy"].double())
  ref = fwd_ref(cs["x"], pre, cs["gamma"], cs["beta"], cs["rm"], cs["rv"], nbt)
  close(ref["running_mean"], sd["running_mean"], 1e-10, "running_mean"); close(ref["running_var"], sd["running_var"], 1e-10, "running_var")
  # (float64 scale / shift / saved: the formula, not the rounding of its inputs, is under test here)
  want = bwd_ref(cs["x"], cs["dy"], pre, post, cs["gamma"], ref["scale"], ref["shift"], ref["saved"])
  close(want["dx"], xi.grad, 1e-10, "dx"); close(want["dgamma"], sd["weight"].grad, 1e-10, "dgamma")
  close(want["dbeta"], sd["bias"].grad, 1e-10, "dbeta"); 
  # (sum(dx) cancels to ~0 without pre_relu: against sum|dx|, as everywhere)
  assert float((want["dsum"] - xi.grad.sum((0, 2))).abs().max()) <= 1e-10 * float(xi.grad.abs().sum((0, 2)).max())
  yo = out_ref(cs["x"], pre, ref["scale"], ref["shift"])
  close(yo.clamp(min=0) if post else yo, y.detach(), 1e-10, "y")


def test_mask_margin_converges_for_every_post_relu_case():
  """The host-side precondition of every post_relu case above, without a GPU."""
  for B, C, S in REG_SHAPES[:4] + TWO_PASS_SHAPES[:2] + [(2, 64, 256)]:
    cs = make_case(B, C, S, False, True)
    r32 = f32(fwd_ref(cs["x"], False, cs["gamma"], cs["beta"], cs["rm"], cs["rv"], cs["nbt"]))
    assert mask_margin(cs["x"], False, r32["scale"], r32["shift"]) >= MASK_MARGIN
