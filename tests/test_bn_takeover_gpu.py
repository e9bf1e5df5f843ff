"""The two-pass BatchRenorm launches (csrc/batch_renorm.hip: bn_partial_kernel + finalize, bn_bwd_partial_kernel +
bn_bwd_apply_kernel) take a pending split-K sum over: the first pass adds the splits up in the reduction kernel's order
(split 0 first), stores the sum and accumulates from it.  Everything is compared BIT FOR BIT with reduction launch + the same
call: x / dy after the call, every statistic, every gradient.

Shapes: the smallest channel that leaves the register form, just over 16 Ki elements (B = 2, S = 8200 = 82 x 100), with
C = 3 channels (below the one-workgroup-per-channel forms), so both calls take their two-pass path with two slices per
sample.  The producer is crn_conv_fwd with explicit splits = 3 (the generic fp32 engine: 192 input channels, 1 x 1 window)."""
import numpy as np
import pytest
import torch as t

from corenet_amd import views as V
from corenet_amd.model import conv_geometry as G
from kernel_contract_emu import EmuBackend

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -1234.5
EPS, MOM = 1e-5, 0.01
B, C, CIN, HW = 2, 3, 192, (82, 100)
S = HW[0] * HW[1]
SPLITS = 3


@pytest.fixture(scope="module")
def be():
  from corenet_amd.backend import HipBackend
  assert t.cuda.is_available(), "gpu tests need an MI355X"
  return HipBackend()


def _packed(w, geom):
  idx = t.as_tensor(geom.index); out = t.zeros(idx.numel())
  EmuBackend().gather(w.reshape(-1), idx, out)
  return out


def conv_setup(be, seed, dev=DEV):
  """-> (conv(y_storage, offset=0): the split convolution into the dense [B, C, S] tensor at `offset` floats of the storage,
  plan(y_storage): what it would launch)."""
  g = t.Generator().manual_seed(seed)
  wshape = (C, CIN, 1, 1)
  w = t.randn(wshape, generator=g) / np.sqrt(CIN)
  fwd = G.conv_fwd(wshape, 0)
  wf = _packed(w, fwd).to(dev)
  x = t.randn((B, CIN) + HW, generator=g).to(dev)

  def yview(st, offset):
    return V.View(st, offset, B, C, 1, HW[0], HW[1], C * S, S, S, HW[1], 1)

  def conv(st, offset=0):
    be.conv_fwd(V.view_of(x), None, wf, fwd.npad, None, 0, yview(st, offset), fwd.window, fwd.pad_lo, SPLITS, False, math="fp32")

  def plan(st, offset=0):
    return be.conv_fwd_plan(V.view_of(x), None, wf, fwd.npad, None, 0, yview(st, offset), fwd.window, fwd.pad_lo, SPLITS, False)
  return conv, plan


def _sync():
  t.cuda.synchronize()


def _bits_equal(a, b):
  return bool(t.equal(a.contiguous().view(t.int32), b.contiguous().view(t.int32)))


def _norm_inputs(seed):
  g = t.Generator().manual_seed(seed)
  gamma, beta = (t.rand(C, generator=g) + 0.5).to(DEV), t.randn(C, generator=g).to(DEV)
  rm0, rv0 = t.randn(C, generator=g), t.rand(C, generator=g) * 3 + 0.1
  nbt = t.tensor([12000], dtype=t.int64, device=DEV)
  return g, gamma, beta, rm0, rv0, nbt


def test_the_producer_splits_in_three(be):
  conv, plan = conv_setup(be, 60)
  p = plan(t.empty(B * C * S, device=DEV))
  assert p["path"] == "generic" and p["splits"] == SPLITS, p


@pytest.mark.parametrize("offset", [0, 1], ids=["float4", "scalar_unaligned_base"])
def test_two_pass_statistics_take_the_pending_sum(be, offset):
  """bn_stats over the deferred convolution's output: scale, shift, saved, the running statistics and x itself equal
  reduction + bn_stats bit for bit.  offset 1: x starts 4 bytes off a 16-byte boundary (S % 4 == 0 all the same), which
  forces the scalar kernels -- a dense x cannot have an unaligned batch stride, so the base does it here."""
  conv, _ = conv_setup(be, 61)
  g, gamma, beta, rm0, rv0, nbt = _norm_inputs(62)
  n = B * C * S

  def stats(st):
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    sc, sh, sv = [t.full((k,), SENT, device=DEV) for k in (C, C, 4 * C)]
    be.bn_stats(st[offset:offset + n], B, C, S, C * S, True, gamma, beta, rm, rv, nbt, EPS, MOM, True, sc, sh, sv)
    _sync()
    return sc, sh, sv, rm, rv
  y_ref = t.full((n + 4,), SENT, device=DEV)
  conv(y_ref, offset)
  _sync()
  assert not bool((y_ref[offset:offset + n] == SENT).any())
  want = stats(y_ref)
  y = t.full((n + 4,), SENT, device=DEV)
  be.splitk_defer()
  conv(y, offset)
  _sync()
  assert bool((y == SENT).all()), "the split-K sum was not left pending: the test would prove nothing"
  got = stats(y)
  assert _bits_equal(y, y_ref), "x after the call (the guard floats around it included)"
  for a, b_, nm in zip(got, want, ("scale", "shift", "saved", "running_mean", "running_var")):
    assert _bits_equal(a, b_), nm
    assert not bool((a == SENT).any()), nm


@pytest.mark.parametrize("sbx_pad", [0, 1], ids=["float4", "scalar_unaligned_batch_stride"])
@pytest.mark.parametrize("pre,post", [(True, False), (False, True)])
def test_two_pass_backward_takes_the_pending_sum(be, sbx_pad, pre, post):
  """bn_bwd whose dy is the deferred convolution's output: dx, dgamma, dbeta, dsum and the final contents of dy equal
  reduction + bn_bwd bit for bit.  sbx_pad 1: the norm's input x has a batch stride of C * S + 1 floats, which forces the
  scalar kernels (dy stays dense, as the hand-over requires).
  dsum: the two-pass backward adds its 2 x B shares per channel with atomics, whose order the hardware picks, so in the default
  mode two runs of the SAME call may differ in the last bits; it is compared bit for bit in deterministic mode (ordered sums),
  and in the default mode within 6 x 2^-24 x sum |dx| of the channel (three roundings of at most 2^-24 x sum |dx| per run)."""
  conv, _ = conv_setup(be, 63)
  g, gamma, beta, rm0, rv0, nbt = _norm_inputs(64)
  n = B * C * S
  sBx = C * S + sbx_pad
  xh = t.randn(B, sBx, generator=g) * 2 + 0.4
  xd = xh.reshape(-1).to(DEV)
  sc, sh, sv = [t.full((k,), SENT, device=DEV) for k in (C, C, 4 * C)]
  be.bn_stats(xd, B, C, S, sBx, pre, gamma, beta, rm0.to(DEV), rv0.to(DEV), nbt, EPS, MOM, True, sc, sh, sv)
  nds = C - 1

  def bwd(dy):
    dx = t.full((B, C, S), SENT, device=DEV)
    dg, db, ds = [t.full((C,), SENT, device=DEV) for _ in range(3)]
    be.bn_bwd(xd, sBx, dy, C * S, B, C, S, pre, post, gamma, sc, sh, sv, dx, C * S, dg, db, False, ds, nds)
    _sync()
    return dx, dg, db, ds

  for deterministic in (True, False):
    try:
      be.set_deterministic(deterministic)
      dy_ref = t.full((n,), SENT, device=DEV)
      conv(dy_ref)
      _sync()
      assert not bool((dy_ref == SENT).any())
      want = bwd(dy_ref)
      dy = t.full((n,), SENT, device=DEV)
      be.splitk_defer()
      conv(dy)
      _sync()
      assert bool((dy == SENT).all()), "the split-K sum was not left pending: the test would prove nothing"
      got = bwd(dy)
    finally:
      be.set_deterministic(False)
    assert _bits_equal(dy, dy_ref), "dy after the call"
    for a, b_, nm in zip(got[:3], want[:3], ("dx", "dgamma", "dbeta")):
      assert _bits_equal(a, b_), (nm, deterministic)
      assert not bool((a == SENT).any()), nm
    assert bool((got[3][nds:] == SENT).all()) and not bool((got[3][:nds] == SENT).any())
    if deterministic:
      assert _bits_equal(got[3], want[3]), "dsum"
    else:
      bound = 6 * 2.0 ** -24 * want[0].double().abs().sum((0, 2))[:nds]
      d = (got[3][:nds].double() - want[3][:nds].double()).abs()
      print("dsum, default mode: |difference|", d.tolist(), "bound", bound.tolist())
      assert bool((d <= bound).all()), (d, bound)


def test_a_call_on_another_tensor_still_flushes(be):
  """The hand-over conditions reject a bn_bwd / bn_stats over a different tensor than the pending convolution's output: the
  sum is flushed (the conv's output then holds the reference) and the call gives what it gives with nothing pending."""
  conv, _ = conv_setup(be, 65)
  g, gamma, beta, rm0, rv0, nbt = _norm_inputs(66)
  n = B * C * S
  xd = (t.randn(B, C, S, generator=g) * 2 + 0.4).to(DEV)
  sc, sh, sv = [t.full((k,), SENT, device=DEV) for k in (C, C, 4 * C)]
  be.bn_stats(xd, B, C, S, C * S, True, gamma, beta, rm0.to(DEV), rv0.to(DEV), nbt, EPS, MOM, True, sc, sh, sv)
  y_ref = t.full((n,), SENT, device=DEV)
  conv(y_ref)
  _sync()
  other = t.randn(n, generator=g).to(DEV)

  def bwd(dy):
    dx = t.full((B, C, S), SENT, device=DEV)
    dg, db = [t.full((C,), SENT, device=DEV) for _ in range(2)]
    be.bn_bwd(xd, C * S, dy, C * S, B, C, S, True, False, gamma, sc, sh, sv, dx, C * S, dg, db, False, None, 0)
    _sync()
    return dx, dg, db

  def stats(x):
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    o = [t.full((k,), SENT, device=DEV) for k in (C, C, 4 * C)]
    be.bn_stats(x, B, C, S, C * S, True, gamma, beta, rm, rv, nbt, EPS, MOM, True, *o)
    _sync()
    return (*o, rm, rv)
  for call in (bwd, stats):
    want = call(other.clone())
    y = t.full((n,), SENT, device=DEV)
    be.splitk_defer()
    conv(y)
    _sync()
    assert bool((y == SENT).all()), "the split-K sum was not left pending"
    o2 = other.clone()
    got = call(o2)
    assert _bits_equal(y, y_ref), "the flushed sum"
    assert _bits_equal(o2, other), "the tensor the call was for"
    for a, b_ in zip(got, want):
      assert _bits_equal(a, b_)


def _captured_nodes(be, side, fn):
  """How many launches fn() enqueues on the stream `side`: they are captured into a HIP graph that is never launched (the
  runtime the library itself is linked against, reached through the library's handle)."""
  import ctypes
  hip = be.lib.cdll
  st, graph, n = ctypes.c_void_p(side.cuda_stream), ctypes.c_void_p(), ctypes.c_size_t()
  assert hip.hipStreamBeginCapture(st, 2) == 0            # hipStreamCaptureModeRelaxed
  try:
    fn()
  finally:
    rc = hip.hipStreamEndCapture(st, ctypes.byref(graph))
  assert rc == 0 and graph.value
  assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
  hip.hipGraphDestroy(graph)
  return n.value


def test_the_hand_over_is_one_launch_fewer_than_a_flush(be):
  """The bit-for-bit comparisons above hold whether the two-pass call takes the pending sum over or flushes it first, so the
  hand-over itself is pinned by counting launches: the call over the pending convolution's output enqueues as many launches
  as the same call with nothing pending (first pass + second pass), the call over another tensor one more (the reduction).
  The launches are captured, not run; every buffer and the stream's workspaces exist before the capture."""
  conv, _ = conv_setup(be, 67)
  g, gamma, beta, rm0, rv0, nbt = _norm_inputs(68)
  n = B * C * S
  xd = (t.randn(B, C, S, generator=g) * 2 + 0.4).to(DEV)
  other = t.randn(n, generator=g).to(DEV)
  sc, sh, sv = [t.full((k,), SENT, device=DEV) for k in (C, C, 4 * C)]
  rm, rv = rm0.to(DEV), rv0.to(DEV)
  be.bn_stats(xd, B, C, S, C * S, True, gamma, beta, rm, rv, nbt, EPS, MOM, True, sc, sh, sv)
  dx = t.full((B, C, S), SENT, device=DEV)
  dg, db = [t.full((C,), SENT, device=DEV) for _ in range(2)]
  o = [t.full((k,), SENT, device=DEV) for k in (C, C, 4 * C)]
  ys = [t.full((n,), SENT, device=DEV) for _ in range(5)]
  bwd = lambda dy: be.bn_bwd(xd, C * S, dy, C * S, B, C, S, True, False, gamma, sc, sh, sv, dx, C * S, dg, db, False, None, 0)
  stats = lambda x: be.bn_stats(x, B, C, S, C * S, True, gamma, beta, rm, rv, nbt, EPS, MOM, True, *o)
  _sync()
  side = t.cuda.Stream()
  try:
    with t.cuda.stream(side):
      conv(ys[0]); bwd(ys[0]); stats(ys[0])                  # this stream's scratch and BatchRenorm workspace, code objects
      _sync()
      for k, call in enumerate((bwd, stats)):
        plain = _captured_nodes(be, side, lambda: call(other))
        be.splitk_defer()
        conv(ys[1 + 2 * k])
        flushed = _captured_nodes(be, side, lambda: call(other))
        be.splitk_defer()
        conv(ys[2 + 2 * k])
        taken = _captured_nodes(be, side, lambda: call(ys[2 + 2 * k]))
        _sync()
        print(f"launches of {'bn_bwd' if k == 0 else 'bn_stats'}: nothing pending {plain}, flushed {flushed}, handed over {taken}")
        assert plain == 2, plain
        assert flushed == plain + 1 and taken == plain, (plain, flushed, taken)
  finally:
    _sync()
    be.splitk_release(side)
