"""GPU tests of the small kernels every training step and every evaluation number passes through -- the fused
losses, argmax + confusion matrix, Adam, and the encoder-head / decoder-entry kernels (csrc/losses.hip,
csrc/misc_ops.hip, crn_bias_grad) -- at the shapes where their code takes another path: one thread, ragged blocks,
more than one block, the block caps and the grid-stride trips behind them, both ends of every class-count
instantiation, channel slices of wider buffers, unaligned pointers.

Every reference is written here in float64 (plain torch expressions, autograd through them, or the oracle's loss
functions on .double() logits); integer and copy work must be exact, float32 work within the project's tolerances
for the same kind of quantity.  CRN_TEST_SELFCHECK=1 runs the same assertions against the contract emulator on a
CPU (error returns, alignment rejections and bit-for-bit comparisons of two kernels are then left out)."""
import functools
import os

import numpy as np
import pytest
import torch as t

from oracle import corenet_oracle as O
from kernel_contract_emu import EmuBackend

pytestmark = pytest.mark.gpu

_SELF = os.environ.get("CRN_TEST_SELFCHECK") == "1"
DEV = "cpu" if _SELF else "cuda"
F = t.nn.functional


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


def _device():
  """The device the tensors of the tests live on, with its index (the backend keys its workspaces by it)."""
  return t.empty(0, device=DEV).device


def dev(x):
  """A copy on the device under test, for a tensor the call writes (under the emulator .to() alone would alias it)."""
  return x.clone().to(DEV)


def close(a, b, rtol, name=""):
  a = a.detach().cpu().double(); b = b.detach().cpu().double()
  den = float(b.abs().max()) + 1e-30
  err = float((a - b).abs().max()) / den
  assert err <= rtol, f"{name}: max-abs-err/max = {err:.3e} > {rtol}"


def exact(a, want64, name=""):
  """a (device, float32) equals the float64 reference cast to float32, bit for bit."""
  assert t.equal(a.detach().cpu(), want64.to(a.dtype)), name


# ------------------------------------------------------------------ losses
KINDS = sorted(EmuBackend.LOSSES)
LOSS_RTOL, GRAD_RTOL = 1e-5, 2e-5       # the project's values (test_losses* of test_kernels_gpu.py)


def _loss_inputs(B, C, S, seed, weighted=False, scale=2.0):
  g = t.Generator().manual_seed(seed)
  logits = t.randn(B, C, S, generator=g) * scale
  gt = t.randint(0, C, (B, S), generator=g)
  w = t.rand(B, S, generator=g) * 1.5 if weighted else None
  return logits, gt, w


def _loss_ref(kind, logits, gt, w):
  """The oracle's loss on float64 logits and its autograd gradient: (float, [B][C][S] float64)."""
  B, C, S = logits.shape
  l = logits.double().view(B, C, 1, 1, S).clone().requires_grad_(True)
  v = getattr(O, EmuBackend.LOSSES[kind])(gt.view(B, 1, 1, S), l, None if w is None else w.double().view(B, 1, 1, S))
  assert v.dtype == t.float64
  v.backward()
  return float(v.detach()), l.grad.view(B, C, S)


def _loss_run(be, kind, logits, gt, w, grad_scale=1.0, grad=True):
  B, C, S = logits.shape
  loss = t.full((1,), -7.0, device=DEV)
  dl = t.full((B, C, 1, 1, S), -7.0, device=DEV) if grad else None
  be.loss_fwd_bwd(kind, logits.view(B, C, 1, 1, S).to(DEV), gt.to(t.int32).to(DEV), B, C, S, loss, dl, grad_scale,
                  weights=None if w is None else w.to(DEV))
  return loss.cpu(), (dl.cpu().view(B, C, S) if grad else None)


def _loss_check(be, kind, logits, gt, w, name, gt_ref=None, logits_ref=None):
  want, gwant = _loss_ref(kind, logits if logits_ref is None else logits_ref, gt if gt_ref is None else gt_ref, w)
  loss, dl = _loss_run(be, kind, logits, gt, w)
  err = abs(float(loss) - want) / max(1.0, abs(want))
  assert err <= LOSS_RTOL, f"{name}: loss {float(loss)!r} vs {want!r} (rel {err:.3e})"
  close(dl, gwant, GRAD_RTOL, name)


# S: one thread, a ragged block, exactly one block, two blocks, 65 partials (the second trip of the finalize's lane
# loop), the 512-block cap with a ragged second grid-stride trip
LOSS_S = [1, 255, 2048, 2049, 131073, 1052673]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S,C,B", [(S, 5, 2) for S in LOSS_S] + [(LOSS_S[-1], 2, 1)])
def test_loss_sizes(be, S, C, B, kind):
  logits, gt, w = _loss_inputs(B, C, S, seed=S % 1000 + C)
  _loss_check(be, kind, logits, gt, w, f"S={S} C={C} kind={kind}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [2, 3, 4, 5, 8, 9, 16, 17, 32])
def test_loss_class_counts(be, C, kind):
  """Both ends of every CT instantiation (2, 4, 8, 16, 32 classes in registers), two blocks per sample."""
  logits, gt, w = _loss_inputs(2, C, 2049, seed=50 + C)
  _loss_check(be, kind, logits, gt, w, f"C={C} kind={kind}")


@pytest.mark.parametrize("kind", KINDS)
def test_loss_32_classes_weighted(be, kind):
  logits, gt, w = _loss_inputs(2, 32, 2049, seed=83, weighted=True)
  _loss_check(be, kind, logits, gt, w, f"C=32 weighted kind={kind}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", [1, 17, 64])
def test_loss_batch_sizes(be, B, kind):
  """B = 17: more (sample, quantity) pairs than one round of the finalize's 16 waves; B = 64: the limit."""
  logits, gt, w = _loss_inputs(B, 3, 300, seed=90 + B)
  _loss_check(be, kind, logits, gt, w, f"B={B} kind={kind}")


@pytest.mark.parametrize("S,C,B,weighted", [(2049, 5, 2, False), (131073, 5, 2, True), (1052673, 2, 1, False)])
def test_loss_pass1_partials(be, S, C, B, weighted):
  """The per-block partial sums of the first pass (double [B][nblk][6] at the head of the workspace,
  nblk = min(ceil(S / 2048), 512), block j owning the voxels with (v // 256) % nblk == j), against the per-voxel
  terms in float64: two blocks, 65 blocks, and the 512-block cap with its second grid-stride trip."""
  logits, gt, w = _loss_inputs(B, C, S, seed=S % 1000 + 30, weighted=weighted)
  gt = gt.clone(); gt[0, S // 2] = C; gt[B - 1, S - 1] = -1
  bad = (gt < 0) | (gt >= C)
  g = t.where(bad, t.zeros_like(gt), gt)
  l = logits.double(); wd = t.ones(B, S, dtype=t.float64) if w is None else w.double()
  p = l.softmax(1)
  pfg, gf = p[:, 1:].sum(1), (g >= 1).double()
  hot = F.one_hot(g, C).permute(0, 2, 1)[:, 1:].double()
  ia = (hot * p[:, 1:]).sum(1) * (C - 1) * wd
  ua = (hot * (C - 1) + (1 - hot) * p[:, 1:]).sum(1) * wd
  x = (l.logsumexp(1) - l.gather(1, g[:, None])[:, 0]) * wd
  q = t.stack([t.min(gf, pfg) * wd, t.max(gf, pfg) * wd, ia, ua, x, bad.double()], 2)
  nblk = min(-(-S // 2048), 512)
  want = t.zeros(B, nblk, 6, dtype=t.float64).index_add_(1, (t.arange(S) // 256) % nblk, q)
  _loss_run(be, 1, logits, gt, w)
  got = be.loss_partials(B, C, S, _device()).cpu()
  assert got.shape == want.shape
  err = ((got - want).abs() / want.abs().clamp(min=1.0)).max()
  assert float(err) <= LOSS_RTOL, f"partials: rel err {float(err):.3e}"
  assert t.equal(got[..., 5], want[..., 5])                     # the count of bad labels is exact


def test_loss_batch_65_is_rejected_before_any_launch(be):
  """B = 65 raises, and nothing was launched: loss, dlogits and the workspace (the only memory the first pass
  writes) keep their sentinels."""
  if _SELF:
    pytest.skip("error returns are the library's")
  B, C, S = 65, 3, 300
  logits, gt, _ = _loss_inputs(B, C, S, seed=7)
  lg, gg = logits.to(DEV), gt.to(t.int32).to(DEV)
  loss = t.full((1,), -7.0, device=DEV); dl = t.full((B, C, S), -7.0, device=DEV)
  ws = be.workspace("loss", be.lib.crn_loss_workspace_bytes(B, C), lg.device)
  ws.fill_(0xA5)
  with pytest.raises(_hip_error()):
    be.loss_fwd_bwd(0, lg, gg, B, C, S, loss, dl, 1.0)
  t.cuda.synchronize()
  assert float(loss) == -7.0 and bool((dl == -7.0).all())
  assert bool((ws == 0xA5).all()), "a rejected call wrote its workspace: a kernel was launched"


@functools.lru_cache(maxsize=None)
def _content_case(weighted):
  return _loss_inputs(3, 5, 2049, seed=120 + int(weighted), weighted=weighted)


@pytest.mark.parametrize("kind", KINDS)
def test_loss_zero_weight_sample(be, kind):
  """A sample whose weights are all 0: its unions are 0, so the IoUs divide by 1 and its gradient is zero."""
  logits, gt, w = _content_case(True)
  w = w.clone(); w[1] = 0
  _loss_check(be, kind, logits, gt, w, f"zero-weight sample kind={kind}")
  _, dl = _loss_run(be, kind, logits, gt, w)
  assert float(dl[1].abs().max()) == 0.0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("weighted", [False, True])
def test_loss_uniform_label_samples(be, weighted, kind):
  """One sample all background, one all a single foreground class."""
  logits, gt, w = _content_case(weighted)
  gt = gt.clone(); gt[0] = 0; gt[2] = 3
  _loss_check(be, kind, logits, gt, w, f"uniform labels kind={kind}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("weighted", [False, True])
def test_loss_grad_scale(be, weighted, kind):
  logits, gt, w = _content_case(weighted)
  _, gwant = _loss_ref(kind, logits, gt, w)
  loss1, _ = _loss_run(be, kind, logits, gt, w)
  for gs in (0.125, 1.0 / 3.0):
    loss, dl = _loss_run(be, kind, logits, gt, w, grad_scale=gs)
    close(dl, gwant * gs, GRAD_RTOL, f"grad_scale={gs} kind={kind}")
    assert t.equal(loss, loss1), "grad_scale must not change the loss"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("weighted", [False, True])
def test_loss_saturated_softmax(be, weighted, kind):
  logits, gt, w = _content_case(weighted)
  _loss_check(be, kind, logits * 30, gt, w, f"logits x 30 kind={kind}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("weighted", [False, True])
def test_loss_shift_invariance(be, weighted, kind):
  """+1e4 on every class of every voxel: the result is that of the unshifted logits (lost without the max
  subtraction).  The logits are multiples of 2^-8, so the shifted float32 values are exact (ulp(1e4) = 2^-10)."""
  logits, gt, w = _content_case(weighted)
  logits = (logits * 256).round() / 256
  shifted = logits + 1e4
  assert t.equal(shifted.double(), logits.double() + 1e4)
  _loss_check(be, kind, shifted, gt, w, f"shift 1e4 kind={kind}", logits_ref=logits)


@pytest.mark.parametrize("kind", KINDS)
def test_loss_value_only(be, kind):
  logits, gt, w = _content_case(True)
  want, _ = _loss_ref(kind, logits, gt, w)
  loss, _ = _loss_run(be, kind, logits, gt, w, grad=False)
  assert abs(float(loss) - want) <= LOSS_RTOL * max(1.0, abs(want))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("weighted", [False, True])
def test_loss_labels_out_of_range(be, weighted, kind):
  """Labels -1 and C count as class 0 (value and gradient) and set the status word; the next clean call clears it."""
  logits, gt, w = _content_case(weighted)
  B, C, S = logits.shape
  bad = gt.clone()
  bad[0, 0] = -1; bad[0, 257] = C; bad[1, 2048] = -1; bad[2, 1000] = C; bad[2, 1001] = C + 100
  clean = t.where((bad < 0) | (bad >= C), t.zeros_like(bad), bad)
  _loss_check(be, kind, logits, bad, w, f"bad labels kind={kind}", gt_ref=clean)
  assert be.loss_labels_in_range(B, C, _device()) is False
  _loss_run(be, kind, logits, clean, w)
  assert be.loss_labels_in_range(B, C, _device()) is True


@pytest.mark.parametrize("kind", KINDS)
def test_loss_is_deterministic(be, kind):
  """Fixed-order sums: two runs on the same inputs agree bit for bit (65 partials per sample, weighted)."""
  logits, gt, w = _loss_inputs(2, 5, 131073, seed=140, weighted=True)
  a = _loss_run(be, kind, logits, gt, w)
  b = _loss_run(be, kind, logits, gt, w)
  assert t.equal(a[0], b[0]) and t.equal(a[1], b[1])


# ------------------------------------------------------------------ argmax + confusion matrix (exact)
def _cm_ref(gt, lab, C):
  g = gt.reshape(-1).long(); p = lab.reshape(-1).long()
  ok = (g >= 0) & (g < C)
  return t.bincount(g[ok] * C + p[ok], minlength=C * C)


@pytest.mark.parametrize("C,S,B", [(C, S, 2) for C in (1, 2, 5, 16, 17, 32) for S in (1, 2049)] +
                         [(2, 1052673, 1), (17, 1052673, 1)])
def test_argmax_confusion(be, C, S, B):
  """Logits from {-1, 0, 1}: ties everywhere, the first index wins (torch.argmax's documented rule)."""
  g = t.Generator().manual_seed(C * 7 + S % 100)
  logits = t.randint(-1, 2, (B, C, S), generator=g).float()
  gt = t.randint(0, C, (B, S), generator=g).to(t.int32)
  want = logits.double().argmax(1)
  lg, gg = logits.to(DEV), gt.to(DEV)
  big = (1 << 33) + 5
  # labels and confusion matrix, cm holding values above 2^32
  lab = t.full((B, S), -3, dtype=t.int32, device=DEV)
  cm0 = t.arange(C * C, dtype=t.int64) * 3 + big
  cm = dev(cm0)
  be.argmax_confusion(lg, gg, B, C, S, lab, cm)
  assert t.equal(lab.cpu().long(), want)
  assert cm.dtype == t.int64 and t.equal(cm.cpu(), cm0 + _cm_ref(gt, want, C))
  # labels=None
  cm = dev(cm0)
  be.argmax_confusion(lg, gg, B, C, S, None, cm)
  assert t.equal(cm.cpu(), cm0 + _cm_ref(gt, want, C))
  # gt=None: labels only, cm untouched
  lab = t.full((B, S), -3, dtype=t.int32, device=DEV); cm = dev(cm0)
  be.argmax_confusion(lg, None, B, C, S, lab, cm)
  assert t.equal(lab.cpu().long(), want) and t.equal(cm.cpu(), cm0)
  # gt with -1 and C: skipped in the matrix, the labels are still written
  bad = gt.clone().view(-1)
  pos = t.unique(t.randint(0, B * S, (min(B * S, 9),), generator=g))
  bad[pos[0::2]] = -1; bad[pos[1::2]] = C
  bad = bad.view(B, S)
  n_ok = int(((bad >= 0) & (bad < C)).sum())
  assert n_ok == B * S - pos.numel()
  lab = t.full((B, S), -3, dtype=t.int32, device=DEV); cm = dev(cm0)
  be.argmax_confusion(lg, bad.to(DEV), B, C, S, lab, cm)
  assert t.equal(lab.cpu().long(), want)
  assert int(cm.cpu().sum() - cm0.sum()) == n_ok
  assert t.equal(cm.cpu(), cm0 + _cm_ref(bad, want, C))


# ------------------------------------------------------------------ Adam
# The C ABI takes the scalars as float: the values the kernel works with are the float32 roundings (beta2 = 0.999
# arrives as 0.99900001287..., so 1 - beta2 is 0.99998713e-3, 1.3e-5 off the double 1e-3).  The reference takes
# the same values, in float64 arithmetic.
ADAM = {k: float(np.float32(v)) for k, v in dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-4, gs=0.37).items()}
# Measured on a CPU on the inputs of test_adam_step (10 steps, every n below): float32 torch.optim.Adam deviates
# from the float64 update by at most 2.3e-7 (p), 1.3e-7 (m), 2.5e-7 (v), each as max-abs-err / max-abs.  4x that is below
# the project's floor for Adam (1e-6, test_argmax_confusion_and_adam), so the floor is the tolerance.
ADAM_RTOL = 1e-6
ADAM_N = [1, 3, 4, 5, 1003, 8388608 + 7]     # n < 4 (tail only), n % 4 != 0, the 8192-block cap and its grid stride


def _adam_grad(n, step, g):
  """A fresh gradient per step; elements 0, 3, 6, .. are exactly 0 in the first three steps (v = 0: the denominator
  is eps), elements 1, 4 (mod 6) in every step."""
  gr = t.randn(n, generator=g)
  i = t.arange(n)
  if step <= 3:
    gr[i % 3 == 0] = 0
  gr[i % 6 == 1] = 0
  return gr


def _adam_ref(p, m, v, gr, step):
  """torch.optim.Adam's update (amsgrad off, no weight decay) written out in float64, in place."""
  lr, b1, b2, eps, gs = (ADAM[k] for k in ("lr", "b1", "b2", "eps", "gs"))
  gg = gr.double() * gs
  m.mul_(b1).add_(gg, alpha=1 - b1)
  v.mul_(b2).addcmul_(gg, gg, value=1 - b2)
  denom = v.sqrt() / np.sqrt(1 - b2 ** step) + eps
  p.addcdiv_(m, denom, value=-lr / (1 - b1 ** step))


@pytest.mark.parametrize("n", ADAM_N)
def test_adam_step(be, n):
  g = t.Generator().manual_seed(n % 1000)
  p0 = t.randn(n, generator=g)
  pr, mr, vr = p0.double(), t.zeros(n, dtype=t.float64), t.zeros(n, dtype=t.float64)
  pg, mg, vg = dev(p0), t.zeros(n, device=DEV), t.zeros(n, device=DEV)
  for step in range(1, 11):
    gr = _adam_grad(n, step, g)
    _adam_ref(pr, mr, vr, gr, step)
    be.adam_step(pg, gr.to(DEV), mg, vg, n, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["gs"], step)
  close(pg, pr, ADAM_RTOL, f"adam p n={n}")
  close(mg, mr, ADAM_RTOL, f"adam m n={n}")
  close(vg, vr, ADAM_RTOL, f"adam v n={n}")
  always0 = t.arange(n) % 6 == 1
  assert t.equal(pg.cpu()[always0], p0[always0]), "zero gradient, zero moments: the parameter must not move"


@pytest.mark.parametrize("n", ADAM_N)
def test_adam_step_hyper_equals_adam_step(be, n):
  """crn_adam_set_hyper + crn_adam_step_hyper (the captured-graph variant) against crn_adam_step with the same
  scalars: bit for bit on p, m, v; the second copy lives in a slice of a larger buffer at a 16-byte-aligned offset,
  as the bucketed step has it."""
  g = t.Generator().manual_seed(n % 1000 + 1)
  p0 = t.randn(n, generator=g)
  off = 12                                                        # floats: 48 bytes
  pa, ma, va = dev(p0), t.zeros(n, device=DEV), t.zeros(n, device=DEV)
  bufs = [t.full((n + 40,), 5.0, device=DEV) for _ in range(4)]
  pb, mb, vb, gb = [b[off:off + n] for b in bufs]
  pb.copy_(p0); mb.zero_(); vb.zero_()
  hyper = t.zeros(8, device=DEV)
  for step in range(1, 4):
    gr = _adam_grad(n, step + 2, g)
    be.adam_step(pa, gr.to(DEV), ma, va, n, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["gs"], step)
    gb.copy_(gr)
    be.adam_set_hyper(hyper, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["gs"], step)
    be.adam_step_hyper(pb, gb, mb, vb, n, hyper)
  for a, b, name in ((pa, pb, "p"), (ma, mb, "m"), (va, vb, "v")):
    if _SELF:
      close(b, a, ADAM_RTOL, name)        # (the emulator keeps the scalars of adam_step in double)
    else:
      assert t.equal(a, b), name
  for b in bufs:                          # nothing outside the slice was written
    assert bool((b[:off] == 5.0).all()) and bool((b[off + n:] == 5.0).all())


def test_adam_rejects_misaligned_pointers_and_step_0(be):
  if _SELF:
    pytest.skip("error returns are the library's")
  HipError = _hip_error()
  n = 1003
  g = t.Generator().manual_seed(3)
  host = [t.randn(n + 4, generator=g) for _ in range(4)]
  host[3].abs_()
  bufs = [dev(h) for h in host]
  hyper = t.full((8,), 2.5, device=DEV)
  be.adam_set_hyper(hyper, 1e-3, 0.9, 0.999, 1e-4, 1.0, 1)
  h0 = hyper.clone()

  def unchanged():
    t.cuda.synchronize()
    return all(t.equal(b.cpu(), h) for b, h in zip(bufs, host))

  for k in range(4):                      # each of param, grad, exp_avg, exp_avg_sq one float off 16-byte alignment
    args = [b[1:n + 1] if i == k else b[:n] for i, b in enumerate(bufs)]
    p, gr, m, v = args
    with pytest.raises(HipError):
      be.adam_step(p, gr, m, v, n, 1e-3, 0.9, 0.999, 1e-4, 1.0, 1)
    with pytest.raises(HipError):
      be.adam_step_hyper(p, gr, m, v, n, hyper)
    assert unchanged()
  p, gr, m, v = [b[:n] for b in bufs]
  with pytest.raises(HipError):
    be.adam_step(p, gr, m, v, n, 1e-3, 0.9, 0.999, 1e-4, 1.0, 0)
  assert unchanged()
  with pytest.raises(HipError):
    be.adam_set_hyper(hyper, 1e-3, 0.9, 0.999, 1e-4, 1.0, 0)
  t.cuda.synchronize()
  assert t.equal(hyper, h0)


# ------------------------------------------------------------------ encoder head
MEAN = (103.939, 116.779, 123.68)


@pytest.mark.parametrize("B,H,W,byte_off", [(3, 5, 7, 0), (1, 1, 1, 0), (2, 12, 20, 0), (2, 12, 20, 1), (3, 5, 7, 1)])
def test_preprocess(be, B, H, W, byte_off):
  """u8 RGB -> float32 BGR + mean, one float32 add per element: exact.  H*W % 4 != 0 and a view that starts one
  byte into its storage take the scalar kernel, (2, 12, 20) at offset 0 the four-pixel one."""
  g = t.Generator().manual_seed(B * 100 + H)
  n = B * 3 * H * W
  store = t.randint(0, 256, (n + byte_off,), generator=g, dtype=t.uint8)
  store[byte_off] = 0; store[-1] = 255
  if n > 8: store[byte_off + 5] = 255; store[byte_off + 6] = 0
  img = store[byte_off:].view(B, 3, H, W)
  want = img[:, [2, 1, 0]].float() + t.tensor(MEAN, dtype=t.float32).view(1, 3, 1, 1)
  sg = store.to(DEV)
  ig = sg[byte_off:].view(B, 3, H, W)
  assert _SELF or ig.data_ptr() % 4 == byte_off
  out = t.full((B, 3, H, W), -1.0, device=DEV)
  be.preprocess(ig, out)
  assert t.equal(out.cpu(), want)


def _maxpool_inputs(B, C, H, W, seed):
  """Exact arithmetic: per plane a random permutation of distinct multiples of 2^-6, scale in +-{0.5, 1, 2}, shift a
  multiple of 2^-4.  Channel 0 has a negative scale; channel 1 is shifted so that every activation is <= 0 (its
  largest is exactly 0)."""
  g = t.Generator().manual_seed(seed)
  hw = H * W
  x = t.stack([t.randperm(hw, generator=g) for _ in range(B * C)]).view(B, C, H, W)
  x = (x - hw // 2).float() / 64
  sc = t.tensor([0.5, 1.0, 2.0])[t.randint(0, 3, (C,), generator=g)] * (t.randint(0, 2, (C,), generator=g) * 2 - 1).float()
  sh = t.randint(-8, 9, (C,), generator=g).float() / 16
  sc[0] = -sc[0].abs(); sh[0] = 0.25
  sc[1] = 1.0; sh[1] = -float(x.max())
  return x, sc, sh


@pytest.mark.parametrize("B,C,H,W", [(2, 8, 16, 16), (2, 3, 7, 9), (1, 2, 1, 1), (1, 2, 2, 3), (1, 64, 112, 112)])
def test_maxpool_fwd_bwd(be, B, C, H, W):
  """y, argmax and dx bit-equal to float64 autograd through affine -> ReLU -> ZeroPad2d(1) -> max_pool2d(3, 2);
  dx is the gradient of the scaled-and-shifted, pre-ReLU input."""
  x, sc, sh = _maxpool_inputs(B, C, H, W, seed=H * 10 + W)
  Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
  g = t.Generator().manual_seed(1)
  dy = t.randint(-16, 17, (B, C, Ho, Wo), generator=g).float() / 16
  a = (x.double() * sc.double().view(1, C, 1, 1) + sh.double().view(1, C, 1, 1)).requires_grad_(True)
  assert t.equal(a.detach().float().double(), a.detach())                   # exact in float32
  yr, idx = F.max_pool2d(F.pad(a.relu(), [1, 1, 1, 1]), 3, 2, return_indices=True)
  assert yr.shape == (B, C, Ho, Wo)
  yr.backward(dy.double())
  ih, iw = idx // (W + 2) - 1, idx % (W + 2) - 1
  amr = t.where(yr > 0, ih * W + iw, t.full_like(idx, -1))                  # a zero maximum carries no gradient
  assert bool((a.detach()[:, 1] <= 0).all()) and bool((amr[:, 1] == -1).all()) and bool((amr[:, 0] >= 0).any() or H * W == 1)

  y = t.full((B, C, Ho, Wo), -1.0, device=DEV); am = t.full((B, C, Ho, Wo), -9, dtype=t.int32, device=DEV)
  be.maxpool_fwd(x.to(DEV), sc.to(DEV), sh.to(DEV), B, C, H, W, y, am)
  exact(y, yr.detach(), "maxpool y")
  assert t.equal(am.cpu().long(), amr), "maxpool argmax"
  dx = t.full((B, C, H, W), -1.0, device=DEV)
  be.maxpool_bwd(dy.to(DEV), am, B, C, H, W, dx)
  exact(dx, a.grad, "maxpool dx")
  assert float(dx[:, 1].abs().max()) == 0.0


@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("S", [1, 49, 64, 65, 4096])
def test_relu_mean_fwd_bwd(be, S, C):
  """x and dx are channel slices of wider buffers with different batch strides; S below, at and above the 64
  lanes of the wave that owns a channel."""
  B, c0, Cx, Cd, d0 = 2, 2, C + 5, C + 3, 1
  g = t.Generator().manual_seed(S + C)
  xb = t.randn(B, Cx, S, generator=g)
  xb[0, c0, 0] = 0.0                                            # relu'(0) = 0
  davg = t.randn(B, C, generator=g)
  x = xb[:, c0:c0 + C]
  want_avg = x.double().relu().mean(2)
  want_g = (x.double() > 0) * (davg.double().view(B, C, 1) / S)
  xg = xb.to(DEV)
  avg = t.full((B, C), -7.0, device=DEV)
  be.relu_mean_fwd(xg[:, c0:c0 + C], B, C, S, Cx * S, avg)
  close(avg, want_avg, 1e-6, "relu_mean_fwd")
  for accumulate in (False, True):
    d0b = t.randn(B, Cd, S, generator=g)
    dg = dev(d0b)
    be.relu_mean_bwd(xg[:, c0:c0 + C], davg.to(DEV), B, C, S, Cx * S, dg[:, d0:d0 + C], Cd * S, accumulate)
    want = d0b.double().clone()
    want[:, d0:d0 + C] = want_g + (want[:, d0:d0 + C] if accumulate else 0)
    close(dg[:, d0:d0 + C], want[:, d0:d0 + C], 1e-6, f"relu_mean_bwd accumulate={accumulate}")
    keep = t.ones(Cd, dtype=t.bool); keep[d0:d0 + C] = False
    assert t.equal(dg.cpu()[:, keep], d0b[:, keep]), "channels around the slice were written"


LINEAR_CASES = [(1, 1, 1, 1), (3, 63, 7, 7), (2, 65, 130, 133), (4, 2048, 64, 67)]      # (B, K, N, ld)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("B,K,N,ld", LINEAR_CASES)
def test_linear_fwd(be, B, K, N, ld, bias):
  g = t.Generator().manual_seed(K + N)
  x = t.randn(B, K, generator=g); w = t.randn(N, K, generator=g) / np.sqrt(K)
  b = t.randn(N, generator=g) if bias else None
  want = x.double() @ w.double().t() + (b.double() if bias else 0)
  y = t.full((B, ld), -7.0, device=DEV)
  be.linear_fwd(x.to(DEV), w.to(DEV), None if b is None else b.to(DEV), B, K, N, y, ld)
  close(y[:, :N], want, 2e-5, "linear_fwd")
  assert bool((y[:, N:] == -7.0).all()), "columns [N, ld) were written"


@pytest.mark.parametrize("has_dx,has_dw,has_db", [(a, b, c) for a in (1, 0) for b in (1, 0) for c in (1, 0)])
@pytest.mark.parametrize("B,K,N,ld", LINEAR_CASES)
def test_linear_bwd(be, B, K, N, ld, has_dx, has_dw, has_db):
  """Every combination of dx / dw / db given or None: each one given is written, whichever others are."""
  g = t.Generator().manual_seed(K + N + 1)
  x = t.randn(B, K, generator=g); w = t.randn(N, K, generator=g) / np.sqrt(K)
  dyb = t.randn(B, ld, generator=g)                             # dy: the first N columns of rows of length ld
  dy = dyb[:, :N].double()
  dx = t.full((B, K), -7.0, device=DEV) if has_dx else None
  dw = t.full((N, K), -7.0, device=DEV) if has_dw else None
  db = t.full((N,), -7.0, device=DEV) if has_db else None
  be.linear_bwd(x.to(DEV), w.to(DEV), dyb.to(DEV), ld, B, K, N, dx, dw, db)
  if has_dx: close(dx, dy @ w.double(), 2e-5, "linear_bwd dx")
  if has_dw: close(dw, dy.t() @ x.double(), 2e-5, "linear_bwd dw")
  if has_db: close(db, dy.sum(0), 2e-5, f"linear_bwd db (dw {'given' if has_dw else 'None'})")


# (B, C, S, slice): B*S <= 65536 -> one owner workgroup per channel; above it partial sums + final, float4 where S,
# the batch stride and the pointer allow it, scalar otherwise
BIAS_CASES = [(2, 6, 100, False), (2, 3, 40000, False), (2, 3, 40001, False), (64, 2, 1100, False), (2, 3, 40000, True)]


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("B,C,S,sliced", BIAS_CASES)
def test_bias_grad(be, B, C, S, sliced, accumulate):
  g = t.Generator().manual_seed(S % 1000 + B)
  if sliced:                                                    # a channel slice whose batch stride is no multiple of 4
    sB = 5 * S + 3
    store = t.randn(B * sB, generator=g)
    view = lambda s: t.as_strided(s, (B, C, S), (sB, S, 1), S)
  else:
    sB = C * S
    store = t.randn(B, C, S, generator=g)
    view = lambda s: s
  store += 0.25                                                 # a sum that does not cancel to nothing
  db0 = t.randn(C, generator=g) * 50
  want = view(store).double().sum((0, 2)) + (db0.double() if accumulate else 0)
  sg = store.to(DEV); db = dev(db0)
  be.bias_grad(view(sg), B, C, S, sB, db, accumulate)
  close(db, want, 1e-6, "bias_grad")


def test_bias_grad_rejects_batch_65(be):
  if _SELF:
    pytest.skip("error returns are the library's")
  dy = t.zeros(65, 2, 8, device=DEV); db = t.full((2,), -7.0, device=DEV)
  with pytest.raises(_hip_error()):
    be.bias_grad(dy, 65, 2, 8, 16, db)
  t.cuda.synchronize()
  assert bool((db == -7.0).all())


def test_gather_scatter_past_the_block_cap(be):
  """n = 2^20 + 300: past the 4096-block cap, so the grid-stride loop makes a ragged second trip.  Integer-valued
  floats: every result is exact."""
  n = (1 << 20) + 300
  g = t.Generator().manual_seed(11)
  perm = t.randperm(n, generator=g)
  holes = t.randint(0, n, (1000,), generator=g)
  idx = perm.clone(); idx[holes] = -1
  idx[0] = -1; idx[n - 1] = -1
  valid = idx >= 0
  src = t.randint(-1000, 1000, (n,), generator=g).float()
  ig, sg = idx.to(t.int32).to(DEV), src.to(DEV)
  dst = t.full((n,), -7.0, device=DEV)
  be.gather(sg, ig, dst)
  want = t.where(valid, src.double()[idx.clamp(min=0)], t.zeros((), dtype=t.float64))
  exact(dst, want, "gather")
  for accumulate in (False, True):
    d0 = t.randint(-1000, 1000, (n,), generator=g).float()
    want = d0.double().clone()
    if accumulate: want[idx[valid]] += src.double()[valid]
    else: want[idx[valid]] = src.double()[valid]
    dst = dev(d0)
    be.scatter(sg, ig, dst, accumulate)
    exact(dst, want, f"scatter accumulate={accumulate}")


def test_fill_offset_channels(be):
  B, Cx, S, c0 = 3, 9, 37, 4
  g = t.Generator().manual_seed(12)
  off = t.rand(B, 3, generator=g)
  x0 = t.randn(B, Cx, S, generator=g)
  xg = dev(x0)
  be.fill_offset_channels(xg, B, Cx * S, S, c0, off.to(DEV))
  want = x0.clone(); want[:, c0:c0 + 3] = off.view(B, 3, 1)
  assert t.equal(xg.cpu(), want)


@pytest.mark.parametrize("n", [1, 300])
def test_add_i64(be, n):
  g = t.Generator().manual_seed(n)
  p0 = t.randint(1 << 33, 1 << 40, (n,), generator=g, dtype=t.int64)
  inc = (1 << 35) + 12345
  p = t.cat([p0, t.tensor([-1])]).to(DEV)                       # one element past n keeps its value
  be.add_i64(p, n, inc)
  assert t.equal(p.cpu()[:n], p0 + inc) and int(p[n]) == -1
