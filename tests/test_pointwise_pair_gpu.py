"""crn_conv1x1_fwd_pair (csrc/conv_igemm.hip): two pointwise convolutions onto one output in one launch,
  y[b, n, s] (+)= sum_{c < C1} w1[c, n] x1[b, c, s] + sum_{c < C2} w2[c, n] x2[b, c, s],
against the same sum in float64 on the host.  Error measure and bar are those of the fp32 pointwise rows of
tests/conv_fp32_cases.py (err_inside in units of max |reference of what the call computes|, BAR_FWD).  The summation order
differs from two accumulating launches by design, so nothing here is compared bit for bit with that path.

Shapes: the smallest at which the kernel can go wrong.  It walks K in chunks of 64 through two prefetch slots and switches
source at C1 (a multiple of 64); a workgroup owns 64 positions x 32 columns; a split owns a multiple of 64 channels."""
import numpy as np
import pytest
import torch as t

from corenet_amd import views as V
from conv_fp32_cases import BAR_FWD, SENTINEL, err_inside, outside_equal

pytestmark = pytest.mark.gpu

GUARD = 2            # channels of sentinel behind the N output channels of every sample


@pytest.fixture(scope="module")
def be():
  from corenet_amd.backend import HipBackend
  assert t.cuda.is_available(), "gpu tests need an MI355X"
  return HipBackend()


def _plain(st, B, C, dims, sB=None):
  D, H, W = dims
  return V.View(st, 0, B, C, D, H, W, C * D * H * W if sB is None else sB, D * H * W, H * W, W, 1)


# name: (B, C1, C2, N, dims, splits, batch pad of x2 in floats)
CASES = {
    "one_chunk_each": (1, 64, 64, 32, (1, 8, 8), 1, 0),            # the boundary falls between the two prefetch slots
    "odd_chunks_then_switch_64_128": (1, 64, 128, 32, (1, 8, 8), 1, 0),   # slot parity flips at the switch
    "odd_chunks_then_switch_192_64": (1, 192, 64, 32, (1, 8, 8), 1, 0),
    "k448_splits1": (1, 128, 320, 32, (1, 8, 8), 1, 0),
    "k448_splits2": (1, 128, 320, 32, (1, 8, 8), 2, 0),            # 256 channels per split: the boundary lies behind C1
    "k448_splits3": (1, 128, 320, 32, (1, 8, 8), 3, 0),            # 192 per split
    "k448_splits4": (1, 128, 320, 32, (1, 8, 8), 4, 0),            # 128 per split: a boundary ON C1
    "k448_splits7": (1, 128, 320, 32, (1, 8, 8), 7, 0),            # 64 per split: a boundary in front of C1, one chunk per split
    "k448_auto": (1, 128, 320, 32, (1, 8, 8), 0, 0),               # the launch's own split rule (few blocks, long K)
    "n48": (1, 64, 64, 48, (1, 8, 8), 1, 0),                       # Npad 48: the column guard of the second 32-column block
    "s36_b2": (2, 64, 64, 32, (1, 6, 6), 1, 0),                    # no full position tile
    "s100_b2": (2, 64, 128, 32, (1, 10, 10), 2, 0),                # a full and a partial tile, two samples, split
    "x2_batch_strided": (2, 64, 64, 32, (1, 6, 6), 1, 8),          # the second source's own batch stride
}


def _inputs(name):
  B, C1, C2, N, dims, splits, pad2 = CASES[name]
  S = dims[0] * dims[1] * dims[2]
  g = t.Generator().manual_seed(sum(map(ord, name)))
  npad = (N + 15) // 16 * 16
  x1 = t.randn(B, C1, S, generator=g)
  x2 = t.randn(B, C2, S, generator=g)
  w1 = t.zeros(C1, npad); w1[:, :N] = t.randn(C1, N, generator=g) / np.sqrt(C1 + C2)
  w2 = t.zeros(C2, npad); w2[:, :N] = t.randn(C2, N, generator=g) / np.sqrt(C1 + C2)
  y0 = t.randn(B, N + GUARD, S, generator=g)
  ref = (t.einsum("cn,bcs->bns", w1[:, :N].double(), x1.double()) + t.einsum("cn,bcs->bns", w2[:, :N].double(), x2.double()))
  return B, C1, C2, N, npad, dims, S, splits, pad2, x1, x2, w1, w2, y0, ref


_REF = {}


def _case(name):
  if name not in _REF:
    _REF[name] = _inputs(name)
  return _REF[name]


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_pair_against_float64(be, name, accumulate):
  B, C1, C2, N, npad, dims, S, splits, pad2, x1, x2, w1, w2, y0, ref = _case(name)
  dev = "cuda"
  x1s = x1.reshape(-1).to(dev)
  sB2 = C2 * S + pad2
  x2h = t.full((B, sB2), 7.0)
  x2h[:, :C2 * S] = x2.reshape(B, -1)
  x2s = x2h.reshape(-1).to(dev)
  yh = y0.clone() if accumulate else t.full_like(y0, SENTINEL)
  ys = yh.reshape(-1).to(dev)
  mask = t.zeros(B, N + GUARD, S, dtype=t.bool)
  mask[:, :N] = True
  ok = be.conv1x1_pair(_plain(x1s, B, C1, dims), w1.to(dev), _plain(x2s, B, C2, dims, sB=sB2), w2.to(dev), npad,
                       _plain(ys, B, N, dims, sB=(N + GUARD) * S), splits, accumulate)
  assert ok, "the entry rejected a shape it documents as covered"
  got = ys.cpu().reshape(B, N + GUARD, S)
  want = t.zeros(B, N + GUARD, S, dtype=t.float64)
  want[:, :N] = ref + (yh[:, :N].double() if accumulate else 0.0)
  err = err_inside(got, want, mask, float(ref.abs().max()))
  print(f"{name} accumulate={accumulate}: {err:.3e} of max|ref| (bar {BAR_FWD})")
  assert outside_equal(got.reshape(-1), yh.reshape(-1), mask.reshape(-1)), f"{name}: elements outside [0, N) x [0, S) changed"
  assert err <= BAR_FWD, f"{name}: {err:.3e} of max|ref| > {BAR_FWD}"


def test_pending_sum_of_a_split_pair_is_flushed_by_the_next_entry(be):
  """A split pair armed with crn_splitk_defer leaves ONE pending sum like a single pointwise launch: the next entry point of
  the library completes it, and y then holds the reference."""
  B, C1, C2, N, npad, dims, S, splits, pad2, x1, x2, w1, w2, y0, ref = _case("k448_splits3")
  dev = "cuda"
  ys = t.full((B * N * S,), SENTINEL, device=dev)
  be.splitk_defer()
  assert be.conv1x1_pair(_plain(x1.reshape(-1).to(dev), B, C1, dims), w1.to(dev), _plain(x2.reshape(-1).to(dev), B, C2, dims),
                         w2.to(dev), npad, _plain(ys, B, N, dims), splits, False)
  # the next producer flushes before it uses the scratch itself: the same pair again, split, onto a second output
  y2 = t.full((B * N * S,), SENTINEL, device=dev)
  assert be.conv1x1_pair(_plain(x1.reshape(-1).to(dev), B, C1, dims), w1.to(dev), _plain(x2.reshape(-1).to(dev), B, C2, dims),
                         w2.to(dev), npad, _plain(y2, B, N, dims), splits, False)
  for y in (ys, y2):
    err = err_inside(y.cpu().reshape(B, N, S), ref, t.ones(B, N, S, dtype=t.bool), float(ref.abs().max()))
    assert err <= BAR_FWD, err


@pytest.mark.parametrize("what", ["c1_32", "different_s", "x2_not_plain", "x1_not_plain"])
def test_rejected_pairs_launch_nothing(be, what):
  """CRN_EINVAL before anything is written or launched: the output keeps its sentinel."""
  dev = "cuda"
  B, N, dims = 2, 32, (1, 6, 6)
  S = 36
  C1 = 32 if what == "c1_32" else 64
  C2 = 64
  d2 = (1, 6, 8) if what == "different_s" else dims
  S2 = d2[1] * d2[2]
  x1s = t.randn(B * (C1 * S + 2), device=dev)
  x2s = t.randn(B * (C2 * S2 + 2), device=dev)
  # a batch stride of 2 mod 4 floats: not a plain view (no 16-byte alignment of the second sample)
  x1v = _plain(x1s, B, C1, dims, sB=C1 * S + (2 if what == "x1_not_plain" else 0))
  x2v = _plain(x2s, B, C2, d2, sB=C2 * S2 + (2 if what == "x2_not_plain" else 0))
  ys = t.full((B * N * S,), SENTINEL, device=dev)
  w1, w2 = t.randn(C1, N, device=dev), t.randn(C2, N, device=dev)
  for accumulate in (False, True):
    assert not be.conv1x1_pair(x1v, w1, x2v, w2, N, _plain(ys, B, N, dims), 0, accumulate)
  t.cuda.synchronize()
  assert bool((ys == SENTINEL).all())


@pytest.mark.parametrize("hw,expect", [(64, [True] * 4), (32, [False, True, True, True])], ids=["64x64", "32x32_stage5_falls_back"])
def test_train_step_with_and_without_the_pair_entry(hw, expect):
  """One fused training step of CoreNet (B = 2) with the data gradients of the four down-sampling bottlenecks on the pair
  entry, and the same step from the same state with the entry masked off on the backend object (two launches per block, as
  before).  The pair changes gradients UPSTREAM of each block, so every parameter gradient is compared, the four blocks'
  own included, with the measure of test_model_gpu.test_all_parameter_gradients_against_fp64_truth (the (1 - 1/128)
  quantile of |a - b| / scale over the same strided sub-sample, scale = max(tensor max, 1e-3 of the largest gradient)) against
  the SMALLEST bar that test ever grants: GRAD_MODE_FACTOR x GRAD_ERR_FLOOR, without its noise term (2e-2 for tensors whose
  true gradient is zero, as there), single elements within GRAD_OUTLIER_CAP.  Deterministic mode, so that the summation
  order inside the pair is the only difference between the two runs.
  Image 64 x 64: the smallest at which all four blocks take the entry.  32 x 32, the smallest image the plan accepts: stage 5
  (the first block backward reaches) has ONE position per sample, the entry needs S % 4 == 0 and returns CRN_EINVAL, and the
  engine issues that block's two launches as before -- its fall-back inside a real step."""
  import test_model_gpu as TM
  from oracle import corenet_oracle as O
  from corenet_amd.backend import default_backend
  math = "bf16x3"
  be = default_backend()
  sd = O.make_state(0, 2, nbt=30000)
  _, v2s, off, grid = [x.cuda() for x in O.synthetic_batch(2, 0, 2)]
  image = t.randint(0, 256, (2, 3, hw, hw), generator=t.Generator().manual_seed(hw), dtype=t.uint8).cuda()
  gi = grid.to(t.int32)
  taken = []
  real = be.conv1x1_pair

  def counting(*a, **k):
    taken.append(real(*a, **k))
    return taken[-1]

  def run(entry):
    be.conv1x1_pair = entry
    m = TM._model(2, sd, math).train()
    m.train_step(image, v2s, off, gi, "iou_fgbg", lr=4e-4, adam_eps=1e-4, graph=False)
    t.cuda.synchronize()
    st = m.engine.store
    return {k: st.view(k, grad=True).clone() for k in st.off if st.kind[k] == "param"}

  try:
    be.set_deterministic(True)
    ga = run(counting)
    gb = run(None)
  finally:
    be.set_deterministic(False)
    del be.conv1x1_pair               # (the instance attribute: the class's method is back)
  assert taken == expect, taken
  down = [k for k in ga if any(k.startswith(f"encoder.stage{s}.a.") for s in "2345")]
  assert len(down) >= 4 * 4, down
  gmax = max(float(v.abs().max()) for v in gb.values())
  floor_bar = TM.GRAD_MODE_FACTOR[math] * TM.GRAD_ERR_FLOOR
  rows = []
  for k in ga:
    a, b = ga[k].reshape(-1), gb[k].reshape(-1)
    step = max(1, -(-a.numel() // 512))
    a, b = a[::step].double().cpu(), b[::step].double().cpu()
    tmax = float(gb[k].abs().max())
    scale = max(tmax, 1e-3 * gmax)
    e = ((a - b).abs() / scale).sort().values
    kq = max(1, e.numel() // 128)
    err, worst = float(e[-(kq + 1)]) if e.numel() > kq else 0.0, float(e[-1])
    bar = max(floor_bar, 2e-2) if tmax < 1e-3 * gmax else floor_bar
    rows.append((err / bar, err, worst, k))
  rows.sort(reverse=True)
  print("pair vs two launches, worst tensors (error / bar, error, largest element, name):", rows[:4])
  assert rows[0][0] <= 1.0, rows[:4]
  assert max(r[2] for r in rows) <= TM.GRAD_OUTLIER_CAP, sorted(rows, key=lambda r: -r[2])[:3]
