"""CPU side of tests/convt_par_cases.py (the parity-walk kernels of csrc/convt_par.hip): the four weight-image tables of
conv_geometry against the walk model, the share of the bars that belongs to the references, the kernel bugs the bars catch, what
the table reaches, and the host loops of the persistent kernels mirrored in Python.  No GPU."""
import functools

import pytest
import torch as t
import torch.nn.functional as F

import convt_par_cases as K
from convt_par_cases import CASES, BAR, SPLIT_BAR, SPLIT_MAX_F32, PARITIES
from conv_fp32_cases import err_inside
from kernel_contract_emu import EmuBackend
from corenet_amd.model import conv_geometry as G

EMU = EmuBackend()
NUMERIC = [c for c in CASES if c.op != "ximage"]


@functools.lru_cache(maxsize=None)
def built(name):
  return K.build(K.BY_NAME[name])


@functools.lru_cache(maxsize=None)
def ref_of(name):
  return K.Ref(built(name), f32=True)


# ------------------------------------------------------------------------------------------------ the tables
TABLES = [("walk_fwd", G.convt_par_fwd_table, "fwd", False, (1, 2, 8, 9, 14, 16)),
          ("walk_dgrad", G.convt_par_dgrad_table, "dgrad", False, (1, 2, 8, 9, 14, 16)),
          ("res_fwd", G.convt_res_fwd_table, "fwd", True, (2,)),
          ("res_dgrad", G.convt_res_dgrad_table, "dgrad", True, (1, 2))]


@pytest.mark.parametrize("name,cout", [(tb[0], n) for tb in TABLES for n in tb[4]])
def test_table_builds_the_image_the_kernel_walks(name, cout):
  """The image a table function gathers out of a parameter slab (weights at a non-zero offset), walked the way the kernel's
  comments say the kernel does and multiplied with an unsplit float64 input, is the float64 reference of hi + lo of the weights,
  to float64 rounding; and every element the walk never uses for a real output (taps with k < 0, columns n >= cout) is zero."""
  _, fn, op, resident, _ = next(tb for tb in TABLES if tb[0] == name)
  wofs = 53
  b = K.build(K.Case(f"table_{name}_{cout}", op, resident=resident, cout=cout, B=2, dims=(4, 8, 16), tr="both", bias=False))
  g = t.Generator().manual_seed(cout)
  params = t.cat([t.randn(wofs, generator=g), b.w.reshape(-1), t.randn(7, generator=g)])
  tab, nbytes = fn(b.wshape, wofs)
  img = t.zeros(nbytes, dtype=t.uint8)
  EMU.bf3_gather_image(params, t.as_tensor(tab), img)
  wd = K.windows_of(b, img)
  hi, lo = K._split(b.w)
  w_hl = hi.double() + lo.double()
  if op == "fwd":
    got, want = K.walk_fwd(b, wd, split=False), K.ref_fwd(b, w_hl)
  else:
    got, want = K.walk_dgrad(b, wd, split=False), K.ref_dgrad(b, w_hl)
  err = float((got - want).abs().max() / want.abs().max())
  assert err <= 1e-13, f"{name} cout {cout}: the walk over the image is {err:.2e} of the range from the float64 reference"
  assert wd.unread_max() == 0.0, f"{name} cout {cout}: an image element the walk has no use for is not zero"
  # ... and which half of an entry pair is hi and which lo: the three products of the split operands, term by term, on doubles
  if op == "fwd":
    oh, ol = K._split(K._crop(K._transformed(b, K.x_logical(b, t.float32))))
    f = lambda a, w: F.conv_transpose3d(a.double(), w.double(), None, stride=2, padding=3, output_padding=1)
    got = K.walk_fwd(b, wd)
  else:
    oh, ol = K._split(K.dy_logical(b, t.float32))
    f = lambda a, w: F.conv3d(a.double(), w.double(), stride=2, padding=3)
    got = K.walk_dgrad(b, wd)
  want = f(oh, hi) + f(oh, lo) + f(ol, hi)
  err = float((got - want).abs().max() / want.abs().max())
  assert err <= 1e-13, f"{name} cout {cout}: hi*hi + hi*lo + lo*hi over the image is {err:.2e} of the range from the same sum over the split weights"
  assert bool(wd.read.any(1).sum() > 0)


def test_packed_gradient_geometry_is_the_layers():
  """The real entries of the packed weight gradient as the kernel's comment has them (pair (rd, rh) owns planes zd < 3 + rd, rows
  zh < 3 + rh, column block rw the taps zw < 3 + rw) are those of conv_geometry.convt_fwd, at every Npad of the table."""
  for c in CASES:
    if c.op != "wgrad": continue
    b = built(c.name)
    assert t.equal(K.packed_index(b) >= 0, K.wgrad_real(c.cout, c.Npad)), c.name


# ------------------------------------------------------------------------------------------------ the host loops
def test_rows_get_the_tile_walks_they_name():
  """launch_res and the deal of crn_convt_s2k7_wgrad_bf3, mirrored in Python: a retune of a cost constant or of the workgroup count
  moves a row off the walk it is there for and fails here."""
  for c in CASES:
    if not c.expect: continue
    if c.op == "wgrad":
      per, end = K.wgrad_deal(K.tiles_of(c))
      assert dict(ntiles=K.tiles_of(c), tiles_per_wg=per, wg_end=end) == c.expect, c.name
    else:
      per, wgs = K.res_deal(K.tiles_of(c))
      assert dict(tiles=K.tiles_of(c), per=per, wgs=wgs) == c.expect, c.name
  # the mirror itself against the numbers the header of the issue's shapes give: 64^3 at B 2 and B 4
  assert K.res_deal(1024) == (4, 256) and K.res_deal(256) == (1, 256) and K.res_deal(257) == (2, 129)
  assert K.wgrad_deal(1) == ((1, 1, 1, 1), (1, 2, 3, 4))


# ------------------------------------------------------------------------------------------------ the references
def test_reference_share_of_the_bars():
  """On every row the walk model (exact products of the split operands, summed in float64) is within half of the 2e-5 bar of the
  float64 reference: the other half belongs to the kernel's float32 accumulation.  And the constant behind the sharper bar is what
  this table measures: the largest float32-versus-float64 summation difference of the walk model over all rows."""
  worst, worst_row, share = 0.0, None, [1.0, 0.0, None]
  print()
  for c in NUMERIC:
    r = ref_of(c.name)
    if r.f32_vs_split > worst: worst, worst_row = r.f32_vs_split, c.name
    share[0] = min(share[0], r.split_vs_f64)
    if r.split_vs_f64 > share[1]: share[1], share[2] = r.split_vs_f64, c.name
    print(f"  {c.name:22s} walk model vs float64 {r.split_vs_f64:.2e} (half the bar {BAR / 2:.0e})   float32 sums vs float64 sums {r.f32_vs_split:.2e}")
    assert r.split_vs_f64 <= BAR / 2, c.name
  print(f"  split share {share[0]:.2e} .. {share[1]:.2e} (row {share[2]})")
  print(f"  largest float32-vs-float64 summation difference {worst:.3e} (row {worst_row}): SPLIT_BAR = 4 x {SPLIT_MAX_F32:.2e} = {SPLIT_BAR:.2e}")
  # (upper side only: torch's float32 summation order on the CPU depends on its build and the machine; a smaller figure elsewhere
  # only means the constant, measured where the table was written, is the more careful of the two)
  assert worst <= 1.25 * SPLIT_MAX_F32, worst


# ------------------------------------------------------------------------------------------------ sensitivity
def _tile_keep(c, per, td):
  """[B, 1, D, H, W] 0 / 1 over the coarse grid: 0 on the last tile of every workgroup that walks more than one (slots of `per`
  consecutive tiles; a tile = td x 8 x 16 positions, W fastest)."""
  D, H, W = c.dims
  nD, nH, nW = D // td, H // 8, W // 16
  tiles = c.B * nD * nH * nW
  keep = t.ones(c.B, 1, D, H, W, dtype=t.float64)
  for beg in range(0, tiles, per):
    end = min(beg + per, tiles)
    if end - beg < 2: continue
    tl = end - 1
    wi, hi, di, bi = tl % nW, tl // nW % nH, tl // (nW * nH) % nD, tl // (nW * nH * nD)
    keep[bi, :, di * td:(di + 1) * td, hi * 8:(hi + 1) * 8, wi * 16:(wi + 1) * 16] = 0
  return keep


def _swapped(wd):
  """The windows with the taps zw = 1 and zw = 2 exchanged: a tap read one position off."""
  import copy
  m = copy.copy(wd)
  m.k = [{r: k[r][..., [0, 2, 1, 3]] for r in PARITIES} for k in wd.k]
  return m


def mutate(kind, b, r):
  """fwd / dgrad: the storage a kernel with bug `kind` would leave (float64); wgrad: what it would have added to the packed
  gradient [16][64][Npad].  None: the row cannot show that bug."""
  c = b.case
  if c.op == "wgrad":
    wg = lambda **kw: K.walk_wgrad(b, **kw)
    if kind == "tap_one_off": return r.model.view(16, 4, 4, 4, -1)[:, :, :, [0, 2, 1, 3]].reshape(16, 64, -1)
    if kind == "lo_hi_dropped": return wg(terms=K.TERMS[:2])
    if kind == "zw3_skip_on_rw1":
      m = r.model.clone()
      for i, (rd, rh, rw) in enumerate(PARITIES):
        if rw == 1: m.view(16, 4, 4, 4, -1)[:, :, :, 3, i * c.cout:(i + 1) * c.cout] = 0
      return m
    if kind == "clamped_duplicate_added":        # pair (0, 0): 36 taps dealt in 5 rounds of 8, four waves redo tap 35 = (2, 2, 3), rw 1
      m = r.model.clone()
      m[:, (2 * 4 + 2) * 4 + 3, c.cout:2 * c.cout] *= 5
      return m
    if kind == "shift_on_padding": return wg(pad_first=True) if c.tr in ("shift", "pre", "post", "both") else None
    if kind == "accumulate_ignored": return (r.model - r.base.view(16, 64, -1)) if c.accumulate else (r.model + K.SENTINEL)
    if kind == "last_tile_skipped":
      per = c.expect["tiles_per_wg"]
      if max(per) < 2: return None
      keeps = [_tile_keep(c, p, 2).float() for p in per]
      return wg(q_keep=lambda pair: keeps[pair])
    return None
  wd = K.windows_of(b, r.img)
  walk = K.walk_fwd if c.op == "fwd" else K.walk_dgrad
  bias = 0.0 if b.bias is None else b.bias.double().view(1, -1, 1, 1, 1)
  if kind == "tap_one_off": return r.storage(b, walk(b, _swapped(wd)) + bias)
  if kind == "lo_hi_dropped": return r.storage(b, walk(b, wd, terms=K.TERMS[:2]) + bias)
  if kind == "shift_on_padding":
    if c.op != "fwd" or c.tr not in ("shift", "pre", "post", "both"): return None
    return r.storage(b, K.walk_fwd(b, wd, pad_first=True) + bias)
  if kind == "accumulate_ignored": return r.storage(b, r.model, accumulate=False) if c.accumulate else None
  if kind == "bias_missing_on_one_parity":
    if b.bias is None: return None
    m = r.model.clone()
    m[:, :, 1::2, 1::2, 1::2] -= bias
    return r.storage(b, m)
  if kind == "last_tile_skipped":
    if not c.resident or c.expect["per"] < 2: return None
    keep = _tile_keep(c, c.expect["per"], 4)
    if c.op == "fwd": keep = keep.repeat_interleave(2, 2).repeat_interleave(2, 3).repeat_interleave(2, 4)
    lay, base = (b.yl, b.y0) if c.op == "fwd" else (b.xl, b.x0)
    st = r.storage(b, r.model)
    K.write_logical(lay.view(st), t.where(keep.bool(), K.logical(lay.view(st)), K.logical(lay.view(base.double()))))
    return st
  return None


MUTATIONS = {"tap_one_off": 20, "lo_hi_dropped": 20, "zw3_skip_on_rw1": 6, "clamped_duplicate_added": 6, "shift_on_padding": 8,
             "accumulate_ignored": 8, "bias_missing_on_one_parity": 6, "last_tile_skipped": 6}       # bug -> rows it must at least show on


@pytest.mark.parametrize("kind", list(MUTATIONS))
def test_bars_catch_a_kernel_bug(kind):
  """Every row to which the bug applies sees it at 10 times the bar or more."""
  hit, least = 0, None
  for c in NUMERIC:
    b, r = built(c.name), ref_of(c.name)
    m = mutate(kind, b, r)
    if m is None: continue
    hit += 1
    if c.op == "wgrad": err = float((K.unpack(b, m) - r.grad).abs().max()) / r.range
    else: err = err_inside(m, r.want, r.mask, r.range)
    least = err if least is None else min(least, err)
    assert err >= 10 * BAR, f"{c.name}: {kind} moves the result by {err:.2e} of the range only"
  print(f"\n  {kind}: {hit} rows, the least visible at {least / BAR:.0f} bars")
  assert hit >= MUTATIONS[kind], (kind, hit)


# ------------------------------------------------------------------------------------------------ reach
def test_table_reaches_every_kernel_and_every_switch():
  sel = lambda op, resident=False: [c for c in CASES if c.op == op and c.resident == resident]
  six = {"none", "scale", "shift", "pre", "post", "both"}
  borders = {(4, 8, 16), (8, 16, 32), (12, 8, 16), (4, 24, 16), (4, 8, 48)}
  f = sel("fwd")
  assert {c.cout for c in f} >= {1, 8, 9, 14, 16} and {c.dims for c in f} >= borders and {c.tr for c in f} == six
  assert any(K.tiles_of(c) % 8 for c in f) and {c.bias for c in f} == {True, False} and {c.B for c in f} >= {1, 3}
  assert any(c.c0 for c in f) and any(c.c_slack for c in f) and any(c.x_slack for c in f)
  assert any(c.tr in ("shift", "both", "pre", "post") and c.dims == (4, 8, 16) for c in f)           # a shift where every halo is padding
  d = sel("dgrad")
  assert {c.cout for c in d} >= {1, 8, 9, 16} and {c.dims for c in d} >= borders and {c.accumulate for c in d} == {True, False}
  assert any(c.c_slack == 0 for c in d) and any(c.c_slack > 0 for c in d) and any(c.x_slack for c in d)
  rf, rd = sel("fwd", True), sel("dgrad", True)
  assert {c.tr for c in rf} == six and all(c.cout == 2 for c in rf)
  assert {(c.cout, c.accumulate) for c in rd} == {(1, False), (1, True), (2, False), (2, True)}
  for rows in (rf, rd):
    assert any(c.expect["tiles"] < 256 for c in rows)
    assert any(c.expect["per"] > 1 and c.expect["tiles"] % c.expect["per"] and c.expect["wgs"] % 8 for c in rows)
  g = sel("wgrad")
  plain = [c for c in g if not c.deterministic]
  assert sorted(c.name[:-6] for c in plain if c.ximg == "ahead") == sorted(c.name[:-6] for c in plain if c.ximg == "fused")
  assert len(plain) >= 12 and {c.tr for c in plain} == six
  assert any(c.expect["ntiles"] == 1 for c in g)
  assert any(56 <= c.expect["ntiles"] <= 60 and len(set(c.expect["tiles_per_wg"])) > 1 and c.expect["ntiles"] % c.expect["tiles_per_wg"][0]
             for c in g)
  assert {c.cout for c in g} >= {1, 9, 16} and any(c.Npad == 8 * c.cout for c in g) and any(c.Npad > 8 * c.cout for c in g)
  assert {c.accumulate for c in plain} == {True, False} and any(c.dims[0] % 4 == 2 for c in g) and any(c.x_slack for c in g)
  assert sum(c.deterministic for c in g) == 1
  xi = sel("ximage")
  assert {c.tr for c in xi} == six and any(c.x_slack for c in xi) and any(c.dims == (3, 5, 12) for c in xi)
  assert any((c.dims[0] * c.dims[1] * c.dims[2] // 4) % 256 and c.dims[0] * c.dims[1] * c.dims[2] // 4 > 256 for c in xi)
  for c in CASES:                                     # no tensor above about 2.5 M elements
    D, H, W = c.dims
    assert max(c.B * 16 * D * H * W + c.B * c.x_slack, c.B * (c.c0 + c.cout + c.c_extra) * (8 * D * H * W + c.c_slack)) <= 2.6e6, c.name


def test_inputs_are_poisoned_and_outputs_start_at_the_sentinel():
  for c in CASES:
    b = built(c.name)
    if c.op in ("dgrad", "wgrad"):
      assert bool(b.dys[~b.yl.mask()].isnan().all()) and not bool(K.dy_logical(b, t.float32).isnan().any())
      assert int((~b.yl.mask()).sum()) >= 8 + (c.c0 + c.c_extra) * c.B
    if c.op != "dgrad":
      assert bool(b.xs[~b.xl.mask()].isnan().all()) and int((~b.xl.mask()).sum()) == 8 + c.B * c.x_slack
    out = {"fwd": getattr(b, "y0", None), "dgrad": getattr(b, "x0", None), "wgrad": getattr(b, "dw0", None)}.get(c.op)
    if out is not None and not c.accumulate:
      assert bool((out == K.SENTINEL).all())
