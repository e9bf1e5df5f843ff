"""What the encoder conv-engine case table (tests/conv_e2d_cases.py) reaches, asked of the plan queries on the CPU
(crn_conv2d_bf3_plan / crn_conv_wgrad_2d_bf3_plan: the selection code the launches themselves run), what the entries reject, and
whether the table's references can carry the bars of tests/test_conv_e2d_gpu.py: the share of the 2e-5 bar that the operand split
itself takes, the float32-versus-float64 summation difference that sets the sharper bar, and sensitivity to nine kernel bugs (and why a tenth,
unzeroed operand rows past C, can change no stored element)."""
import copy
import ctypes as C
import dataclasses
import functools
import os

import pytest
import torch as t
import torch.nn.functional as F

import conv_e2d_cases as K
import conv_fp32_cases as K32
from conv_e2d_cases import CASES, BAR, SPLIT_BAR, SPLIT_MAX_F32
from kernel_contract_emu import logical, write_logical
from corenet_amd.model import conv_geometry as G

_DET_ENV = os.environ.get("CRN_DETERMINISTIC", "0") == "1"
IDS = [c.name for c in CASES]
FWD_KERNELS, WG_KERNELS = ("k1", "k3w16", "k3w8"), ("wg1", "wg3")
LDS_MAX = 160 * 1024


@functools.lru_cache(maxsize=None)
def be():
  from corenet_amd.backend import HipBackend
  return HipBackend()          # loads the library; no GPU is touched by the plan queries


@functools.lru_cache(maxsize=None)
def built(name):
  return K.build(K.BY_NAME[name])


@functools.lru_cache(maxsize=None)
def ref_of(name):
  return K.make_ref(built(name))


@functools.lru_cache(maxsize=None)
def plan_of(name):
  b = built(name)
  c = b.case
  be().lib.crn_set_deterministic(int(c.deterministic or _DET_ENV))
  try:
    return K.query_plan(be(), b, b.xs, b.y0 if c.op == "fwd" else b.dys, b.wop, None if c.op == "fwd" else b.dw0)
  finally:
    be().lib.crn_set_deterministic(int(_DET_ENV))


def _want(c):
  return {k: v for k, v in c.expect.items() if not (_DET_ENV and c.op == "wgrad" and k in K.DET_FIELDS)}


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("name", IDS)
def test_every_case_gets_the_variant_its_row_names(name):
  c = K.BY_NAME[name]
  b, p = built(name), plan_of(name)
  want = _want(c)
  got = {k: p[k] for k in want}
  assert got == want, f"{name}: the plan query says {got}, the row is there for {want}"
  D, H, W = c.odims
  S = D * H * W
  if c.op == "fwd":
    assert p["kernel"] in FWD_KERNELS
    assert p["kernel"] == ("k1" if c.k == (1, 1, 1) else "k3w16" if W % 16 == 0 else "k3w8")
    assert p["nblk"] == b.ycin // 32 and p["nchunks"] == (-(-p["nblk"] // 4) if p["kernel"] == "k1" else p["nblk"])
    assert p["tiles"] == S // 64
    assert 1 <= p["splits"] <= 16 and p["splits"] == -(-p["nchunks"] // p["per_split"]), p
    assert p["mode"] == (3 if p["splits"] > 1 else int(c.accumulate)), p
    assert p["tab"] == (0 if not c.tr else p["per_split"] * (128 if p["kernel"] == "k1" else 32)), p
    assert p["lds_bytes"] == p["tab"] * 8 + (69632 if p["kernel"] == "k1" else 33792) and p["lds_bytes"] <= LDS_MAX, p
    assert (p["grid_x"], p["grid_y"], p["grid_z"]) == (p["tiles"] * c.B, b.ycout // 64, p["splits"]), p
    assert max(b.xs.numel(), b.y0.numel(), b.wp.numel()) <= 2_200_000, name
  else:
    assert p["kernel"] == ("wg1" if c.k == (1, 1, 1) else "wg3")
    assert p["row_tiles"] == (-(-c.cin // 64) if p["kernel"] == "wg1" else -(-3 * c.cin // 32)) and p["col_tiles"] == -(-c.cout // 32)
    assert p["ksteps"] == c.B * S // 32 and p["splits"] == -(-p["ksteps"] // p["per_block"]), p
    assert (p["grid_x"], p["grid_y"], p["grid_z"]) == (p["row_tiles"], p["col_tiles"], p["splits"]), p
    assert p["zero_bytes"] == (0 if c.accumulate else b.dw0.numel() * 4), p
    assert b.npad == -(-c.cout // 16) * 16


def _fwd_rows(kernel=None):
  return [(c, plan_of(c.name)) for c in CASES if c.op == "fwd" and (kernel is None or plan_of(c.name)["kernel"] == kernel)]


def _wg_rows(kernel=None):
  return [(c, plan_of(c.name)) for c in CASES if c.op == "wgrad" and (kernel is None or plan_of(c.name)["kernel"] == kernel)]


def test_table_reaches_every_kernel_and_every_switch():
  assert {p["kernel"] for _, p in _fwd_rows()} == set(FWD_KERNELS) and {p["kernel"] for _, p in _wg_rows()} == set(WG_KERNELS)
  for kern in FWD_KERNELS:
    rows = _fwd_rows(kern)
    # store, accumulate, partial sums: each with and without a transform
    assert {(p["mode"], bool(c.tr)) for c, p in rows} == {(m, tr) for m in (0, 1, 3) for tr in (False, True)}, kern
    assert any(p["splits"] > 1 and p["nchunks"] % p["per_split"] for _, p in rows), kern                 # a short last split
    assert any(p["splits"] == 16 for _, p in rows) or kern != "k3w16"                                    # the cap, reached exactly
    assert any(p["nchunks"] > 16 and p["per_split"] == 2 for _, p in rows), kern                          # ... and exceeded
    assert {p["mode"] for _, p in rows if p["splits"] == 1 and p["nchunks"] >= 3} == {0, 1}, kern          # both LDS buffers in one split
    assert {c.tr for c, _ in rows} >= {"", "shift", "pre", "post", "both"}, kern
    assert {(c.bias, c.bias_b) for c, _ in rows} >= {(False, False), (True, False), (True, True)}, kern
    assert any(c.bias_b and c.B > 1 for c, _ in rows), kern
    assert any(c.accumulate and p["splits"] > 1 for c, p in rows) and any(c.accumulate and p["splits"] == 1 for c, p in rows), kern
    assert {c.xview for c, _ in rows} >= {"plain", "slice", "nc"} and {c.yview for c, _ in rows} >= {"plain", "slice", "nc"}, kern
    assert any(c.geom == "dgrad" for c, _ in rows), kern
    assert {c.cout for c, _ in rows} >= {64, 128}, kern
    assert any(c.B > 1 and p["splits"] > 1 for c, p in rows), kern
    if kern == "k1":
      assert any(p["nblk"] % 4 and p["splits"] > 1 and c.tr for c, p in rows)                              # the clamp of the table fill
      assert any(p["nblk"] % 4 and p["splits"] == 1 and p["nchunks"] >= 3 for c, p in rows)
      assert any(p["nblk"] == 1 for _, p in rows) and any(c.odims[0] > 1 for c, _ in rows)
    else:
      assert {c.pad for c, _ in rows} >= {(0, 1, 1), (0, 0, 0), (0, 2, 2), (0, 0, 2), (0, 1, 0)}, kern
      tw = 16 if kern == "k3w16" else 8
      assert any(c.odims[1] >= 3 * (64 // tw) and c.odims[2] >= 3 * tw for c, _ in rows), kern              # a tile that touches no border
      assert any(c.odims[1] == 64 // tw and c.odims[2] == tw for c, _ in rows), kern                        # a tile that touches all four
  assert any(c.odims == (1, 8, 40) for c, _ in _fwd_rows("k3w8"))
  if _DET_ENV: return
  for kern in WG_KERNELS:
    rows = _wg_rows(kern)
    per_row = 64 if kern == "wg1" else 32
    rows_of = lambda c: c.cin if kern == "wg1" else 3 * c.cin
    assert any(rows_of(c) % per_row for c, _ in rows) and any(rows_of(c) % per_row == 0 for c, _ in rows), kern
    assert any(c.cout % 32 and c.cout > 32 for c, _ in rows) and any(c.cout < 16 for c, _ in rows) and any(c.cout % 32 == 0 for c, _ in rows), kern
    assert any(c.cout % 16 and c.accumulate for c, _ in rows) and any(c.cout % 16 and not c.accumulate for c, _ in rows), kern
    assert any(p["splits"] > 1 and p["ksteps"] % p["per_block"] for _, p in rows), kern                   # uneven blocks
    assert any(p["splits"] == 3 for _, p in rows), kern
    assert {p["ksteps"] for _, p in rows} >= {1, 5, 9, 19, 24}, kern
    assert any(p["ksteps"] % 4 for _, p in rows), kern
    assert any(c.B > 1 and (c.odims[0] * c.odims[1] * c.odims[2] // 32) % 4 for c, _ in rows), kern        # a wave's next step is in another sample
    assert sum(c.deterministic and p["splits"] == 1 and p["ksteps"] >= 16 for c, p in rows) >= 2, kern
    assert {c.tr for c, _ in rows} >= {"", "post", "both"}, kern
    assert any(c.tr == "both" and rows_of(c) % per_row for c, _ in rows), kern                             # T(0) != 0 in rows past C
    assert any(c.xview == "slice" and c.yview == "slice" for c, _ in rows), kern
  assert any(c.odims[0] > 1 for c, _ in _wg_rows("wg1"))
  assert {c.odims for c, _ in _wg_rows("wg3")} >= {(1, 4, 8), (1, 8, 8), (1, 4, 16), (1, 4, 24), (1, 8, 32)}
  assert {c.cin for c, _ in _wg_rows("wg3")} >= {5, 11, 32}
  assert {(c.cout, built(c.name).npad) for c, _ in _wg_rows("wg3")} >= {(12, 16), (40, 48), (64, 64)}
  assert {(c.cin, c.cout, built(c.name).npad) for c, _ in _wg_rows("wg1")} >= {(67, 12, 16), (35, 40, 48), (64, 64, 64)}


# ------------------------------------------------------------------------------------------------ the model's own shapes
def _model_layers():
  """(name, (Cout, Cin, kh, kw), (H, W)) of the encoder's stride-1 convolutions behind the stem and of the decoder's rt_skip 1x1
  layers, from the model's own parameter list at a 256 x 256 image: stage n works on 256 / 2^n positions per side; rt_skip_n reads the
  encoder map with its Cin - 3 channels."""
  from corenet_amd.model.engine import param_specs
  out = []
  side = {256: 64, 512: 32, 1024: 16, 2048: 8}
  for key, shape, _ in param_specs(2):
    parts = key.split(".")
    if parts[-1] != "weight" or len(shape) != 4: continue
    if parts[0] == "encoder" and parts[1].startswith("stage") and parts[1] != "stage1":
      n = 256 >> int(parts[1][5:])
      out.append((key[:-7], tuple(shape), (n, n)))
    if parts[0] == "decoder" and parts[1].startswith("rt_skip"):
      n = side[shape[1] - 3]
      out.append((key[:-7], tuple(shape), (n, n)))
  return out


def _model_plans(B=4):
  from corenet_amd import _lib
  out = {}
  for name, (co, ci, kh, kw), (H, W) in _model_layers():
    k, pad, dims = (1, kh, kw), (0, kh // 2, kw // 2), (1, H, W)
    xs, ys = t.empty(K.view_numel("plain", B, ci, dims)), t.empty(K.view_numel("plain", B, co, dims))
    xv, yv = K.make_view("plain", xs, B, ci, dims), K.make_view("plain", ys, B, co, dims)
    npad = G.pad16(co)
    if name.startswith("encoder"):
      out[name, "fwd"] = be().conv2d_bf3_plan(xv, None, xs, npad, None, 0, yv, k, pad)
      out[name, "dgrad"] = be().conv2d_bf3_plan(yv, None, xs, ci, None, 0, xv, k, pad)
    else:
      with pytest.raises(_lib.HipError):             # 2051 channels: the forward pass of these layers stays on the fp32 engine
        be().conv2d_bf3_plan(xv, None, xs, npad, None, 0, yv, k, pad)
    out[name, "wgrad"] = be().conv_wgrad_2d_bf3_plan(xv, None, yv, xs, npad, k, pad, False)
  return out


def test_model_shapes_are_covered():
  model = _model_plans()
  names = {n for n, _ in model}
  assert len([n for n in names if n.startswith("encoder")]) == 52 and len([n for n in names if n.startswith("decoder")]) == 4
  print()
  for (n, ps), p in model.items():
    if ps == "wgrad":
      print(f"  {n:44s} {ps:5s} {p['kernel']:5s} tiles {p['row_tiles']}x{p['col_tiles']} ksteps {p['ksteps']} per block {p['per_block']} splits {p['splits']}")
    else:
      print(f"  {n:44s} {ps:5s} {p['kernel']:5s} tiles {p['tiles']} chunks {p['nchunks']} per split {p['per_split']} splits {p['splits']} mode {p['mode']} lds {p['lds_bytes']}")
  table = {(p["kernel"], p["mode"], p["splits"] > 1) for _, p in _fwd_rows()}
  used = {(p["kernel"], p["mode"], p["splits"] > 1) for (n, ps), p in model.items() if ps != "wgrad"}
  # the engine accumulates some data gradients (the residual sum): the same launches with mode 1 where they do not split
  used |= {(k, 1, False) for k, m, s in used if not s}
  assert used <= table, used - table
  if _DET_ENV: return
  tw = {(p["kernel"], p["splits"] > 1) for _, p in _wg_rows()}
  uw = {(p["kernel"], p["splits"] > 1) for (n, ps), p in model.items() if ps == "wgrad"}
  assert uw <= tw, uw - tw
  # the rt_skip layers: 2051 channels = a 33rd row tile of 3 channels, 12 .. 96 columns
  sk = {n: p for (n, ps), p in model.items() if ps == "wgrad" and n.startswith("decoder")}
  assert {(p["row_tiles"], p["col_tiles"]) for p in sk.values()} == {(33, 3), (17, 2), (9, 1), (5, 1)}


def test_what_no_call_reaches():
  """What no row runs, with the arithmetic."""
  # 1. The LDS bound of the forward kernels: the tables take 8 bytes per channel of one split next to four patch planes; the bound
  # is passed at 16288 channels (3x3) / 11808 (1x1) in ONE split, which takes 256 workgroups without a split: x alone is 10^9 bytes or
  # more.  Rows of rejections() ask the query on both sides of it; no launch reaches it.
  assert (LDS_MAX - 33792) // 8 == 16256 and (LDS_MAX - 69632) // 8 == 11776
  assert 4 * 16288 * 64 * 64 * 4 >= 10 ** 9
  # 2. The same for a sample or the operand blocks of 2 GiB.
  # 3. `cbeg < cend` of conv_e2d_kernel is true in every workgroup: splits = ceil(nchunks / per_split), so the last split starts at
  # (splits - 1) * per_split < nchunks -- asked of the query over every chunk count and fill a launch can have.
  ys = t.empty(64)
  for nblk in range(1, 80):
    for k, dims in (((1, 3, 3), (1, 4, 16)), ((1, 1, 1), (1, 8, 8)), ((1, 3, 3), (1, 32, 32))):
      for B in (1, 4, 16):
        xv, yv = K.make_view("plain", ys, B, 32 * nblk, dims), K.make_view("plain", ys, B, 64, dims)     # (never touched)
        p = be().conv2d_bf3_plan(xv, None, ys, 64, None, 0, yv, k, (0, k[1] // 2, k[2] // 2))
        assert (p["splits"] - 1) * p["per_split"] < p["nchunks"] <= p["splits"] * p["per_split"] and p["splits"] <= 16, p
  # 4. Weight gradient: `kbeg < kend` likewise (splits = ceil(ksteps / per_block)); a wave whose first step is past kend (ksteps 1:
  # three of them, row g1_c67_n12_k1) loads zeros and multiplies nothing.
  # 5. Rows past C under a transform.  The kernels zero the operand rows of channels past C (`T(0) is not 0`), but a row of the MFMA
  # result depends on the same row of the A operand only, and rows past C are not stored (`c < g.C` / `q < 3 * g.C` in front of the
  # atomics): whatever those operand rows hold, no element of dw can tell.  test_sensitivity_wgrad shows it on the model.


# ------------------------------------------------------------------------------------------------ rejections
def _ask(op, a, out):
  L = be().lib
  if op == "fwd": return L._crn_conv2d_bf3_plan(*a["args"], C.byref(out))
  return L._crn_conv_wgrad_2d_bf3_plan(*a["args"], C.byref(out))


def test_plan_queries_reject_what_the_launches_reject():
  from corenet_amd import _lib
  out = _lib.CrnE2dPlan()
  rej, acc = K.rejections(), K.rejections(accepted=True)
  assert len(rej) >= 60
  for name, op, mk, _ in rej:
    assert _ask(op, mk("cpu"), out) == -1, name
  for name, op, mk, _ in acc:
    assert _ask(op, mk("cpu"), out) == 0, name
  assert {n for n, _, _, launch in rej if not launch} >= {"fwd: a sample of 2 GiB", "wgrad: a sample of x of 2 GiB"}
  assert sum("LDS bound" in n for n, _, _, launch in rej if not launch) == 2
  a = acc[0][2]("cpu")
  assert be().lib._crn_conv2d_bf3_plan(*a["args"], None) == -1


# ------------------------------------------------------------------------------------------------ the references
def test_reference_share_of_the_bars():
  """On every row the split model (exact products of the split operands, summed in float64) is within half of the 2e-5 bar of the
  float64 reference: the other half belongs to the kernel's float32 accumulation.  And the constant behind the sharper bar is what
  this table measures: the largest float32-versus-float64 summation difference of the split model over all rows."""
  worst, wname = 0.0, ""
  print()
  for c in CASES:
    r = ref_of(c.name)
    if r.f32_vs_split > worst: worst, wname = r.f32_vs_split, c.name
    print(f"  {c.name:18s} split model vs float64 {r.split_vs_f64:.2e} (half the bar {BAR / 2:.0e})   float32 sums vs float64 sums {r.f32_vs_split:.2e}")
    assert r.split_vs_f64 <= BAR / 2, c.name
  print(f"  largest float32-vs-float64 summation difference {worst:.3e} ({wname}): SPLIT_BAR = 4 x {SPLIT_MAX_F32:.2e} = {SPLIT_BAR:.2e}")
  # (upper side only: torch's float32 summation order on the CPU depends on its build and the machine)
  assert worst <= 1.25 * SPLIT_MAX_F32, worst


# ------------------------------------------------------------------------------------------------ sensitivity
def _chan_of_split(p, kernel):
  return p["per_split"] * (128 if kernel == "k1" else 32)


def _with(b, **kw):
  b2 = copy.copy(b)
  for k, v in kw.items(): setattr(b2, k, v)
  return b2


def fault_fwd(kind, b, p, r):
  """The storage a forward kernel with fault `kind` would leave (float64), or None when the row cannot show it."""
  c = b.case
  k1 = p["kernel"] == "k1"
  per = _chan_of_split(p, p["kernel"])
  if kind == "lo_hi_dropped":
    return K.expected_y(b, K.split_fwd(b, terms=(("h", "h"), ("h", "l"))))
  if kind == "bias_on_every_split":
    if b.bp is None or p["splits"] <= 1: return None
    return K.expected_y(b, r.conv, bias_times=p["splits"])
  if kind == "last_short_split_dropped":
    if p["splits"] <= 1 or p["nchunks"] % p["per_split"] == 0: return None
    keep = (t.arange(b.ycin) < (p["splits"] - 1) * per).double()
    return K.expected_y(b, K32.corr_logical(b, chan_keep=keep))
  if kind == "last_partial_chunk_dropped":
    if not k1 or p["nblk"] % 4 == 0: return None
    keep = (t.arange(b.ycin) < (p["nchunks"] - 1) * 128).double()
    return K.expected_y(b, K32.corr_logical(b, chan_keep=keep))
  if kind == "table_without_split_origin":
    if not c.tr or p["splits"] <= 1: return None
    idx = t.arange(b.ycin) % per                                    # every split reads the table of split 0
    return K.expected_y(b, K32.corr_logical(_with(b, scale=b.scale[idx], shift=b.shift[idx])))
  if kind == "padding_transformed":
    if k1 or not c.tr: return None
    return K.expected_y(b, K32.corr_logical(b, pad_first=True))
  if kind == "tile_row_offset_of_other_width":
    if k1: return None
    # the patch of tile row thi is staged from image row thi * TH' with TH' the height of the OTHER tile form; the epilogue is right
    D, H, W = c.odims
    TH = 4 if p["kernel"] == "k3w16" else 8
    THo = 12 - TH
    if H <= TH: return None
    x = K32.logical_x(b)
    xt = K32._transformed(b, x)
    xt = F.pad(xt, (0, 0, 0, 2 * H))                                # rows past the image read as zeros (out-of-range loads)
    b2 = _with(b, case=dataclasses.replace(c, odims=(1, 3 * H, W)))
    full = F.conv3d(F.pad(xt, K32._pads(b2, xt, b.pad_lo)), b.wp.double().view(b.ycin, *b.window, b.npad).permute(4, 0, 1, 2, 3))[:, :b.ycout]
    rows = t.cat([t.arange(TH) + thi * THo for thi in range(H // TH)])
    return K.expected_y(b, full[:, :, :, rows])
  raise ValueError(kind)


FWD_FAULTS = {          # fault -> the row that must see it at 10 bars or more
    "lo_hi_dropped": "a_3ch_m0", "bias_on_every_split": "a_c96_b2", "last_short_split_dropped": "b_24_c96",
    "last_partial_chunk_dropped": "c_c288_m0", "table_without_split_origin": "c_c160_s192", "padding_transformed": "a_pad22",
    "tile_row_offset_of_other_width": "b_24_c96"}


@pytest.mark.parametrize("kind", list(FWD_FAULTS))
def test_sensitivity_fwd(kind):
  hit, seen = 0, {}
  for c in CASES:
    if c.op != "fwd": continue
    b, p, r = built(c.name), plan_of(c.name), ref_of(c.name)
    st = fault_fwd(kind, b, p, r)
    if st is None: continue
    hit += 1
    seen[c.name] = K32.err_inside(st, r.want, r.mask, r.range)
  print(f"\n  {kind}: {hit} rows; " + ", ".join(f"{n} {e / BAR:.0f}" for n, e in seen.items()) + " bars")
  named = FWD_FAULTS[kind]
  assert seen[named] >= 10 * BAR, f"{named}: {kind} moves the result by {seen[named]:.2e} of the range only"
  for kern in FWD_KERNELS:            # ... and on every kernel the fault can happen in
    mine = [e for n, e in seen.items() if plan_of(n)["kernel"] == kern]
    assert not mine or max(mine) >= 10 * BAR, (kind, kern)
  assert {plan_of(n)["kernel"] for n in seen} >= ({"k1"} if kind == "last_partial_chunk_dropped" else
                                                  {"k3w16", "k3w8"} if kind in ("padding_transformed", "tile_row_offset_of_other_width")
                                                  else set(FWD_KERNELS)), kind


def _wgrad_packed_from(b, xp, dy):
  """The packed weight gradient [cin][T][npad] (float64) of a padded, transformed input xp and dy."""
  gw = F.conv3d(xp.transpose(0, 1).contiguous(), dy.transpose(0, 1).contiguous())           # [cin, cout, 1, kh, kw]
  out = t.zeros(b.ycin, b.window[0] * b.window[1] * b.window[2], b.npad, dtype=t.float64)
  out[:, :, :b.ycout] = gw.permute(0, 2, 3, 4, 1).reshape(b.ycin, -1, b.ycout)
  return out.reshape(-1)


def fault_wgrad(kind, b, p, r):
  c = b.case
  D, H, W = c.odims
  S = D * H * W
  base = b.dw0.double() if c.accumulate else 0.0
  if kind == "lo_hi_dropped":
    xh, xl = K.KB._split(K.KB._x_operand(b)); dh, dl = K.KB._split(logical(K.yview(b, b.dys)))
    g = _wgrad_packed_from(b, xh.double(), dh.double()) + _wgrad_packed_from(b, xh.double(), dl.double())
    return g + base
  if kind == "rows_past_C_not_zeroed":
    # operand rows c >= C hold T(0) = shift instead of 0: they reach rows c >= C of the result only, which are not stored
    if not c.tr: return None
    return r.grad + base
  if kind == "edge_across_row_end":
    if p["kernel"] != "wg3": return None
    xt = K32._transformed(b, K32.logical_x(b))
    xp = F.pad(xt, K32._pads(b, xt, b.pad_lo))                      # [B, C, 1, H + 2, W + 2]
    flat = F.pad(xt.reshape(c.B, b.ycin, H * W), (1, 1))            # the channel plane with one element before and behind it
    prev = flat[:, :, 0:H * W:W].reshape(c.B, b.ycin, 1, H)         # element s - 1 of the first position of every row
    nxt = flat[:, :, W + 1:H * W + 2:W].reshape(c.B, b.ycin, 1, H)  # element s + 1 of the last
    xp = xp.clone()
    xp[:, :, :, 1:H + 1, 0] = prev
    xp[:, :, :, 1:H + 1, W + 1] = nxt
    return _wgrad_packed_from(b, xp, logical(K.yview(b, b.dys.double()))) + base
  if kind == "last_step_of_a_block_skipped":
    steps = t.arange(c.B * S) // 32
    last = [min((z + 1) * p["per_block"], p["ksteps"]) - 1 for z in range(p["splits"])]
    keep = (~t.isin(steps, t.tensor(last))).view(c.B, 1, D, H, W)
    return K32.ref_wgrad_packed(b, dy_keep=keep) + base
  raise ValueError(kind)


WG_FAULTS = {"lo_hi_dropped": "g1_k24", "edge_across_row_end": "g3_4x8_c5_k1", "last_step_of_a_block_skipped": "g1_k19"}


@pytest.mark.parametrize("kind", list(WG_FAULTS) + ["rows_past_C_not_zeroed"])
def test_sensitivity_wgrad(kind):
  seen = {}
  for c in CASES:
    if c.op != "wgrad": continue
    b, p, r = built(c.name), plan_of(c.name), ref_of(c.name)
    g = fault_wgrad(kind, b, p, r)
    if g is None: continue
    seen[c.name] = K32.err_inside(g, r.want, r.real, r.range)
  print(f"\n  {kind}: {len(seen)} rows; " + ", ".join(f"{n} {e / BAR:.0f}" for n, e in seen.items()) + " bars")
  if kind == "rows_past_C_not_zeroed":
    # no stored element depends on those operand rows (test_what_no_call_reaches, 5.): the one listed fault that no row can see,
    # whatever its shape.  What a row CAN see of it -- a write to the rows behind C * taps -- is a write outside dw: the GPU module
    # keeps a sentinel there.
    assert seen and max(seen.values()) == 0.0
    return
  named = WG_FAULTS[kind]
  assert seen[named] >= 10 * BAR, f"{named}: {kind} moves the gradient by {seen[named]:.2e} of the range only"
  for kern in WG_KERNELS:
    mine = [e for n, e in seen.items() if plan_of(n)["kernel"] == kern]
    assert not mine or max(mine) >= 10 * BAR, (kind, kern)
  # an ignored accumulate
  if kind == "lo_hi_dropped":
    acc = [c for c in CASES if c.op == "wgrad" and c.accumulate]
    assert len(acc) >= 6
    for c in acc:
      r = ref_of(c.name)
      assert K32.err_inside(r.grad, r.want, r.real, r.range) >= 10 * BAR, c.name


def test_operand_table_of_the_gpu_module():
  """The five-layer table of crn_bf3_operands that tests/test_conv_e2d_gpu.py launches: what it is there for."""
  packed, desc, blocks, nbytes = K.operand_layers()
  assert desc.shape == (5, 7) and len({int(d) for d in desc[:, 6]}) == 2                       # both orders in one table
  first = [int(d) for d in desc[:, 5]]
  assert first == sorted(first) and blocks > first[-1]
  assert [int(d) for d in desc[:, 1]] != sorted(int(d) for d in desc[:, 1])                    # out of order in the output
  out = t.full((nbytes + K.OPERAND_SLACK,), K.OPERAND_SENTINEL, dtype=t.uint8)
  K._EMU.bf3_operands(packed, (t.as_tensor(desc), blocks), out)
  assert bool((out[nbytes:] == K.OPERAND_SENTINEL).all())
  assert int((out[:nbytes] == K.OPERAND_SENTINEL).sum()) < nbytes // 64                        # every entry written
