"""What the split-bf16 conv-engine case table (tests/conv_bf3_cases.py) reaches, asked of the plan queries on the CPU
(crn_conv_fwd_bf3_plan / crn_conv_wgrad_bf3_plan: the selection code the launches themselves run), what the entries reject, and
whether the table's references can carry the bars of tests/test_conv_bf3_gpu.py: the share of the 2e-5 bar that the operand split
itself takes, the float32-versus-float64 summation difference that sets the sharper bar, and sensitivity to eight kernel bugs."""
import ctypes as C
import functools
import os

import pytest
import torch as t

import conv_bf3_cases as K
import conv_fp32_cases as K32
from conv_bf3_cases import CASES, BAR, SPLIT_BAR, SPLIT_MAX_F32
from kernel_contract_emu import logical, write_logical
from corenet_amd.model import conv_geometry as G

_DET_ENV = os.environ.get("CRN_DETERMINISTIC", "0") == "1"
IDS = [c.name for c in CASES]
FWD_KERNELS = ({("plain", n, x, g, s) for n in (1, 2, 4) for x, g in ((1, 7), (1, 4), (2, 4)) for s in (0, 1)} |
               {("half", 1, 1, g, s) for g in (7, 4) for s in (0, 1)} | {("ws", 2, 1, 7, 1)})
WG_KERNELS = {(n,) + v for n in (1, 2) for v in ((1, 8, 16), (2, 4, 16), (1, 4, 16), (1, 8, 8), (2, 4, 8))}


def _model_layers(num_classes=2):
  """The decoder's convolutions with k5 / k7 windows, from the model's own parameter list (engine.param_specs: stages 3-6, c1 =
  Conv3d k5 'same', t1 = ConvTranspose3d k7 stride 2 padding 3): (name, kind, weight shape, padding, input extent).  Stage st works
  on 2^st positions per side (stage_6.t1 writes the 128^3 grid)."""
  from corenet_amd.model.engine import param_specs
  out = []
  for key, shape, _ in param_specs(num_classes):
    parts = key.split(".")
    if parts[0] != "decoder" or not parts[1].startswith("stage_") or parts[-1] != "weight" or len(shape) != 5: continue
    st, layer, k = int(parts[1][6:]), parts[2], shape[2]
    if (layer, k) not in (("c1", 5), ("t1", 7)): continue
    out.append((f"s{st}{layer}", "conv" if layer == "c1" else "convT", tuple(shape), (k - 1) // 2, (2 ** st,) * 3))
  return out


MODEL_LAYERS = _model_layers()


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
    fuse = None
    if c.fuse:
      ws = t.zeros(K.WS_BYTES(b) // 8, dtype=t.float64)
      fuse = K.fuse_request(b, ws, t.zeros(600), getattr(b, "bn_x", None), getattr(b, "bn_saved", None))
    return K.query_plan(be(), b, b.xs, b.y0 if c.op == "fwd" else b.dys, b.wp, None if c.op == "fwd" else b.dw0,
                        slab=b.slab if c.slabs else None, fuse=fuse)
  finally:
    be().lib.crn_set_deterministic(int(_DET_ENV))


def _fkey(p): return (p["kind"], p["nsub"], p["xmode"], p["ng"], p["slabs"])
def _wkey(p): return (p["nsub"], p["dmode"], p["tpw"], p["twt"])


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("name", IDS)
def test_every_case_gets_the_variant_its_row_names(name):
  c = K.BY_NAME[name]
  p = plan_of(name)
  want = {k: v for k, v in c.expect.items() if not (_DET_ENV and k in ("splits", "per_split"))}
  got = {k: p[k] for k in want}
  assert got == want, f"{name}: the plan query says {got}, the row is there for {want}"
  # invariants of any plan
  assert p["lds_bytes"] <= 160 * 1024 - 512, p
  assert 1 <= p["splits"] <= max(1, p["chunks"]) and p["splits"] == -(-p["chunks"] // p["per_split"]), p
  assert (p["td"], p["th"], p["tw"]) in ((4, 8, 16), (8, 8, 8)), p
  if c.op == "fwd":
    assert _fkey(p) in FWD_KERNELS, p
    assert p["mode"] == (3 if p["splits"] > 1 else int(c.accumulate)), p
    assert p["chunks"] == -(-built(name).ycin // 8)
    if p["splits"] > 1: assert p["vec_store"] == 1 and p["nparts"] == 0, p      # the scratch is dense; a split launch fuses nothing
    # every row but the whole-tile ones has a partial tile in D or H
    assert c.odims[0] % p["td"] or c.odims[1] % p["th"], name
  else:
    assert _wkey(p) in WG_KERNELS, p
    assert c.odims[0] % p["td"] or c.odims[1] % p["th"], name
    assert p["pipe"] == int(p["nsub"] == 1 or (p["tpw"], p["twt"]) == (8, 16)), p


def _model_plans():
  """(layer, pass) -> plan for the decoder's own layer shapes: views over untouched (never filled) storage."""
  from corenet_amd import _lib
  out = {}
  B = 4
  for name, kind, wshape, pad, dims in MODEL_LAYERS:
    if kind == "conv":
      cin, cout = wshape[1], wshape[0]
      fwd, dgr, odims, ykind, ych = G.conv_fwd(wshape, pad), G.conv_dgrad(wshape, pad), dims, "plain", cout
    else:
      cin, cout = wshape[0], wshape[1]
      fwd, dgr, odims, ykind, ych = G.convt_fwd(wshape, pad), G.convt_dgrad(wshape, pad), dims, "s2d", 8 * cout
    xs = t.empty(K.view_numel("plain", B, cin, dims)); ys = t.empty(K.view_numel(ykind, B, ych, odims))
    xv, yv = K.make_view("plain", xs, B, cin, dims), K.make_view(ykind, ys, B, ych, odims)
    slab = t.empty(64, dtype=t.uint8)
    try:                                 # (batch 4: the benchmark's)
      out[name, "fwd"] = be().conv_fwd_bf3_plan(xv, None, None, fwd.npad, None, 0, yv, fwd.window, fwd.pad_lo, boxes=(fwd.n_boxes, fwd.c_boxes), wslab=slab)
      out[name, "dgrad"] = be().conv_fwd_bf3_plan(yv, None, None, dgr.npad, None, 0, xv, dgr.window, dgr.pad_lo, boxes=(dgr.n_boxes, dgr.c_boxes), wslab=slab)
      out[name, "wgrad"] = be().conv_wgrad_bf3_plan(xv, None, yv, xs, fwd.npad, fwd.window, fwd.pad_lo, True, boxes=(fwd.n_boxes, fwd.c_boxes))
    except _lib.HipError as e:           # a layer the engine rejects runs on the fp32 engine
      out[name, "rejected"] = str(e)
  return out


FWD_SWITCHES = ("vec_store", "rowskip", "half_last", "lead")
WG_SWITCHES = ("inherit", "boxskip", "lead")


def test_table_reaches_every_instantiated_kernel_and_every_switch():
  fp = [plan_of(c.name) for c in CASES if c.op == "fwd"]
  wp = [plan_of(c.name) for c in CASES if c.op == "wgrad"]
  fwd, wg = {_fkey(p) for p in fp}, {_wkey(p) for p in wp}
  model = _model_plans()
  assert len(MODEL_LAYERS) == 8 and not [k for k in model if k[1] == "rejected"], model.keys()
  mf = {_fkey(p) for (n, ps), p in model.items() if ps in ("fwd", "dgrad")}
  mw = {_wkey(p) for (n, ps), p in model.items() if ps == "wgrad"}
  print(f"\nforward kernels reached: table {len(fwd)}/{len(FWD_KERNELS)}, the decoder's layer shapes (slabs, batch 4) {len(mf)}/{len(FWD_KERNELS)}")
  for k in sorted(FWD_KERNELS): print(f"  {k}: table {'x' if k in fwd else '-'}  model {'x' if k in mf else '-'}")
  print(f"weight-gradient kernels reached: table {len(wg)}/{len(WG_KERNELS)}, the decoder's layer shapes {len(mw)}/{len(WG_KERNELS)}")
  for k in sorted(WG_KERNELS): print(f"  {k}: table {'x' if k in wg else '-'}  model {'x' if k in mw else '-'}")
  for sw in FWD_SWITCHES + ("mode",):
    print(f"  forward {sw}: table {sorted({p[sw] for p in fp})}  model {sorted({p[sw] for (n, ps), p in model.items() if ps in ('fwd', 'dgrad')})}")
  for sw in WG_SWITCHES:
    print(f"  weight gradient {sw}: table {sorted({p[sw] for p in wp})}  model {sorted({p[sw] for (n, ps), p in model.items() if ps == 'wgrad'})}")
  assert fwd == FWD_KERNELS, FWD_KERNELS - fwd
  assert wg == WG_KERNELS, WG_KERNELS - wg
  for sw in FWD_SWITCHES: assert {p[sw] for p in fp} == {0, 1}, sw
  assert {p["mode"] for p in fp} == {0, 1, 3}
  assert {p["n_groups"] for p in fp} == {0, 8} and {p["c_groups"] for p in fp} == {0, 8}
  for sw in WG_SWITCHES: assert {p[sw] for p in wp} == {0, 1}, sw
  assert {p["tw"] for p in fp} == {16, 8}
  # splits of the weight gradient: 1 without and with deterministic mode, between, and one per tile
  if not _DET_ENV:
    sp = {("one" if p["splits"] == 1 else "all" if p["splits"] == p["chunks"] else "between") for p in wp}
    assert sp == {"one", "between", "all"}
    assert plan_of("g_splits1")["splits"] == 1 and not K.BY_NAME["g_splits1"].deterministic
  assert plan_of("g_det")["splits"] == 1 and plan_of("g_det")["chunks"] == 8
  # the wave-specialised kernel with 1, 2 and 3 chunks per split
  assert {p["per_split"] for p in fp if p["kind"] == "ws"} >= {1, 2, 3}
  # dy->C < Npad, zero_first 0 and 1
  wc = [c for c in CASES if c.op == "wgrad"]
  assert any(c.cout % 16 and c.accumulate for c in wc) and any(c.cout % 16 and not c.accumulate for c in wc)


def test_table_carries_every_edge_once_per_staging_mode():
  rows = [(c, plan_of(c.name)) for c in CASES if c.op == "fwd"]
  for xm in (1, 2):
    mine = [(c, p) for c, p in rows if p["xmode"] == xm]
    assert any(built(c.name).ycin < 8 for c, _ in mine), xm                                   # one partial chunk
    assert any(1 <= built(c.name).ycin % 8 <= 4 and built(c.name).ycin > 8 for c, _ in mine), xm
    assert any(built(c.name).ycin % 8 >= 5 and built(c.name).ycin > 8 for c, _ in mine), xm
    assert any(p["half_last"] and p["kind"] == "plain" for _, p in mine), xm
    assert any(p["lead"] for _, p in mine), xm                                                # odd pw
    assert any(c.B > 1 for c, _ in mine) and any(p["splits"] > 1 for _, p in mine) and any(p["splits"] == 1 for _, p in mine), xm
    assert any(c.accumulate and p["splits"] > 1 for c, p in mine) and any(c.accumulate and p["splits"] == 1 for c, p in mine), xm
    assert any(c.bias and p["splits"] > 1 for c, p in mine), xm
    assert any(p["rowskip"] for _, p in mine) and any(p["ng"] == 4 and not p["rowskip"] for _, p in mine), xm
    # pads of 0 under a larger x, pads above the model's 3, x extents unlike y's (larger and smaller)
    assert any(c.pad == (0, 0, 0) and c.xdims and all(x > o for x, o in zip(c.xdims, c.odims)) for c, _ in mine), xm
    assert any(max(c.pad) > 3 for c, _ in mine), xm
    assert any(c.xdims and all(x < o for x, o in zip(c.xdims, c.odims)) for c, _ in mine), xm
    assert any(c.B > 1 and c.xview in ("sb2", "s2co", "s2d", "slice") for c, _ in mine), xm
  unit = [(c, p) for c, p in rows if p["xmode"] == 1]
  assert {c.tr for c, _ in unit} >= {"", "shift", "pre", "post", "both", "scale"}
  assert {c.tr for c, p in rows if p["xmode"] == 2} >= {"", "pre", "post", "both"}
  assert {c.xview for c, _ in rows} >= {"plain", "slice", "sb2", "s2co", "s2d"}
  assert {c.yview for c, _ in rows} >= {"plain", "slice", "off1", "sb2", "co", "s2d"}
  assert any(c.boxes == "odd" for c, _ in rows)
  for tw in (16, 8):         # per tile form: both store forms, each with and without accumulation; per-sample bias split and not
    mine = [(c, p) for c, p in rows if p["tw"] == tw]
    st = {(p["vec_store"], p["mode"]) for c, p in mine if p["splits"] == 1}
    assert st >= {(1, 0), (1, 1), (0, 0), (0, 1)}, (tw, st)
    assert any(c.bias_b and p["splits"] > 1 for c, p in mine) and any(c.bias_b and p["splits"] == 1 and c.accumulate for c, p in mine), tw
    assert any(c.odims[0] % p["td"] and c.odims[1] % p["th"] for c, p in mine), tw             # partial in D and in H at once
  # every branch of the N-block selection
  P = plan_of
  assert P("f_n1_g7_w")["nsub"] == 1 and P("f_n2_g7_w")["nsub"] == 2                        # Npad 16, Npad 32
  assert P("f_n4_g7_w")["nsub"] == 4 and K.BY_NAME["f_n4_g7_w"].cin > 32                    # Npad 48 on 4 tiles of 16-wide sub-tiles
  assert P("n_tiles72_c20")["nsub"] == 4 and P("n_tiles72_c40")["nsub"] == 2 and P("n_tiles72_nbox")["nsub"] == 2      # 72 tiles
  assert P("n_tiles72_nbox")["n_groups"] == 8 and built("n_tiles72_nbox").ycin <= 32
  assert P("n_mw8_c40")["nsub"] == 2 and P("f_n4_g7_s")["nsub"] == 4 and P("f_n4_g7_s")["tw"] == 8                    # 8-wide sub-tiles
  # windows
  assert {c.k for c, _ in rows} >= {(3, 4, 4), (2, 5, 5), (7, 4, 4), (1, 2, 7), (5, 3, 5), (5, 4, 7), (5, 3, 9), (7, 5, 5), (2, 3, 5)}
  assert {c.k for c in CASES if c.op == "wgrad"} >= {(6, 3, 3), (1, 7, 8), (2, 5, 5), (2, 8, 8)}
  assert P("g_633_noinherit")["inherit"] == 0 and P("g_633_w8_inherit")["inherit"] == 1
  # fused epilogues: both kinds fuse on both W extents and on the wave-specialised kernel; every reachable reason to decline
  fr = [(c, plan_of(c.name)) for c in CASES if c.fuse]
  for kind in ("stats", "bnbwd"):
    assert {(c.odims, p["kind"]) for c, p in fr if c.fuse == kind and p["nparts"]} >= {((5, 9, 16), "plain"), ((6, 10, 32), "plain"), ((5, 9, 16), "ws")}
  assert all(p["nparts"] == K.parts_of(c) for c, p in fr if p["nparts"])
  assert {c.name for c, p in fr if not p["nparts"]} == {"s_decl_splits", "s_decl_scalar_store", "s_decl_ws_short", "s_decl_ndsum",
                                                         "s_decl_x_misaligned", "s_decl_sB_x"}


def test_what_no_call_reaches():
  """The arithmetic behind the table's 'unreachable' comment."""
  # a patch has at most kNUX * kThreads = 1024 staging units of 2 positions x 16 bytes x (hi, lo)
  patch = 1024 * 2 * 16 * 2
  assert 3 * 512 * 4 + patch + 2 * 7 * 4 * 4 * 16 * 16 <= 160 * 1024 - 512          # forward, NSUB 4, 5x5 planes, 512 channels
  assert 1024 + patch + 2 * 512 * 32 * 2 <= 160 * 1024 - 512                         # weight gradient, NSUB 2
  # wave-specialised kernel: PD = 8 planes, so 8 * UP <= 1024 units gives 2 * UP <= 256 = the producers' lanes, and
  assert 3 * 512 * 4 + 256 + 2 * 8 * 256 * 16 + 4 * 7 * 4 * 32 * 16 <= 160 * 1024 - 512
  # the timetable holds for every chunk count a launch can have (x->C <= 512: at most 64 chunks, 16 splits of at most 4): every
  # call that meets the kernel's conditions gets it -- its fall-back to the plain kernel is unreachable
  b = built("f_ws_1")
  for cin in range(1, 513, 3):
    xs = t.empty(K.view_numel("plain", 1, cin, (5, 9, 16))); ys = t.empty(K.view_numel("plain", 1, 24, (5, 9, 16)))
    p = be().conv_fwd_bf3_plan(K.make_view("plain", xs, 1, cin, (5, 9, 16)), None, None, 32, None, 0,
                               K.make_view("plain", ys, 1, 24, (5, 9, 16)), (5, 5, 5), (2, 2, 2), wslab=b.slab)
    assert p["kind"] == "ws" and p["per_split"] <= 4, (cin, p)
  # an accepted y has W % 8 == 0, so `D*H*W % 4 != 0` never declines a fused epilogue


def test_plan_queries_reject_what_the_launches_reject():
  """The rejections, built from the code (conv_bf3_cases.rejections); tests/test_conv_bf3_gpu.py repeats the list on the launches
  with sentinels in y / dw (the split-K scratch belongs to the library and cannot be seen from a test).  The calls next to them on the accepted side are accepted."""
  from corenet_amd import _lib
  L = be().lib
  out = _lib.CrnBf3Plan()
  def ask(op, a):
    if op == "fwd": return L._crn_conv_fwd_bf3_plan(*a["args"][:2], a["w"], None, *a["args"][2:], None, C.byref(out))
    return L._crn_conv_wgrad_bf3_plan(*a["args"], C.byref(out))
  rej, acc = K.rejections(), K.rejections(accepted=True)
  assert len(rej) >= 40
  for name, op, mk in rej:
    assert ask(op, mk("cpu")) == -1, name
  for name, op, mk in acc:
    assert ask(op, mk("cpu")) == 0, name
  # the forward query wants exactly one form of the weights, and slabs for a fuse request
  a = acc[0][2]("cpu")
  assert L._crn_conv_fwd_bf3_plan(*a["args"][:2], None, None, *a["args"][2:], None, C.byref(out)) == -1
  assert L._crn_conv_fwd_bf3_plan(*a["args"][:2], a["w"], a["w"], *a["args"][2:], None, C.byref(out)) == -1
  f = _lib.CrnBnBwdFuse(); f.ws, f.ws_bytes = a["w"], 1 << 20
  assert L._crn_conv_fwd_bf3_plan(*a["args"][:2], a["w"], None, *a["args"][2:], C.addressof(f), C.byref(out)) == -1
  assert L._crn_conv_fwd_bf3_plan(*a["args"][:2], None, a["w"], *a["args"][2:], C.addressof(f), C.byref(out)) == 0


# ------------------------------------------------------------------------------------------------ the references
def test_reference_share_of_the_bars():
  """On every row the split model (exact products of the split operands, summed in float64) is within half of the 2e-5 bar of the
  float64 reference: the other half belongs to the kernel's float32 accumulation.  And the constant behind the sharper bar is what
  this table measures: the largest float32-versus-float64 summation difference of the split model over all rows."""
  worst = 0.0
  print()
  for c in CASES:
    r = ref_of(c.name)
    worst = max(worst, r.f32_vs_split)
    print(f"  {c.name:24s} split model vs float64 {r.split_vs_f64:.2e} (half the bar {BAR / 2:.0e})   float32 sums vs float64 sums {r.f32_vs_split:.2e}")
    assert r.split_vs_f64 <= BAR / 2, c.name
  print(f"  largest float32-vs-float64 summation difference {worst:.3e}: SPLIT_BAR = 4 x {SPLIT_MAX_F32:.2e} = {SPLIT_BAR:.2e}")
  # (upper side only: torch's float32 summation order on the CPU depends on its build and the machine; a smaller figure elsewhere
  # only means the constant, measured where the table was written, is the more careful of the two)
  assert worst <= 1.25 * SPLIT_MAX_F32, worst


# ------------------------------------------------------------------------------------------------ sensitivity
def _swap_taps(b):
  """Packed weights with the centre tap of every input channel moved to the next tap: one tap read one position off."""
  kd, kh, kw = b.window
  pd, ph, pw = b.pad_lo
  tap = (min(pd, kd - 1) * kh + min(ph, kh - 1)) * kw + min(pw, kw - 2)       # reads x at (or next to) the output position
  wp = b.wp.clone().view(b.ycin, -1, b.npad)
  wp[:, [tap, tap + 1]] = wp[:, [tap + 1, tap]]
  return wp.reshape(-1)


def _box_row_dropped(b, p):
  """Packed weights with one window row INSIDE the tap box of the first channel group zeroed for that group."""
  kd, kh, kw = b.window
  wp = b.wp.clone().view(b.ycin, kd, kh, kw, b.npad)
  if p["n_groups"]:
    box = b.boxes[0][0]
    wp[:, :, box[2], :, :b.ycout // p["n_groups"]] = 0
  else:
    box = b.boxes[1][0]
    wp[:b.ycin // p["c_groups"], :, box[2]] = 0
  return wp.reshape(-1)


def mutate_fwd(kind, b, p, r):
  """The storage a forward kernel with bug `kind` would leave (float64), or None when the row cannot show that bug."""
  c = b.case
  ycin = b.ycin
  if kind in ("hi_lo_dropped", "lo_hi_dropped"):
    terms = [x for x in (("h", "h"), ("h", "l"), ("l", "h")) if x != (("h", "l") if kind == "hi_lo_dropped" else ("l", "h"))]
    return K.expected_y(b, K.split_fwd(b, terms=terms))
  if kind == "lo_of_half_chunk_dropped":
    if not p["half_last"] or ycin > 20: return None                 # (4 of more than 20 channels: below 10 bars by construction)
    keep = (t.arange(ycin) < ycin // 8 * 8).float()
    return K.expected_y(b, K.split_fwd(b, lo_keep=keep))
  if kind == "tap_shifted_by_one":
    return K.expected_y(b, K.split_fwd(b, wp=_swap_taps(b)))
  if kind == "partial_tile_row_unwritten":
    st = r.want.clone()
    v_w, v_k = K.yview(b, st), K.yview(b, b.y0.double())
    lw, lk = logical(v_w).clone(), logical(v_k)
    lw[-1, -1, -1, -1, :] = lk[-1, -1, -1, -1, :]
    write_logical(v_w, lw)
    return st
  if kind == "bias_on_every_split":
    if b.bp is None or p["splits"] <= 1: return None
    return K.expected_y(b, r.conv, bias_times=p["splits"])
  if kind == "accumulate_ignored_when_split":
    if not c.accumulate or p["splits"] <= 1: return None
    return K.expected_y(b, r.conv, accumulate=False)
  if kind == "box_row_skipped":
    if not p["rowskip"]: return None
    return K.expected_y(b, K.split_fwd(b, wp=_box_row_dropped(b, p)))
  raise ValueError(kind)


FWD_MUTATIONS = ["hi_lo_dropped", "lo_hi_dropped", "lo_of_half_chunk_dropped", "tap_shifted_by_one", "partial_tile_row_unwritten",
                 "bias_on_every_split", "accumulate_ignored_when_split", "box_row_skipped"]


@pytest.mark.parametrize("kind", FWD_MUTATIONS)
def test_forward_bar_catches_a_kernel_bug(kind):
  """Every forward row to which the bug applies sees it at 10 times the bar or more."""
  hit, least = 0, None
  for c in CASES:
    if c.op != "fwd": continue
    b, p, r = built(c.name), plan_of(c.name), ref_of(c.name)
    st = mutate_fwd(kind, b, p, r)
    if st is None: continue
    hit += 1
    err = K32.err_inside(st, r.want, r.mask, r.range)
    least = err if least is None else min(least, err)
    assert err >= 10 * BAR, f"{c.name}: {kind} moves the result by {err:.2e} of the range only"
  print(f"\n  {kind}: {hit} rows, the least visible at {least / BAR:.0f} bars")
  assert hit >= 3, kind


def test_wgrad_bar_catches_a_dropped_product_and_an_ignored_accumulate():
  hit = 0
  for c in CASES:
    if c.op != "wgrad": continue
    b, r = built(c.name), ref_of(c.name)
    xh, xl = K._split(K._x_operand(b)); dh, dl = K._split(logical(K.yview(b, b.dys)))
    corr = lambda a, d: t.nn.functional.conv3d(a.double().transpose(0, 1).contiguous(), d.double().transpose(0, 1).contiguous())
    g = t.zeros(b.ycin, b.window[0] * b.window[1] * b.window[2], b.npad, dtype=t.float64)
    g[:, :, :b.ycout] = (corr(xh, dh) + corr(xl, dh)).permute(0, 2, 3, 4, 1).reshape(b.ycin, -1, b.ycout)       # hi * lo dropped
    base = b.dw0.double() if c.accumulate else 0.0
    err = K32.err_inside(g.reshape(-1) + base, r.want, r.real, r.range)
    assert err >= 10 * BAR, f"{c.name}: a dropped product moves the gradient by {err:.2e} of the range only"
    if c.accumulate:
      hit += 1
      assert K32.err_inside(r.grad, r.want, r.real, r.range) >= 10 * BAR, c.name
  assert hit >= 3


def test_stats_bar_catches_a_position_past_the_extent():
  """One position past a partial tile counted in the sums of crn_conv_fwd_bf3_slabs_stats.  What the kernel's accumulator holds
  there is the convolution continued past the extent (the patch still sees real x under the window's reach), so the float64
  reference is computed on the same inputs with D one larger and the position (D, 0, 0) of sample 0 is added to the sums.
  Against the 3e-6 of the statistics comparison."""
  import dataclasses
  hit = 0
  for c in CASES:
    if c.fuse != "stats" or not plan_of(c.name)["nparts"]: continue
    b, r = built(c.name), ref_of(c.name)
    D, H, W = c.odims
    b2 = K.build(dataclasses.replace(c, odims=(D + 1, H, W), xdims=c.xd))
    assert t.equal(b2.xs, b.xs) and t.equal(b2.wp, b.wp) and t.equal(b2.bp, b.bp)          # the same seeded inputs
    y2 = (K32.ref_fwd_logical(b2) + K.bias_logical(b2)).relu()
    y = (r.conv + K.bias_logical(b)).relu()
    assert float((y2[:, :, :D] - y).abs().max()) <= 1e-12
    s1, s2 = y.sum((0, 2, 3, 4)), (y * y).sum((0, 2, 3, 4))
    ghost = y2[0, :, D, 0, 0]
    e1 = float(ghost.abs().max() / s1.abs().max()); e2 = float((ghost * ghost).abs().max() / s2.abs().max())
    print(f"\n  {c.name}: one position too many moves the sums by {e1:.1e} / {e2:.1e} of the largest")
    assert e1 >= 10 * 3e-6 and e2 >= 10 * 3e-6, c.name
    hit += 1
  assert hit >= 3
