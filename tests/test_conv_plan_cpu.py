"""What the fp32 conv-engine case table (tests/conv_fp32_cases.py) reaches, asked of the plan query on the CPU
(crn_conv_fwd_plan / crn_conv_wgrad_plan: the selection code the launches themselves run), and whether the table's float64
references can carry the bars of tests/test_conv_fp32_gpu.py: conditioning of the inputs and sensitivity to ten kernel bugs."""
import ctypes as C
import functools
import os

import pytest
import torch as t

import conv_fp32_cases as K
from conv_fp32_cases import CASES, BAR_FWD, BAR_WGRAD
from kernel_contract_emu import EmuBackend, logical, write_logical

EMU = EmuBackend()
# CRN_DETERMINISTIC=1 makes the library ask for no position / slice splits: `splits` is then left out of the comparisons, as
# tests/test_conv_fp32_gpu.py does
_DET_ENV = os.environ.get("CRN_DETERMINISTIC", "0") == "1"
FWD_CONFIGS = [(8, 1), (4, 2), (4, 1), (2, 4), (2, 2), (2, 1), (1, 4), (1, 2), (1, 1)]     # CRN_FWD_CONFIGS = CRN_WG_CONFIGS
IDS = [c.name for c in CASES]

# What no shape reaches.  Every instantiated kernel IS reached, and so is the forced scalar fall-back of the forward selection
# (e_forced: position pairs chosen for a stride-2 view, but an output one position wide has no tile of even width).
UNREACHABLE = {
    "wg_select: second search behind a failed re-derivation":
        "The candidate is re-derived for the variant that runs when x or dy is staged as scalars.  The re-derived call differs "
        "from the accepted one only in staging dy as scalars, whose slot limit NB * 2^ceil(log2 npos) <= 8192 holds whenever the "
        "float4 limit NB * npos <= 8192 with npos <= 512 does (NB is 16, 32 or 64), and in an LDS budget of 150 KiB instead of "
        "72 KiB: wg_cand cannot reject what it accepted.  It selects no kernel of its own.",
}


@functools.lru_cache(maxsize=None)
def be():
  from corenet_amd.backend import HipBackend
  return HipBackend()          # loads the library; no GPU is touched by the plan queries


@functools.lru_cache(maxsize=None)
def built(name):
  return K.build(K.BY_NAME[name])


@functools.lru_cache(maxsize=None)
def plan_of(name):
  b = built(name)
  c = b.case
  be().lib.crn_set_deterministic(int(c.deterministic or _DET_ENV))
  try:
    return K.query_plan(be(), b, b.xs, b.y0 if c.op == "fwd" else b.dys, b.wp, None if c.op == "fwd" else b.dw0)
  finally:
    be().lib.crn_set_deterministic(int(_DET_ENV))        # the state CRN_DETERMINISTIC gives the process


@functools.lru_cache(maxsize=None)
def ref_of(name):
  b = built(name)
  return K.FwdRef(b) if b.case.op == "fwd" else K.WgradRef(b)


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("name", IDS)
def test_every_case_gets_the_variant_its_row_names(name):
  c = K.BY_NAME[name]
  p = plan_of(name)
  want = {k: v for k, v in c.expect.items() if not (_DET_ENV and k == "splits")}
  got = {k: p[k] for k in want}
  assert got == want, f"{name}: the plan query says {got}, the row is there for {want}"
  # invariants of any plan
  assert p["lds_bytes"] <= p["lds_budget"], p
  assert 1 <= p["splits"] <= max(1, p["chunks"]), p
  if p["path"] == "generic":
    assert (p["msub"], p["nsub"]) in FWD_CONFIGS
    if c.op == "fwd":
      if p["xstage"]: assert p["tw"] % (4 if p["xstage"] == 1 else 2) == 0 and not p["forced"], p
      assert p["cc"] % 4 == 0 and p["chunks"] == -(-built(name).ycin // p["cc"])
    else:
      if p["xstage"] or p["dystage"]: assert p["tw"] % 4 == 0, p
      assert p["td"] * p["th"] * p["tw"] <= 512


def test_table_reaches_every_instantiated_kernel():
  fwd = {(p["msub"], p["nsub"], p["xstage"]) for c in CASES if c.op == "fwd" for p in [plan_of(c.name)] if p["path"] == "generic"}
  wg = {(p["msub"], p["nsub"], p["xstage"], p["dystage"]) for c in CASES if c.op == "wgrad" for p in [plan_of(c.name)]
        if p["path"] == "generic"}
  assert fwd == {(m, n, x) for m, n in FWD_CONFIGS for x in (0, 1, 2)}, "forward kernels not reached"
  assert wg == {(m, n) + v for m, n in FWD_CONFIGS for v in ((0, 0), (1, 0), (1, 1), (1, 2))}, "weight-gradient kernels not reached"
  assert {plan_of(c.name)["path"] for c in CASES} == {"dense_cols", "dense_rows", "dense_wgrad", "pointwise", "generic"}
  gen = [plan_of(c.name) for c in CASES if c.op == "fwd" and plan_of(c.name)["path"] == "generic"]
  assert {p["forced"] for p in gen} == {0, 1} and {p["vec_store"] for p in gen} == {0, 1}
  assert {plan_of(c.name)["balanced"] for c in CASES if c.op == "wgrad"} == {0, 1}
  # what the model's own layer shapes reached before this table (the nine `conv` rows of test_kernels_gpu.CONV_CASES):
  # (1,1) (1,2) (1,4) (2,4) (4,2) (8,1), all with float4 staging -- 6 of the 27


def test_table_carries_every_edge_once_per_staging_form():
  rows = [(c, plan_of(c.name)) for c in CASES if c.op == "fwd" and plan_of(c.name)["path"] == "generic" and c.geom == "conv"]
  for xs in (0, 1, 2):
    mine = [(c, p) for c, p in rows if p["xstage"] == xs]
    assert {c.tr for c, _ in mine} >= {"shift", "pre", "post", "both", "scale"}, xs
    assert {c.pad[2] % (2 if xs == 2 else 4) for c, _ in mine} == set(range(2 if xs == 2 else 4)), xs      # every vec_lead
    assert any(c.cin % p["cc"] and c.cin > p["cc"] for c, p in mine), xs                                    # ragged last chunk
    assert any(c.cin < 4 for c, _ in mine), xs
    assert any(c.cout < c.npad for c, _ in mine) and any(c.cout % (16 * p["nsub"]) for c, p in mine), xs
    assert any(all(o % tl for o, tl in zip(c.odims, (p["td"], p["th"], p["tw"]))) for c, p in mine), xs     # partial in D, H, W
    assert any(p["splits"] > 1 for _, p in mine) and any(c.bias and c.accumulate for c, _ in mine), xs
  assert {p["mw"] for c, p in rows if c.odims[2] <= 3} == {1, 2}
  assert {c.xview for c, _ in rows} >= {"plain", "slice", "off1", "sb2", "s2", "s2co", "s2d"}
  assert {c.yview for c, _ in rows} >= {"plain", "slice", "off1", "sb2", "co"}
  assert any(c.odims[2] % 4 for c, _ in rows)


def test_named_claims_of_the_dispatch():
  P = plan_of
  assert P("e_1x1x1_cin1")["xstage"] == 0 and (P("e_1x1x1_cin1")["msub"], P("e_1x1x1_cin1")["nsub"]) == (1, 1)
  assert P("e_s2_oddw")["xstage"] == 0 and P("e_s2co_oddk")["xstage"] == 2          # odd W on a stride-2 input: scalars
  assert P("e_forced")["forced"] == 1 and P("e_forced")["xstage"] == 0
  assert P("p_c2048_s4")["path"] == "pointwise" and P("p_c2052_notr")["path"] == "pointwise"
  assert P("p_c2052_tr_generic")["path"] == "generic"                              # past the LDS tables of the pointwise kernel
  assert P("p_blocks255")["splits"] > 1 and P("p_blocks256")["splits"] == 1
  assert P("p_c260_s68")["splits"] == 2                                            # slices of 160 and 100 channels
  assert P("d_cols_1024")["path"] == P("d_cols_1030_b3")["path"] == P("d_cols_b8_c2048")["path"] == "dense_cols"
  assert P("d_cols_c2049_leaves")["path"] == "generic"
  assert P("d_b9_generic")["path"] == "generic" and P("d_b9_generic")["mw"] == 1
  assert _DET_ENV or (P("d_rows_4096")["splits"] == 2 and P("d_rows_4100")["splits"] == 2)      # atomic slices: not when deterministic
  assert P("d_rows_1024")["splits"] == 1
  assert P("d_rows_4100_nc")["splits"] == 1 and P("d_rows_4100_nc")["path"] == "dense_rows"
  assert P("d_rows_scale_leaves")["path"] == "generic"
  assert P("s_5chunks_4asked_b")["chunks"] == 5 and P("s_5chunks_4asked_b")["splits"] == 3
  assert P("s_4chunks_3asked_b")["chunks"] == 4 and P("s_4chunks_3asked_b")["splits"] == 2
  assert P("s_more_than_chunks_b")["splits"] == P("s_more_than_chunks_b")["chunks"]
  assert P("w_det")["splits"] == 1
  assert P("w_convT_balanced")["balanced"] == 1 and P("w_boxes_ignored")["balanced"] == 0
  assert P("w_t512")["path"] == "generic" and P("w_t512")["cc"] == 1               # T = 512: one channel per block row


def _raw_views(B=2, cin=8, cout=16, dims=(2, 4, 8)):
  from corenet_amd.backend import _cview
  xs = t.zeros(B * cin * dims[0] * dims[1] * dims[2]); ys = t.zeros(B * cout * dims[0] * dims[1] * dims[2])
  return xs, ys, _cview(K.make_view("plain", xs, B, cin, dims)), _cview(K.make_view("plain", ys, B, cout, dims))


def test_plan_queries_reject_what_the_launch_rejects():
  from corenet_amd import _lib
  L = be().lib
  xs, ys, xv, yv = _raw_views()
  out = _lib.CrnConvPlan()
  w = xs.data_ptr()
  def fwd(x=xv, y=yv, npad=16, k=(3, 3, 3), boxes=None):
    return L._crn_conv_fwd_plan(C.byref(x), None, w, npad, None, 0, C.byref(y), *k, 1, 1, 1, 0, 0, boxes, C.byref(out))
  def wg(x=xv, y=yv, npad=16, k=(3, 3, 3)):
    return L._crn_conv_wgrad_plan(C.byref(x), None, C.byref(y), w, npad, *k, 1, 1, 1, 1, None, C.byref(out))
  assert fwd() == 0 and wg() == 0
  assert fwd(npad=24) == -1 and wg(npad=24) == -1                      # Npad not a multiple of 16
  _, _, _, y17 = _raw_views(cout=17)
  assert fwd(y=y17) == -1                                              # Cout > Npad
  _, _, x3, _ = _raw_views(B=3)
  assert fwd(x=x3) == -1 and wg(x=x3) == -1                            # batch mismatch
  for n, cg in ((9, 0), (0, 9), (-1, 0)):
    tb = _lib.CrnTapBoxes(); tb.n_groups, tb.c_groups = n, cg
    assert fwd(boxes=C.cast(C.pointer(tb), C.c_void_p)) == -1          # tap-box group counts out of range
  assert fwd(k=(6, 6, 6)) == -1                                        # no configuration holds a 6^3 window's weight chunk
  assert wg(k=(8, 8, 8)) == 0 and wg(k=(8, 8, 9)) == -1                # T = 512 is the last window the weight gradient takes


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("name", IDS)
def test_reference_side_alone_is_within_a_third_of_the_bar(name):
  """The float32 contract emulator against the float64 reference: what is left of the bar belongs to the kernel.  And the packed
  form of the reference (the one the sensitivity test mutates) is the operator torch computes in the reference layout."""
  b = built(name)
  c = b.case
  r = ref_of(name)
  from corenet_amd.backend import Transform
  if c.op == "fwd":
    got = K.run_fwd(EMU, b, "cpu")
    err, outside = r.check(b, got)
    assert outside and err <= BAR_FWD / 3, f"{name}: float32 emulator {err:.2e} of the range, outside intact: {outside}"
    assert float((K.corr_logical(b) - K.ref_fwd_logical(b)).abs().max()) <= 1e-12 * max(r.range, 1.0)
  else:
    got = K.run_wgrad(EMU, b, "cpu")
    err, pad_ok = r.check(b, got)
    assert pad_ok and err <= BAR_WGRAD / 3, f"{name}: float32 emulator {err:.2e} of the range"


# ------------------------------------------------------------------------------------------------ sensitivity
def _center_tap(b):
  kd, kh, kw = b.window
  pd, ph, pw = b.pad_lo
  return (min(pd, kd - 1) * kh + min(ph, kh - 1)) * kw + min(pw, kw - 1)       # reads x at (or next to) the output position


def _keep_below(b, n):
  return (t.arange(b.ycin) < n).double()


def _split_channels(b, p):
  """First input channel of the last split of a forward plan (None: the launch does not split its channels)."""
  if p["splits"] <= 1: return None
  if p["path"] == "generic": return (p["splits"] - 1) * -(-p["chunks"] // p["splits"]) * p["cc"]
  if p["path"] == "pointwise": return (p["splits"] - 1) * ((-(-b.ycin // p["splits"]) + 31) // 32 * 32)
  if p["path"] == "dense_rows": return (p["splits"] - 1) * -(-b.ycin // p["splits"])
  return None


def _has_pad(b):
  c = b.case
  return any(lo > 0 or o + k - 1 - lo - x > 0 for lo, o, k, x in zip(b.pad_lo, c.odims, b.window, c.xd))


def mutate_fwd(kind, b, p, r):
  """The storage a forward kernel with bug `kind` would leave (float64), or None when the case cannot show that bug."""
  c = b.case
  conv = lambda **kw: K.expected_y(b, K.corr_logical(b, **kw))
  if kind == "tap_dropped":
    if c.geom != "conv": return None
    wp = b.wp.clone(); wp.view(b.ycin, -1, b.npad)[b.ycin - 1, _center_tap(b)] = 0
    return conv(wp=wp)
  if kind == "patch_shifted_one_column":
    if c.geom != "conv": return None
    return conv(pad_lo=(b.pad_lo[0], b.pad_lo[1], b.pad_lo[2] + 1))
  if kind == "zero_pad_transformed":
    if c.geom != "conv" or c.tr in ("", "scale") or not _has_pad(b): return None
    return conv(pad_first=True)
  if kind == "ragged_chunk_skipped":
    cc = p["cc"] if p["path"] in ("generic", "pointwise") else 0
    if not cc or b.ycin % cc == 0 or b.ycin < cc: return None
    return conv(chan_keep=_keep_below(b, b.ycin // cc * cc))
  if kind == "last_split_skipped":
    first = _split_channels(b, p)
    return None if first is None else conv(chan_keep=_keep_below(b, first))
  if kind == "bias_on_every_split":
    if not c.bias or p["splits"] <= 1: return None
    return K.expected_y(b, K.corr_logical(b), bias_times=p["splits"])
  if kind == "bias_never":
    return K.expected_y(b, K.corr_logical(b), bias_times=0) if c.bias else None
  if kind == "accumulate_ignored":
    if not c.accumulate: return None
    st = K.expected_y(b, K.corr_logical(b), accumulate=False)
    return st
  if kind == "column_past_cout_written":
    if bool(r.mask.all()): return None
    st = r.want.clone()
    first_out = int((~r.mask).nonzero()[0])
    st[first_out] = 0.0
    return st
  if kind == "partial_tile_row_unwritten":
    if p["path"] != "generic" or not any(o % tl for o, tl in zip(c.odims, (p["td"], p["th"], p["tw"]))): return None
    st = r.want.clone()
    keep = b.y0.double()
    v_w, v_k = K.yview(b, st), K.yview(b, keep)
    lw, lk = logical(v_w).clone(), logical(v_k)
    lw[-1, -1, -1, -1, :] = lk[-1, -1, -1, -1, :]
    write_logical(v_w, lw)
    return st
  raise ValueError(kind)


FWD_MUTATIONS = ["tap_dropped", "patch_shifted_one_column", "zero_pad_transformed", "ragged_chunk_skipped", "last_split_skipped",
                 "bias_on_every_split", "bias_never", "accumulate_ignored", "column_past_cout_written", "partial_tile_row_unwritten"]


@pytest.mark.parametrize("kind", FWD_MUTATIONS)
def test_forward_bars_catch_a_kernel_bug(kind):
  """Every forward row to which the bug applies sees it at 10 times its bar or more (a write outside the view: at all)."""
  hit = 0
  for c in CASES:
    if c.op != "fwd": continue
    b, p, r = built(c.name), plan_of(c.name), ref_of(c.name)
    st = mutate_fwd(kind, b, p, r)
    if st is None: continue
    hit += 1
    err, outside = r.check(b, st.float() if kind == "column_past_cout_written" else st)
    if kind == "column_past_cout_written":
      assert not outside, c.name
    else:
      assert err >= 10 * BAR_FWD, f"{c.name}: {kind} moves the result by {err:.2e} of the range only"
  assert hit >= 3, kind


def _last_split_positions(c, p):
  """0/1 over [B, 1, D, H, W]: the output positions outside the last position-tile split of a weight-gradient plan.  Tiles are
  numbered ((b * tilesD + d) * tilesH + h) * tilesW + w and split s takes tiles [s * tps, (s + 1) * tps) (conv_wgrad_kernel)."""
  D, H, W = c.odims
  td, th, tw = p["td"], p["th"], p["tw"]
  nd, nh, nw = -(-D // td), -(-H // th), -(-W // tw)
  tps = -(-p["chunks"] // p["splits"])
  keep = t.ones(c.B, 1, D, H, W)
  for tile in range((p["splits"] - 1) * tps, p["chunks"]):
    wi, r = tile % nw, tile // nw
    hi, r = r % nh, r // nh
    di, bi = r % nd, r // nd
    keep[bi, 0, di * td:(di + 1) * td, hi * th:(hi + 1) * th, wi * tw:(wi + 1) * tw] = 0
  return keep


# The other three of the forward mutations have no weight-gradient form: there is no bias, and the weight gradient writes
# whole dw rows per block (no partial-tile epilogue: a partial position tile only shortens a sum, which tap_dropped and
# last_split_skipped cover).
WGRAD_MUTATIONS = ["tap_dropped", "patch_shifted_one_column", "zero_pad_transformed", "accumulate_ignored", "ragged_chunk_skipped",
                   "last_split_skipped", "column_past_cout_written"]


@pytest.mark.parametrize("kind", WGRAD_MUTATIONS)
def test_wgrad_bars_catch_a_kernel_bug(kind):
  hit = 0
  for c in CASES:
    if c.op != "wgrad": continue
    b, r, p = built(c.name), ref_of(c.name), plan_of(c.name)
    base = b.dw0.double() if c.accumulate else 0.0
    if kind == "ragged_chunk_skipped":                      # the dw rows of the last, short channel block stay as they were
      cc = p["cc"] if p["path"] == "generic" else 0
      if not cc or b.ycin % cc == 0 or b.ycin < cc: continue
      g = r.want.clone()
      first = b.ycin // cc * cc
      g.view(b.ycin, -1, b.npad)[first:] -= r.grad.view(b.ycin, -1, b.npad)[first:]
    elif kind == "last_split_skipped":                      # (balanced plans split per group: not modelled)
      if p["path"] != "generic" or p["splits"] <= 1 or p["balanced"]: continue
      g = K.ref_wgrad_packed(b, dy_keep=_last_split_positions(c, p)) + base
    elif kind == "column_past_cout_written":
      if c.boxes == "geom" or bool(r.real.all()): continue
      g = r.want.clone().float()
      g[int((~r.real).nonzero()[0])] = 1.0
      hit += 1
      assert not r.check(b, g)[1], c.name
      continue
    elif kind == "tap_dropped":
      g = r.want.clone()
      rows = g.view(b.ycin, -1, b.npad)
      tap = _center_tap(b) if c.geom == "conv" else int(r.real.view(b.ycin, -1, b.npad)[b.ycin - 1].any(1).nonzero()[0])
      rows[b.ycin - 1, tap] -= r.grad.view(b.ycin, -1, b.npad)[b.ycin - 1, tap]
    elif kind == "patch_shifted_one_column":
      if c.geom != "conv": continue
      g = K.ref_wgrad_packed(b, pad_lo=(b.pad_lo[0], b.pad_lo[1], b.pad_lo[2] + 1)) + (b.dw0.double() if c.accumulate else 0.0)
    elif kind == "zero_pad_transformed":
      if c.geom != "conv" or c.tr in ("", "scale") or not _has_pad(b): continue
      g = K.ref_wgrad_packed(b, pad_first=True) + (b.dw0.double() if c.accumulate else 0.0)
    else:
      if not c.accumulate: continue
      g = r.grad.clone()
    hit += 1
    err, _ = r.check(b, g)
    assert err >= 10 * BAR_WGRAD, f"{c.name}: {kind} moves the gradient by {err:.2e} of the range only"
  assert hit >= 3 or (_DET_ENV and kind == "last_split_skipped"), kind        # (deterministic mode splits no positions)
