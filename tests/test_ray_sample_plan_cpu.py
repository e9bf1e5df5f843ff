"""CPU side of tests/ray_cases.py (the ray-traced skip connection, csrc/ray_sample.hip): every row reaches the dispatch paths it
names (the host code of ray_fwd / ray_project / ray_scatter and the kernel's window-box decision mirrored in Python), the reference
indices are the oracle's, the float32 contract emulator stays inside the scatter bound (the bound is the reference's own), and
seeded kernel bugs miss the checks the GPU module applies.  No GPU."""
import functools
import math

import pytest
import torch as t

import ray_cases as K
from ray_cases import CASES, BY_NAME
from kernel_contract_emu import EmuBackend
from oracle import corenet_oracle as O

EMU = EmuBackend()
FWD = [c.name for c in CASES if c.op == "fwd"]
SCATTER = [c.name for c in CASES if c.op == "scatter"]


@functools.lru_cache(maxsize=None)
def indices(name):
  return K.ref_indices(BY_NAME[name])


@functools.lru_cache(maxsize=None)
def wgs(name):
  return K.workgroups(BY_NAME[name], indices(name)[0])


@functools.lru_cache(maxsize=None)
def built(name, grad=None):
  return K.build(BY_NAME[name], grad)


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("name", [c.name for c in CASES if c.zero_first and c.grad == "randn"])
def test_reference_indices_are_the_oracles(name):
  """The reference indices are O.ray_sample_indices' wherever the float -> int cast is defined, and outside where it is not (u or v
  not finite or beyond int32); K.project, which the kernel emulation evaluates at arbitrary voxels, gives the same on the grid.  On
  maps below 65535 pixels they are the contract emulator's saved index tensor, and the gather reference is the oracle's gather."""
  c = BY_NAME[name]
  idx, mine = indices(name)
  assert t.equal(idx, mine)
  assert bool(((idx >= -1) & (idx < c.hw)).all())
  m, off = K.cameras(c)
  h, w = c.map
  hostile_row = c.name.startswith(("f_pw0", "f_cut", "s_cut"))
  if c.hw < 65535:
    u16 = EmuBackend.ray_indices_u16(m.reshape(c.B, 16), off, c.B, *c.grid, h, w)
    differs = t.where(u16 == 0xFFFF, t.full_like(u16, -1), u16) != idx
    assert hostile_row or not bool(differs.any())
    assert bool((idx[differs] == -1).all())
  if c.op == "fwd":
    b = built(name)
    want = O.ray_sample(b.map, m, off, c.grid)
    got = K.ref_gather(c, b, idx)
    same = (got == want).all(1)
    assert hostile_row or bool(same.all())
    assert bool((idx[~same] == -1).all())
  assert float((idx >= 0).float().mean()) > 0.05, "hardly any voxel lands in the image"
  if "shift" in c.cams:
    assert float((idx[c.cams.index("shift")] < 0).float().mean()) > 0.05, "the shifted camera leaves no voxel outside"


# ------------------------------------------------------------------------------------------------ path coverage
def _cl_conditions(c):
  ptr, sB, sC, sP = c.map_geom
  return dict(sC=sC == 1, sP=sP % 4 == 0, sB=sB % 4 == 0, C=c.C % 4 == 0, ptr=(ptr * 4) % 16 == 0)


def _v4_conditions(c):
  return dict(W=c.grid[2] % 4 == 0, out_sB=c.out_sB % 4 == 0, out_ptr=(c.out_ptr * 4) % 16 == 0, idx_ptr=(c.idx_off * 2) % 8 == 0)


def _only_fails(conds, key):
  return not conds[key] and all(v for k, v in conds.items() if k != key)


def _lg(c):
  return max(0, math.ceil(math.log2(c.S)))


def _nonfinite_ref(c, name):
  r = K.ScatterRef(c, built(name), indices(name)[0]).ref
  gy = built(name).gy
  nan_in = t.zeros(c.B, c.C, c.hw + 1, dtype=t.bool)
  idx = indices(name)[0]
  for b, ch, z, y, x in t.isnan(gy).nonzero().tolist():
    nan_in[b, ch, idx[b, z, y, x]] = True
  born = t.isnan(r).reshape(c.B, c.C, c.hw) & ~nan_in[:, :, :c.hw]        # +inf and -inf met on a pixel
  return bool(t.isposinf(r).any() and t.isneginf(r).any() and nan_in[:, :, :c.hw].any() and born.any())


PATHS = {
    "fwd<1,false>": lambda c, n: K.fwd_path(c)[:2] == (1, False) and K.fwd_path(c, False)[:2] == (1, False),
    "fwd<1,true>": lambda c, n: K.fwd_path(c)[:2] == (1, True),
    "fwd<4,false>": lambda c, n: K.fwd_path(c)[:2] == (4, False),
    "fwd<4,true>": lambda c, n: K.fwd_path(c)[:2] == (4, True),
    "project<1>": lambda c, n: K.project_path(c) == (1, "u16"),
    "project<4,i32>": lambda c, n: K.project_path(c) == (4, "i32"),
    "idx_store<1>": lambda c, n: K.fwd_path(c, True)[0] == 1,
    "two_groups_full_then_leftover": lambda c, n: K.fwd_path(c)[2] > 1 and K.fwd_path(c)[3],
    "one_group_full_then_leftover": lambda c, n: K.fwd_path(c)[2] == 1 and K.fwd_path(c)[3],
    "leftover_only": lambda c, n: c.C < 12,
    "cl_fail_sP": lambda c, n: _only_fails(_cl_conditions(c), "sP"),
    "cl_fail_sB": lambda c, n: _only_fails(_cl_conditions(c), "sB"),
    "cl_fail_ptr": lambda c, n: _only_fails(_cl_conditions(c), "ptr") and c.layout == "cl_slice",
    "cl_slice_aligned": lambda c, n: all(_cl_conditions(c).values()) and c.layout == "cl_slice" and c.cl_slice[0] > 0,
    "v4_fail_out_ptr": lambda c, n: _only_fails(_v4_conditions(c), "out_ptr"),
    "v4_fail_out_sB": lambda c, n: _only_fails(_v4_conditions(c), "out_sB"),
    "v4_fail_idx_ptr": lambda c, n: _only_fails(_v4_conditions(c), "idx_ptr") and K.fwd_path(c, False)[0] == 4,
    "noncubic_grid": lambda c, n: len(set(c.grid)) == 3,
    "nonsquare_map": lambda c, n: c.map[0] != c.map[1] and c.map[1] > 1,
    "pw_sign_change": lambda c, n: sum(w["both_signs"] for w in wgs(n)) >= 1,
    "pw_zero_plane": lambda c, n: all(bool((K.pw_of(c)[b] == 0).any()) for b in range(c.B)) and bool((indices(n)[0][K.pw_of(c) == 0] == -1).all()),
    "D<8": lambda c, n: c.grid[0] < 8 and K.scatter_plan(c)["zseg"] == c.grid[0],
    "tile8x8_partial": lambda c, n: K.scatter_plan(c)["kTX"] == 8 and any(w["partial"] for w in wgs(n)),
    "tile32x8_partial": lambda c, n: (K.scatter_plan(c)["kTX"], K.scatter_plan(c)["kTY"]) == (32, 8) and any(w["partial"] for w in wgs(n))
                                     and c.grid[1] % 8 != 0 and c.grid[2] % 32 != 0,
    "window": lambda c, n: any(w["kind"] == "window" for w in wgs(n)) and any(w["kind"] == "window" and w["partial"] for w in wgs(n)),
    "channel_clamp": lambda c, n: c.C % K.scatter_plan(c)["CN"] != 0,
    "full_groups": lambda c, n: c.C % K.scatter_plan(c)["CN"] == 0,
    "det_CN12": lambda c, n: c.deterministic and K.scatter_plan(c)["CN"] == 12 and K.scatter_plan(c)["win_floats"] == 0,
    "det_CN4": lambda c, n: c.deterministic and K.scatter_plan(c)["CN"] == 4 and K.scatter_plan(c)["win_floats"] == 0,
    "det_maxabs_scale_finish": lambda c, n: c.deterministic,
    "det_finish_strided": lambda c, n: c.deterministic and c.dmap_sB != c.C * c.hw,
    "i32_window": lambda c, n: K.scatter_plan(c)["IT"] == "i32" and c.entry == "plain" and sum(w["kind"] == "window" for w in wgs(n)) >= 1,
    "i32_box_too_large": lambda c, n: K.scatter_plan(c)["IT"] == "i32" and sum(w["kind"] == "too_large" for w in wgs(n)) >= 1,
    "i32_det": lambda c, n: K.scatter_plan(c)["IT"] == "i32" and c.deterministic,
    "u16_box_too_large": lambda c, n: K.scatter_plan(c)["IT"] == "u16" and sum(w["kind"] == "too_large" for w in wgs(n)) >= 1,
    "run_outside_box": lambda c, n: sum(w["kind"] == "window" and w["outside_runs"] for w in wgs(n)) >= 1,
    "memset_per_sample": lambda c, n: K.scatter_plan(c)["memset_per_sample"],
    "dout_slice": lambda c, n: c.dout_sB != c.C * c.S and c.dout_ptr > 0,
    "width_one_reshape": lambda c, n: K.scatter_plan(c)["reshaped"] and (K.scatter_plan(c)["h"], K.scatter_plan(c)["w"]) == (1, c.map[0]),
    # the scale 2^(61 - lg - e) of the whole tensor's max is beyond float32: exponent > 127
    "det_tiny_scale": lambda c, n: c.deterministic and 61 - _lg(c) - math.frexp(float(built(n).gy.abs().max()))[1] > 127,
    "det_nonfinite": lambda c, n: c.deterministic and _nonfinite_ref(c, n),
    "det_zero": lambda c, n: c.deterministic and float(built(n).gy.abs().max()) == 0.0,
}


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_case_reaches_the_paths_it_names(name):
  c = BY_NAME[name]
  assert c.paths, f"{name} names no path"
  for p in c.paths:
    assert PATHS[p](c, name), f"{name} does not reach {p}"


def test_every_path_of_the_list_is_named():
  named = {p for c in CASES for p in c.paths}
  assert not set(K.REQUIRED_PATHS) - named, sorted(set(K.REQUIRED_PATHS) - named)
  assert not named - set(PATHS), sorted(named - set(PATHS))
  # every scatter shape in all four (mode, zero_first) combinations unless it is about the deterministic branch alone
  for c in CASES:
    if c.op == "scatter" and not c.deterministic and c.zero_first:
      assert all(c.name + s in BY_NAME for s in ("_acc", "_det", "_det_acc")), c.name
    if c.op == "scatter" and c.entry == "both":
      assert c.hw < 65535


def test_int32_window_case_counts():
  """2 x 128 x 128 | 256 x 256: of the 192 workgroups 60 take the LDS window and 116 overflow it (16 see no corner in the image)."""
  kinds = [w["kind"] for w in wgs("s_i32")]
  assert len(kinds) == 192
  assert kinds.count("window") >= 1 and kinds.count("too_large") >= 1
  print({k: kinds.count(k) for k in set(kinds)})


def test_plane_cut_and_zoom_conditions():
  cut = wgs("s_cut")
  assert sum(w["both_signs"] for w in cut) >= 1 and sum(w["kind"] == "window" and w["outside_runs"] for w in cut) >= 1
  assert sum(w["kind"] == "too_large" for w in wgs("s_zoom")) >= 1 and K.scatter_plan(BY_NAME["s_zoom"])["win_floats"] < 6 * 1024
  print("plane cut:", sum(w["both_signs"] for w in cut), "tiles with both signs,", sum(w["outside_runs"] for w in cut), "with runs outside the box;",
        "zoom:", sum(w["kind"] == "too_large" for w in wgs("s_zoom")), "boxes too large")


# ------------------------------------------------------------------------------------------------ the bound is the reference's own
def _finite(c):
  return c.grad != "nonfinite"


@pytest.mark.parametrize("name", [n for n in SCATTER if _finite(BY_NAME[n])])
def test_contract_emulator_is_inside_the_bound(name):
  """Sequential float32 index_add_ (EmuBackend.ray_sample_bwd_idx / ray_sample_bwd) against the float64 reference."""
  c, b = BY_NAME[name], built(name)
  idx = indices(name)[0]
  ref = K.ScatterRef(c, b, idx)
  st = b.dmap0.clone()
  if c.entry == "both":
    i16 = t.where(idx >= 0, idx, t.full_like(idx, 0xFFFF)).to(t.int32).to(t.int16)
    EMU.ray_sample_bwd_idx(b.dout_st[c.dout_ptr:], c.dout_sB, c.B, c.C, *c.grid, i16, st[c.dmap_ptr:], c.dmap_sB, *c.map, c.zero_first)
  else:
    EMU.ray_sample_bwd(b.dout_st[c.dout_ptr:], c.dout_sB, c.B, c.C, *c.grid, b.m.reshape(c.B, 16), b.off, st[c.dmap_ptr:], c.dmap_sB, *c.map,
                       c.zero_first)
  ratio, kinds, rest = ref.check(c, b, st)
  assert kinds and rest
  assert ratio <= 1.0, f"{name}: the float32 emulator is at {ratio:.2f} of the bound"
  assert float(ref.n.max()) >= 2 and float(ref.bound.max()) > 0 or c.grad == "zero"


@pytest.mark.parametrize("name", [n for n in SCATTER if BY_NAME[n].grad == "randn"])
def test_integer_gradients_are_exact_in_the_reference(name):
  """The float64 sums of integer gradients (also times 2^40 and 2^-40) are float32 numbers: rounding them changes nothing."""
  c = BY_NAME[name]
  for e in (0, 40, -40):
    b = K.scaled(built(name, "int"), e)
    ref = K.ScatterRef(c, b, indices(name)[0])
    assert t.equal(ref.ref.float().double(), ref.ref)
    assert ref.exact(c, K.emu_scatter(c, b, indices(name)[0]))


# ------------------------------------------------------------------------------------------------ seeded bugs
def _fwd_ok(name, bug):
  c, b = BY_NAME[name], built(name)
  want = K.want_fwd(c, b, indices(name)[0])
  got = K.emu_fwd(c, b, bug)
  return t.equal(got[0].view(t.int32), want[0].view(t.int32)), t.equal(got[1], want[1])


def _scatter_ok(name, bug):
  c, b = BY_NAME[name], built(name)
  idx = indices(name)[0]
  ratio, kinds, rest = K.ScatterRef(c, b, idx).check(c, b, K.emu_scatter(c, b, idx, bug))
  return ratio <= 1.0 and kinds and rest


@pytest.mark.parametrize("name", FWD)
def test_forward_emulation_without_a_bug_passes(name):
  assert _fwd_ok(name, None) == (True, True)


@pytest.mark.parametrize("name", SCATTER)
def test_scatter_emulation_without_a_bug_passes(name):
  assert _scatter_ok(name, None)


@pytest.mark.parametrize("bug", ["swap_hw", "swap_HD", "drop_leftover"])
def test_seeded_forward_bug_fails(bug):
  failing = [n for n in FWD if _fwd_ok(n, bug) != (True, True)]
  print(bug, "fails", failing)
  assert failing, f"no forward row notices {bug}"
  if bug != "drop_leftover":          # the index tensor alone (crn_ray_project's check) notices too
    assert [n for n in FWD if not _fwd_ok(n, bug)[1]]
  # ... and the cubic grids / square maps of the older tests would not have: the bug is invisible on them
  if bug == "swap_HD":
    assert all(len(set(BY_NAME[n].grid)) > 1 for n in failing)
  if bug == "swap_hw":
    assert all(BY_NAME[n].map[0] != BY_NAME[n].map[1] for n in failing)


@pytest.mark.parametrize("bug", ["drop_outside", "zero_stride", "no_clamp"])
def test_seeded_scatter_bug_fails(bug):
  failing = [n for n in SCATTER if not _scatter_ok(n, bug)]
  print(bug, "fails", failing)
  assert failing, f"no scatter row notices {bug}"
  if bug == "zero_stride":
    assert all(BY_NAME[n].dmap_slice[1] and BY_NAME[n].zero_first for n in failing)
  if bug == "drop_outside":
    assert any(n.startswith("s_cut") for n in failing)


# ------------------------------------------------------------------------------------------------ the mirror against known plans
@pytest.mark.parametrize("res,C,tile,win", [(8, 96, (8, 8), 576), (16, 48, (8, 8), 576), (32, 24, (8, 8), 576), (64, 12, (32, 8), 1728)])
def test_mirror_reproduces_the_decoder_scales(res, C, tile, win):
  """The four decoder scales (map = grid): 8 x 8 tiles below 64^3, 32 x 8 at 64^3; the window holds (kTX + 4)(kTY + 4) pixels of
  4 channels, 8 bytes each: 144 x 4 and 432 x 4 entries; none in deterministic mode, which takes 12 channels per workgroup."""
  for det in (False, True):
    p = K.scatter_plan(K.Case("scale", "scatter", (res,) * 3, (res, res), C, deterministic=det))
    assert (p["kTX"], p["kTY"]) == tile and p["zseg"] == 8 and p["nseg"] == res // 8
    assert p["win_floats"] == (0 if det else win) and p["CN"] == (12 if det else 4) and p["IT"] == "u16" and not p["reshaped"]
  c = K.Case("scale", "fwd", (res,) * 3, (res, res), C, layout="cl")
  assert K.fwd_path(c) == (4, True, C // 12, False) and K.project_path(c) == (4, "u16")
