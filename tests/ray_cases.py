"""The case table of the ray-traced skip connection (csrc/ray_sample.hip: crn_ray_sample_fwd, crn_ray_sample_fwd_idx,
crn_ray_project, crn_ray_sample_bwd_idx, crn_ray_sample_bwd) and what its tests share.  TEST INFRASTRUCTURE ONLY.

One row = one call shape: grid D x H x W, map h x w, C channels, one camera per sample, the layout of every tensor.  The rows
are the smallest shapes that reach each dispatch path of ray_fwd, ray_project and ray_scatter; `paths` names what a row is there
to pin, tests/test_ray_sample_plan_cpu.py proves with the host mirror below that the row does reach it, shows that the contract
emulator stays inside the bound and that seeded kernel bugs miss it; tests/test_ray_sample_gpu.py runs every row on the GPU.

Storage discipline.  Every tensor is a view into a flat storage that is wider than the view.  Inputs hold NaN wherever their view
does not reach (a gather copies, a scatter adds: a NaN that is read shows).  Outputs start at a sentinel (forward, index tensor) or
at random contents (scatter); whatever the view does not address must come back bit-identical.

References.  Indices: the oracle's index arithmetic (O.ray_sample_indices, bit-defined), -1 = outside; voxels whose u or v is not
finite, or beyond the int32 range, are marked outside explicitly (what project() in the kernel file documents; a float -> int cast
of those is not defined on the host).  Gather: copies of the map's values at those indices, compared bit for bit.  Scatter:
index_add_ of the gradient in float64 on those indices, with n_p = the number of voxels that land on output element p and
A_p = the sum of their |g| (+ |previous content| when accumulating).

The scatter bound, per element:    |got - ref64| <= (n_p + 3) 2^-24 A_p + n_p 2^-43 max|dout|
The first term bounds any float32 summation order of n_p terms plus the final add and one conversion (each of at most n_p + 2
roundings is 2^-24 of a partial sum that is at most A_p, to first order; one more for the second order).  The second term is the
resolution the kernel's comments give its fixed-point addends: 2^-44 of 2^e, M < 2^e <= 2 M <= 2 max|dout|, in the LDS window;
1 / scale <= 2^(lg - 60) max|dout| with lg = ceil(log2(D H W)) <= 17 at these shapes in deterministic mode.  Nothing in it is
measured.  Integer-valued gradients make every sum exact on every path: bit equality.
For the record (no bar comes from these): the sequential float32 contract emulator reaches 0.42 of the bound (row s_slice_c10_acc);
on an MI355X the largest err / bound per path is 0.29 ... 0.38 (LDS window 0.35, 32-bit indices 0.37, runs outside the box 0.36,
deterministic CN = 12 / 4 0.35 / 0.36, 2^-100 gradients and non-finite gradients in deterministic mode 0.35 -- before the fix of
ray_det_scale_kernel the 2^-100 rows stood at 4e6 bounds and the non-finite rows lost their inf / NaN).
"""
from __future__ import annotations

import dataclasses
import math
import zlib
from typing import Tuple

import numpy as np
import torch as t

from oracle import corenet_oracle as O

SENTINEL = -1234.5
IDX_SENTINEL = 0x4D4D
TAIL = 8                       # elements behind the last sample of every storage
OUT_C0 = 2                     # the forward output is the channel slice [OUT_C0, OUT_C0 + C) of a buffer with one more channel behind


@dataclasses.dataclass(frozen=True)
class Case:
  name: str
  op: str                                    # fwd | scatter
  grid: Tuple[int, int, int]                 # D, H, W
  map: Tuple[int, int]                       # h, w
  C: int
  cams: Tuple[str, ...] = ("base", "shift", "roll")       # one per sample: B = len(cams)
  zoom: float = 1.0                          # x/y zoom of every camera about the image point zoom_at (u, v in [0, 1])
  zoom_at: Tuple[float, float] = (0.5, 0.5)
  layout: str = "cf"                         # map: cf = [B][C][h][w] | cl = [B][h][w][C] | cl_slice = channels [start, start + C) of
  cl_slice: Tuple[int, int] = (0, 0)         # a [B][h][w][width] buffer: (start, width)
  map_pad: int = 0                           # map_sB = the sample's extent + map_pad
  out_off: int = 0                           # elements the out / idx / dmap pointer is advanced beyond what the slice needs
  idx_off: int = 0
  dmap_off: int = 0
  out_sB_extra: int = 0                      # out_sB = (OUT_C0 + C + 1) D H W + out_sB_extra
  dout_slice: Tuple[int, int] = (0, 0)       # dout = channels [c0, c0 + C) of a buffer with `extra` more: (c0, extra)
  dmap_slice: Tuple[int, int] = (0, 0)       # dmap likewise: dmap_sB = (C + extra) h w
  deterministic: bool = False
  zero_first: bool = True
  grad: str = "randn"                        # randn | tiny (x 2^-100) | nonfinite | zero
  entry: str = "both"                        # scatter: idx + plain (both) | plain (maps of 65535 pixels and more)
  same_as: str = ""                          # fwd: the aligned row whose bits this one must reproduce
  paths: Tuple[str, ...] = ()

  @property
  def B(self): return len(self.cams)
  @property
  def S(self): return self.grid[0] * self.grid[1] * self.grid[2]
  @property
  def hw(self): return self.map[0] * self.map[1]
  @property
  def out_sB(self): return (OUT_C0 + self.C + 1) * self.S + self.out_sB_extra
  @property
  def out_ptr(self): return OUT_C0 * self.S + self.out_off
  @property
  def dout_sB(self): return (self.C + self.dout_slice[1]) * self.S
  @property
  def dout_ptr(self): return self.dout_slice[0] * self.S
  @property
  def dmap_sB(self): return (self.C + self.dmap_slice[1]) * self.hw
  @property
  def dmap_ptr(self): return self.dmap_slice[0] * self.hw + self.dmap_off
  @property
  def map_geom(self):
    """(pointer offset, map_sB, map_sC, map_sP) in elements."""
    h, w = self.map
    if self.layout == "cf": return 0, self.C * h * w + self.map_pad, h * w, 1
    start, width = (0, self.C) if self.layout == "cl" else self.cl_slice
    return start, h * w * width + self.map_pad, 1, width


# ------------------------------------------------------------------------------------------------ the table
G_ODD, M_ODD = (5, 9, 10), (7, 13)          # nothing a multiple of 4 but nothing
G_FLAT, M_FLAT = (3, 20, 28), (12, 20)      # D < 8, W % 4 == 0, 8 x 8 tiles cut by H and W
G_WIDE, M_WIDE = (3, 68, 72), (40, 24)      # 32 x 8 tiles cut by H and W
CUT = ("cut", "cut_roll")
NONCUBIC = ("noncubic_grid", "nonsquare_map")


def _f(name, grid, map_, C, **kw):
  return Case(name, "fwd", grid, map_, C, **kw)


def _s(name, grid, map_, C, paths=(), det_paths=(), modes=(False, True), **kw):
  """One scatter row per (mode, zero_first)."""
  rows = []
  for det in modes:
    for zf in (True, False):
      rows.append(Case(name + ("_det" if det else "") + ("" if zf else "_acc"), "scatter", grid, map_, C, deterministic=det,
                       zero_first=zf, paths=tuple(det_paths if det else paths), **kw))
  return rows


ALIGNED = "f_flat_c12_cl"
CASES = [
    # ---- forward / index tensor / projection
    _f("f_odd_c28_cf", G_ODD, M_ODD, 28, paths=("fwd<1,false>", "project<1>", "idx_store<1>", "two_groups_full_then_leftover") + NONCUBIC),
    _f("f_odd_c28_cl", G_ODD, M_ODD, 28, layout="cl", paths=("fwd<1,true>", "two_groups_full_then_leftover") + NONCUBIC),
    _f("f_flat_c16_cl", G_FLAT, M_FLAT, 16, layout="cl", paths=("fwd<4,true>", "one_group_full_then_leftover") + NONCUBIC),
    _f("f_flat_c20_cl", G_FLAT, M_FLAT, 20, layout="cl", paths=("fwd<4,true>", "one_group_full_then_leftover")),
    _f("f_flat_c10_cf", G_FLAT, M_FLAT, 10, paths=("fwd<4,false>", "leftover_only") + NONCUBIC),
    _f(ALIGNED, G_FLAT, M_FLAT, 12, layout="cl", paths=("fwd<4,true>",)),
    _f("f_flat_out1", G_FLAT, M_FLAT, 12, layout="cl", out_off=1, same_as=ALIGNED, paths=("fwd<1,true>", "v4_fail_out_ptr")),
    _f("f_flat_outsB", G_FLAT, M_FLAT, 12, layout="cl", out_sB_extra=1, same_as=ALIGNED, paths=("fwd<1,true>", "v4_fail_out_sB")),
    _f("f_flat_idx1", G_FLAT, M_FLAT, 12, layout="cl", idx_off=1, same_as=ALIGNED, paths=("fwd<1,true>", "v4_fail_idx_ptr", "idx_store<1>")),
    _f("f_flat_sl2", G_FLAT, M_FLAT, 12, layout="cl_slice", cl_slice=(2, 16), same_as=ALIGNED, paths=("fwd<4,false>", "cl_fail_ptr")),
    _f("f_flat_sl4", G_FLAT, M_FLAT, 12, layout="cl_slice", cl_slice=(4, 16), same_as=ALIGNED, paths=("fwd<4,true>", "cl_slice_aligned")),
    _f("f_flat_w14", G_FLAT, M_FLAT, 12, layout="cl_slice", cl_slice=(0, 14), same_as=ALIGNED, paths=("fwd<4,false>", "cl_fail_sP")),
    _f("f_flat_sB2", G_FLAT, M_FLAT, 12, layout="cl", map_pad=2, same_as=ALIGNED, paths=("fwd<4,false>", "cl_fail_sB")),
    _f("f_flat_sB8", G_FLAT, M_FLAT, 12, layout="cl", map_pad=8, same_as=ALIGNED, paths=("fwd<4,true>",)),
    _f("f_cut_c12", (16, 16, 16), (16, 16), 12, layout="cl", cams=CUT, paths=("pw_sign_change",)),
    _f("f_pw0_c12", (16, 16, 16), (16, 16), 12, layout="cl", cams=("pw0", "pw0_roll"), paths=("pw_zero_plane",)),
    # ---- scatter: every row in default and deterministic mode, zeroing first and accumulating
    *[r for C in (1, 2, 10, 12) for r in _s(
        f"s_flat_c{C}", G_FLAT, M_FLAT, C,
        paths=("D<8", "tile8x8_partial", "window", "channel_clamp" if C % 4 else "full_groups") + NONCUBIC,
        det_paths=("D<8", "tile8x8_partial", "det_CN12" if C == 12 else "det_CN4", "det_maxabs_scale_finish") + NONCUBIC)],
    *[r for C in (4, 24) for r in _s(
        f"s_wide_c{C}", G_WIDE, M_WIDE, C, paths=("tile32x8_partial", "window", "D<8") + NONCUBIC,
        det_paths=("tile32x8_partial", "det_CN12" if C == 24 else "det_CN4") + NONCUBIC)],
    *_s("s_i32", (2, 128, 128), (256, 256), 4, entry="plain", paths=("i32_window", "i32_box_too_large", "project<4,i32>"),
        det_paths=("i32_det",)),
    *_s("s_zoom", (8, 16, 16), (64, 64), 4, zoom=2.0, zoom_at=(0.25, 0.25), paths=("u16_box_too_large",), det_paths=("det_CN4",)),
    *_s("s_cut", (16, 16, 16), (16, 16), 4, cams=CUT, paths=("run_outside_box", "pw_sign_change"), det_paths=("det_CN4", "pw_sign_change")),
    *[r for C in (10, 12) for r in _s(
        f"s_slice_c{C}", G_FLAT, M_FLAT, C, dmap_slice=(1, 3), dout_slice=(2, 3), paths=("memset_per_sample", "dout_slice"),
        det_paths=("memset_per_sample", "dout_slice", "det_finish_strided"))],
    *_s("s_w1", (8, 8, 8), (8, 1), 96, modes=(True,), det_paths=("width_one_reshape", "det_CN12")),
    *_s("s_tiny", G_FLAT, M_FLAT, 12, grad="tiny", modes=(True,), det_paths=("det_tiny_scale",)),
    *_s("s_nonfinite", G_FLAT, M_FLAT, 12, grad="nonfinite", modes=(True,), det_paths=("det_nonfinite",)),
    *_s("s_zero", G_FLAT, M_FLAT, 12, grad="zero", modes=(True,), det_paths=("det_zero",)),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# what the issue's list of never-executed branches comes to, path by path: every one is named by at least one row
REQUIRED_PATHS = (
    "fwd<1,false>", "fwd<1,true>", "project<1>", "idx_store<1>", "two_groups_full_then_leftover", "one_group_full_then_leftover",
    "cl_fail_sP", "cl_fail_sB", "cl_fail_ptr", "cl_slice_aligned", "v4_fail_out_ptr", "v4_fail_out_sB", "v4_fail_idx_ptr",
    "noncubic_grid", "nonsquare_map", "tile32x8_partial", "tile8x8_partial", "D<8", "i32_window", "i32_box_too_large",
    "u16_box_too_large", "run_outside_box", "pw_sign_change", "pw_zero_plane", "memset_per_sample", "dout_slice", "det_CN12", "det_CN4",
    "det_maxabs_scale_finish", "det_finish_strided", "det_tiny_scale", "det_nonfinite", "det_zero", "width_one_reshape", "channel_clamp")


# ------------------------------------------------------------------------------------------------ cameras
def _seed(*key):
  return zlib.crc32(repr(key).encode())


def camera(kind, grid, zoom=1.0, zoom_at=(0.5, 0.5)):
  """(matrix [4, 4], offset [3]) of one sample.  base: the canonical camera on the unit cube, per axis for a non-cubic grid."""
  D, H, W = grid
  base = O.canonical_camera() @ O.scale([1.0 / 128] * 3) @ O.scale([128.0 / W, 128.0 / H, 128.0 / D])
  a = math.radians(20.0)
  roll = t.tensor([[math.cos(a), -math.sin(a), 0, 0], [math.sin(a), math.cos(a), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=t.float32)
  off = t.tensor([0.5, 0.5, 0.5])
  if kind == "base":
    m = base
  elif kind == "shift":                       # part of the grid leaves the image, a slab is behind the camera
    m, off = O.translate([0.9, -0.4, -0.95]) @ base, t.tensor([0.25, 0.5, 0.75])
  elif kind == "roll":                        # a general matrix
    m = roll @ base
  elif kind in ("cut", "cut_roll"):
    # the camera plane (pw = 0) lies inside the grid and nothing is culled (row 2 = [0 0 0 1], pz = 1): pw changes sign inside
    # tiles, the extremes of a tile's pixels are no longer at its corners
    m = O.canonical_camera() @ O.translate([0.1, 0.05, -1.1]) @ O.scale([1.0 / W, 1.0 / H, 1.0 / D])
    if kind == "cut_roll": m = roll @ m
    m = m.clone()
    m[2] = t.tensor([0.0, 0.0, 0.0, 1.0])
  elif kind in ("pw0", "pw0_roll"):
    # pw = cz - (k + 0.5) is exactly 0 on the voxel plane z = k: px / pw is +-inf there, NaN where px is 0 too
    m = (base if kind == "pw0" else roll @ base).clone()
    m[2] = t.tensor([0.0, 0.0, 0.0, 1.0])
    m[3] = t.tensor([0.0, 0.0, 1.0, -(D // 4 + 0.5)])
    if kind == "pw0":                                           # px = x: 0 on the plane x = 0 -> 0 / 0 = NaN on one voxel row
      m[0], off = t.tensor([1.0, 0.0, 0.0, 0.0]), t.tensor([0.0, 0.5, 0.5])
  else:
    raise ValueError(kind)
  if zoom != 1.0:
    au, av = 2 * zoom_at[0] - 1, 2 * zoom_at[1] - 1           # px' = zoom (px - au pw): the image point zoom_at goes to the centre
    z = t.tensor([[zoom, 0, 0, -zoom * au], [0, zoom, 0, -zoom * av], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=t.float32)
    m = z @ m
  return m.contiguous(), off


def cameras(c: Case):
  ms, offs = zip(*[camera(k, c.grid, c.zoom, c.zoom_at) for k in c.cams])
  return t.stack(ms), t.stack(offs)


# ------------------------------------------------------------------------------------------------ reference indices
def project(m, off, x, y, z, wh, swap_hw=False):
  """The flat pixel index of voxels (x, y, z) (int64 tensors of one shape) for ONE camera, -1 outside: the oracle's arithmetic
  (O.ray_sample_indices: fp32, this evaluation order) at arbitrary voxels, also returns pw.  swap_hw: the seeded bug iy * h + ix."""
  w, h = wh
  cx, cy, cz = x.float() + off[0], y.float() + off[1], z.float() + off[2]
  row = lambda n: ((m[n, 0] * cx + m[n, 1] * cy) + m[n, 2] * cz) + m[n, 3]
  px, py, pz, pw = row(0), row(1), row(2), row(3)
  with np.errstate(all="ignore"):
    fu = ((px / pw) / 2 + 0.5) * float(w)
    fv = ((py / pw) / 2 + 0.5) * float(h)
  ok = t.isfinite(fu) & t.isfinite(fv) & (fu.abs() < 2147483520.0) & (fv.abs() < 2147483520.0)
  ix = t.where(ok, fu, t.zeros_like(fu)).to(t.int64)          # (trunc toward zero, like the C cast)
  iy = t.where(ok, fv, t.zeros_like(fv)).to(t.int64)
  ok &= (pz >= 0) & (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)
  return t.where(ok, iy * (h if swap_hw else w) + ix, t.full_like(ix, -1)), pw


def ref_indices(c: Case):
  """int64 [B][D][H][W], -1 outside: O.ray_sample_indices, with the voxels whose u / v cast is undefined marked outside."""
  m, off = cameras(c)
  h, w = c.map
  with np.errstate(all="ignore"):
    iy, ix, keep = O.ray_sample_indices(m, off, c.grid, (w, h))
  inside = keep & (iy >= 1) & (iy <= h) & (ix >= 1) & (ix <= w)
  po = t.where(inside, (iy - 1) * w + (ix - 1), t.full_like(iy, -1))
  D, H, W = c.grid
  zz, yy, xx = t.meshgrid(t.arange(D), t.arange(H), t.arange(W), indexing="ij")
  mine = t.stack([project(m[b], off[b], xx, yy, zz, (w, h))[0] for b in range(c.B)])
  hostile = (mine < 0) & (po >= 0)            # only ever the voxels whose cast is undefined (tests/test_ray_sample_plan_cpu.py)
  return t.where(hostile, t.full_like(po, -1), po), mine


def pw_of(c: Case):
  m, off = cameras(c)
  D, H, W = c.grid
  zz, yy, xx = t.meshgrid(t.arange(D), t.arange(H), t.arange(W), indexing="ij")
  return t.stack([project(m[b], off[b], xx, yy, zz, (c.map[1], c.map[0]))[1] for b in range(c.B)])


# ------------------------------------------------------------------------------------------------ host mirror
def fwd_path(c: Case, with_idx=True):
  """(VX, CL, gridDim.z, the last group runs a full 12 and then leftovers) as ray_fwd decides them.  Allocations are aligned to
  256 bytes and more, so a pointer's alignment is that of its element offset."""
  W = c.grid[2]
  v4 = W % 4 == 0 and c.out_sB % 4 == 0 and (c.out_ptr * 4) % 16 == 0 and (not with_idx or (c.idx_off * 2) % 8 == 0)
  ptr, sB, sC, sP = c.map_geom
  cl = sC == 1 and sP % 4 == 0 and sB % 4 == 0 and c.C % 4 == 0 and (ptr * 4) % 16 == 0
  gz = max(1, c.C // 12)
  return (4 if v4 else 1), cl, gz, (c.C >= 12 and c.C % 12 != 0)


def project_path(c: Case):
  return (4 if c.grid[2] % 4 == 0 else 1), ("u16" if c.hw < 65535 else "i32")


def scatter_plan(c: Case):
  D, H, W = c.grid
  h, w = c.map
  reshaped = w == 1 and h > 1
  if reshaped: w, h = h, 1
  det = c.deterministic
  CN = 12 if (c.C % 12 == 0 and det) else 4
  zseg = min(D, 8)
  big = W >= 64 and H >= 64
  kTX = 32 if big else 8
  kTY = 256 // kTX if big else 8
  sx, sy = max(1.0, w / W), max(1.0, h / H)
  wpix = int(kTX * sx + 4) * int(kTY * sy + 4)
  win = 0 if det else min(wpix * CN, 6 * 1024)
  return dict(CN=CN, zseg=zseg, nseg=-(-D // zseg), kTX=kTX, kTY=kTY, tilesX=-(-W // kTX), tilesY=-(-H // kTY), win_floats=win,
              IT="u16" if c.hw < 65535 else "i32", reshaped=reshaped, h=h, w=w, memset_per_sample=c.dmap_sB != c.C * c.hw)


def workgroups(c: Case, idx=None):
  """Every workgroup of the scatter (one per sample, tile and z segment; the channel groups share it) classified from the
  reference indices the way the kernel does from its 8 corner loads: a list of dicts with the box (x0, width, y0, height; width 0 =
  no window), kind = window | no_corner | too_large, partial = the tile is cut by the grid, outside_runs = a voxel of a window
  workgroup lands outside its box, both_signs = in-image voxels with pw > 0 and with pw < 0."""
  p = scatter_plan(c)
  D, H, W = c.grid
  w = p["w"]
  idx = ref_indices(c)[0] if idx is None else idx
  pw = pw_of(c)
  out = []
  for b in range(c.B):
    for s in range(p["nseg"]):
      z0, z1 = s * p["zseg"], min(D, (s + 1) * p["zseg"])
      for ty in range(p["tilesY"]):
        for tx in range(p["tilesX"]):
          x0, y0 = tx * p["kTX"], ty * p["kTY"]
          x1, y1 = min(W, x0 + p["kTX"]), min(H, y0 + p["kTY"])
          cor = idx[b][[z0, z1 - 1]][:, [y0, y1 - 1]][:, :, [x0, x1 - 1]].reshape(-1)
          cor = cor[cor >= 0]
          vox = idx[b, z0:z1, y0:y1, x0:x1]
          inimg = vox >= 0
          rec = dict(b=b, z=(z0, z1), y=(y0, y1), x=(x0, x1), partial=x0 + p["kTX"] > W or y0 + p["kTY"] > H, box=(0, 0, 0, 0),
                     outside_runs=False, both_signs=bool(((pw[b, z0:z1, y0:y1, x0:x1] > 0) & inimg).any() and
                                                         ((pw[b, z0:z1, y0:y1, x0:x1] < 0) & inimg).any()))
          if p["win_floats"] == 0:
            rec["kind"] = "deterministic"
          elif cor.numel() == 0:
            rec["kind"] = "no_corner"
          else:
            iy, ix = cor // w, cor % w
            ix0, ix1 = max(0, int(ix.min()) - 1), min(w - 1, int(ix.max()) + 1)
            iy0, iy1 = max(0, int(iy.min()) - 1), min(p["h"] - 1, int(iy.max()) + 1)
            if (ix1 - ix0 + 1) * (iy1 - iy0 + 1) * p["CN"] > p["win_floats"]:
              rec["kind"] = "too_large"
            else:
              rec["kind"], rec["box"] = "window", (ix0, ix1 - ix0 + 1, iy0, iy1 - iy0 + 1)
              vy, vx = vox // w, vox % w
              rec["outside_runs"] = bool((inimg & ((vx < ix0) | (vx > ix1) | (vy < iy0) | (vy > iy1))).any())
          out.append(rec)
  return out


# ------------------------------------------------------------------------------------------------ tensors of a row
class Built:
  pass


def build(c: Case, grad=None):
  """Seeded storages of a row.  The seed depends on the shapes only: rows that differ in layout hold the same logical tensors."""
  b = Built()
  b.case = c
  D, H, W = c.grid
  h, w = c.map
  B, C, S = c.B, c.C, c.S
  g = t.Generator().manual_seed(_seed(c.grid, c.map, C, B))
  b.m, b.off = cameras(c)
  if c.op == "fwd":
    b.map = t.randn(B, C, h, w, generator=g)
    ptr, sB, sC, sP = c.map_geom
    b.map_st = t.full((ptr + B * sB + TAIL,), float("nan"))
    t.as_strided(b.map_st, (B, C, h, w), (sB, sC, w * sP, sP), ptr).copy_(b.map)
    b.out_st = t.full((c.out_ptr + B * c.out_sB + TAIL,), SENTINEL)
    b.idx_st = t.full((c.idx_off + B * S + TAIL,), IDX_SENTINEL, dtype=t.int16)
    return b
  kind = grad or c.grad
  b.grad_kind = kind
  if kind == "int":
    gy = t.randint(-8, 9, (B, C, D, H, W), generator=g).float()
    prev = t.randint(-8, 9, (c.dmap_ptr + B * c.dmap_sB + TAIL,), generator=g).float()
  else:
    gy = t.randn(B, C, D, H, W, generator=g)
    prev = t.randn(c.dmap_ptr + B * c.dmap_sB + TAIL, generator=g)
  if kind == "tiny":
    gy, prev = gy * 2.0 ** -100, prev * 2.0 ** -100
  elif kind == "zero":
    gy = t.zeros_like(gy)
  elif kind == "nonfinite":
    # one +inf, one -inf and one NaN in different tiles, and a pixel that receives +inf and -inf (neighbours in z)
    gy[0, 1, 1, 3, 5] = float("inf"); gy[0, 2, D - 1, H - 2, W - 3] = float("-inf"); gy[1, 0, D // 2, 9, 11] = float("nan")
    gy[B - 1, 3, 0, 10, 14] = float("inf"); gy[B - 1, 3, 1, 10, 14] = float("-inf")
  b.gy, b.dmap0 = gy, prev
  b.dout_st = t.full((c.dout_ptr + B * c.dout_sB + TAIL,), float("nan"))
  t.as_strided(b.dout_st, (B, C, S), (c.dout_sB, S, 1), c.dout_ptr).copy_(gy.reshape(B, C, S))
  return b


def scaled(b, e):
  """The row's tensors times 2^e (exact)."""
  s = Built()
  s.__dict__.update(b.__dict__)
  f = 2.0 ** e
  s.gy, s.dmap0, s.dout_st = b.gy * f, b.dmap0 * f, b.dout_st * f
  return s


def out_view(c, st): return t.as_strided(st, (c.B, c.C) + c.grid, (c.out_sB, c.S, c.grid[1] * c.grid[2], c.grid[2], 1), c.out_ptr)
def idx_view(c, st): return t.as_strided(st, (c.B,) + c.grid, (c.S, c.grid[1] * c.grid[2], c.grid[2], 1), c.idx_off)
def dmap_view(c, st): return t.as_strided(st, (c.B, c.C) + c.map, (c.dmap_sB, c.hw, c.map[1], 1), c.dmap_ptr)


# ------------------------------------------------------------------------------------------------ references
def ref_gather(c, b, idx):
  """[B][C][D][H][W]: the map's values at the reference indices, 0 outside."""
  flat = b.map.reshape(c.B, c.C, c.hw)
  got = t.gather(flat, 2, idx.clamp(min=0).reshape(c.B, 1, c.S).expand(c.B, c.C, c.S)).view(c.B, c.C, *c.grid)
  return t.where((idx >= 0)[:, None], got, t.zeros_like(got))


def want_fwd(c, b, idx):
  """The storages a forward call must leave: (out, idx as uint16 values in int16 storage)."""
  out, ist = b.out_st.clone(), b.idx_st.clone()
  out_view(c, out).copy_(ref_gather(c, b, idx))
  idx_view(c, ist).copy_(t.where(idx >= 0, idx, t.full_like(idx, 0xFFFF)).to(t.int32).to(t.int16))
  return out, ist


class ScatterRef:
  """float64 index_add_ on the reference indices, with what the bound needs."""

  def __init__(self, c, b, idx):
    B, C, hw = c.B, c.C, c.hw
    keep = idx >= 0
    lin = (t.arange(B)[:, None, None, None] * (hw + 1) + t.where(keep, idx, t.full_like(idx, hw))).reshape(-1)
    g = b.gy.double().permute(0, 2, 3, 4, 1).reshape(-1, C)
    fin = t.isfinite(g)
    acc = lambda v: t.zeros(B * (hw + 1), v.shape[1], dtype=t.float64).index_add_(0, lin, v).view(B, hw + 1, -1)[:, :hw].permute(0, 2, 1)
    with np.errstate(all="ignore"):
      s = acc(g).reshape(B, C, *c.map)
      self.A = acc(t.where(fin, g.abs(), t.zeros_like(g))).reshape(B, C, *c.map)
    self.n = acc(t.ones(g.shape[0], 1, dtype=t.float64)).reshape(B, 1, *c.map)
    prev = dmap_view(c, b.dmap0).double()
    if c.zero_first:
      self.ref = s
    else:
      self.ref, self.A = s + prev, self.A + prev.abs()
    self.gmax = float(b.gy[t.isfinite(b.gy)].abs().max()) if bool(t.isfinite(b.gy).any()) else 0.0
    self.bound = (self.n + 3) * 2.0 ** -24 * self.A + self.n * 2.0 ** -43 * self.gmax

  def check(self, c, b, st):
    """(largest err / bound over the finite elements (0 / 0 = 0), non-finite positions and kinds equal, the rest bit-identical)."""
    got = dmap_view(c, st).double()
    ref = self.ref
    kinds = bool(t.equal(t.isnan(got), t.isnan(ref)) and t.equal(t.isposinf(got), t.isposinf(ref)) and t.equal(t.isneginf(got), t.isneginf(ref)))
    f = t.isfinite(ref) & t.isfinite(got)
    err, bound = (got - ref).abs()[f], self.bound.expand_as(ref)[f]
    ratio = t.where(err == 0, t.zeros_like(err), err / bound)
    a, z = st.clone(), b.dmap0.clone()
    dmap_view(c, a).zero_(); dmap_view(c, z).zero_()
    return (float(ratio.max()) if ratio.numel() else 0.0), kinds, bool(t.equal(a.view(t.int32), z.view(t.int32)))

  def exact(self, c, st):
    return bool(t.equal(dmap_view(c, st), self.ref.float()))


# ------------------------------------------------------------------------------------------------ GPU drivers
def run_fwd(be, c, b, dev, with_idx):
  """(out storage, idx storage) after crn_ray_sample_fwd_idx / crn_ray_sample_fwd, on the CPU."""
  ptr, sB, sC, sP = c.map_geom
  mp, out, ist = b.map_st.to(dev), b.out_st.to(dev), b.idx_st.to(dev)
  md, od = b.m.reshape(c.B, 16).to(dev), b.off.to(dev)
  args = (mp[ptr:], sB, c.B, c.C, c.map[0], c.map[1], md, od, out[c.out_ptr:], c.out_sB) + c.grid
  if with_idx: be.ray_sample_fwd_idx(*args, ist[c.idx_off:], map_sC=sC, map_sP=sP)
  else: be.ray_sample_fwd(*args, map_sC=sC, map_sP=sP)
  return out.cpu(), ist.cpu()


def run_project(be, c, b, dev):
  ist = b.idx_st.to(dev)
  be.ray_project(b.m.reshape(c.B, 16).to(dev), b.off.to(dev), c.B, *c.grid, c.map[0], c.map[1], ist[c.idx_off:])
  return ist.cpu()


def run_scatter(be, c, b, dev, entry, idx=None):
  """The dmap storage after crn_ray_sample_bwd_idx (entry "idx": on the reference indices) / crn_ray_sample_bwd ("plain")."""
  dout, dmap = b.dout_st.to(dev), b.dmap0.to(dev)
  if entry == "idx":
    i16 = t.where(idx >= 0, idx, t.full_like(idx, 0xFFFF)).to(t.int32).to(t.int16).contiguous().to(dev)
    be.ray_sample_bwd_idx(dout[c.dout_ptr:], c.dout_sB, c.B, c.C, *c.grid, i16, dmap[c.dmap_ptr:], c.dmap_sB, c.map[0], c.map[1], c.zero_first)
  else:
    be.ray_sample_bwd(dout[c.dout_ptr:], c.dout_sB, c.B, c.C, *c.grid, b.m.reshape(c.B, 16).to(dev), b.off.to(dev),
                      dmap[c.dmap_ptr:], c.dmap_sB, c.map[0], c.map[1], c.zero_first)
  return dmap.cpu()


# ------------------------------------------------------------------------------------------------ kernels in Python, with seeded bugs
def emu_fwd(c, b, bug=None):
  """ray_sample_fwd_kernel thread by thread (vectorised): the decomposition of the thread index, the projection of the voxels the
  thread decodes, the stores at the address it computes, group by group.  bug: swap_hw (iy * h + ix) | swap_HD (r % D, r / D in
  the decomposition) | drop_leftover (the c < cend loop missing)."""
  D, H, W = c.grid
  h, w = c.map
  VX, _, gz, _ = fwd_path(c)
  out, ist = b.out_st.clone(), b.idx_st.clone()
  wx = W // VX
  r = t.arange(D * H * wx)
  x0, r = (r % wx) * VX, r // wx
  y, z = (r % D, r // D) if bug == "swap_HD" else (r % H, r // H)
  flat = b.map.reshape(c.B, c.C, c.hw)
  for bb in range(c.B):
    for k in range(VX):
      po, _ = project(b.m[bb], b.off[bb], x0 + k, y, z, (w, h), swap_hw=bug == "swap_hw")
      po = t.where(po < c.hw, po, t.full_like(po, -1))          # (an index past the map would fault: the emulation drops it)
      loc = (z * H + y) * W + x0 + k
      ok = loc < c.S
      ist[c.idx_off + bb * c.S + loc[ok]] = t.where(po >= 0, po, t.full_like(po, 0xFFFF)).to(t.int32).to(t.int16)[ok]
      for grp in range(gz):
        cc = grp * 12
        cend = c.C if grp + 1 == gz else cc + 12
        chans = list(range(cc, cc + (cend - cc) // 12 * 12)) + ([] if bug == "drop_leftover" else list(range(cc + (cend - cc) // 12 * 12, cend)))
        for ch in chans:
          v = t.where(po >= 0, flat[bb, ch][po.clamp(min=0)], t.zeros(()))
          out[c.out_ptr + bb * c.out_sB + ch * c.S + loc[ok]] = v[ok]
  return out, ist


def emu_scatter(c, b, idx, bug=None):
  """What ray_scatter adds where, in float64 (the order of its sums is the bound's business): the zeroing, the workgroups' boxes,
  the channel groups with their clamp.  bug: drop_outside (a run outside a box that is in use is lost) | zero_stride (the zeroing
  walks C h w per sample) | no_clamp (channel slot k of the last group is added although cbase + k >= C: it lands in the next
  channel, with the gradient the clamped load fetched)."""
  p = scatter_plan(c)
  B, C, hw = c.B, c.C, c.hw
  st = b.dmap0.double().clone()
  if c.zero_first:
    for bb in range(B):
      o = c.dmap_ptr + bb * (C * hw if bug == "zero_stride" else c.dmap_sB)
      st[o:o + C * hw] = 0
  use = idx >= 0
  if bug == "drop_outside":
    use = use.clone()
    for wg in workgroups(c, idx):
      if wg["kind"] != "window": continue
      bx0, bw, by0, bh = wg["box"]
      (z0, z1), (y0, y1), (x0, x1) = wg["z"], wg["y"], wg["x"]
      v = idx[wg["b"], z0:z1, y0:y1, x0:x1]
      vy, vx = v // p["w"], v % p["w"]
      use[wg["b"], z0:z1, y0:y1, x0:x1] &= (vx >= bx0) & (vx < bx0 + bw) & (vy >= by0) & (vy < by0 + bh)
  groups = -(-C // p["CN"])
  for bb in range(B):
    sel = use[bb].reshape(-1)
    po = idx[bb].reshape(-1)[sel]
    for ch in range(groups * p["CN"] if bug == "no_clamp" else C):
      src = ch if ch < C else ch // p["CN"] * p["CN"]
      o = c.dmap_ptr + bb * c.dmap_sB + ch * hw
      if o + hw > st.numel(): continue
      st[o:o + hw].index_add_(0, po, b.gy[bb, src].double().reshape(-1)[sel])
  return st.float()                 # (one rounding of the exact sum: inside the bound's first term)
