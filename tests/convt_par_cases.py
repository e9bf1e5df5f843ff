"""The case table of the parity-walk kernels of decoder stage_6.t1 (csrc/convt_par.hip: ConvTranspose3d 16 -> cout, k 7, stride 2,
padding 3, output_padding 1) and what its tests share.  TEST INFRASTRUCTURE ONLY.

One row = one call of crn_convt_s2k7_{fwd,dgrad,c2_fwd,c2_dgrad,wgrad}_bf3 or crn_convt_s2k7_ximage on seeded tensors.  The
transform kinds, the sentinel and the error measures are those of tests/conv_fp32_cases.py.  tests/test_convt_par_model_cpu.py
proves on the CPU what the table reaches, checks the four weight-image tables of conv_geometry against the walk model below and
shows which kernel bugs the bars catch; tests/test_convt_par_gpu.py runs every row on the GPU.

Storage discipline.  Every tensor is a view into a flat storage that is wider than the view (channels in front of / behind a
channel slice, slack between channels and between samples, 8 elements behind the last sample).  Output storages start at SENTINEL,
or at random contents for accumulating rows; input storages hold NaN wherever the view does not reach: the channels of dy at and
beyond cout, the slack between the samples of x.  A row passes only if no NaN appears in the output and every element outside the
output view comes back bit-identical.

References.  (1) float64: torch's conv_transpose3d on T(x) as doubles, its adjoint (a stride-2 conv3d), autograd for the weight
gradient (the engine's packed output is brought back through conv_geometry.convt_fwd(...).index).  (2) The walk model: it reads a
weight IMAGE the way the header comments of convt_par.hip say the kernels do -- plain loops over parity and window, k = 5 - 2 z + r
forward, k = 2 z - 1 + r for the data gradient; it never sees the table that built the image --, splits T(x) / dy into bf16 hi and
lo and sums the exact products hi*hi + hi*lo + lo*hi in float64.  From the walk model only the order of the float32 sums separates
a kernel.

Bars.  Against float64: BAR = 2e-5 of max|reference|, the project's bar for this layer; the operand split alone (walk model against
float64) takes 2.3e-6 .. 7.7e-6 of it on the rows here (largest: row rf_261).  Against the walk model: SPLIT_BAR = 4 x SPLIT_MAX_F32,
SPLIT_MAX_F32 = 2.61e-6 = the largest difference over the rows of this table between the walk model summed in float32 in torch's
order and in float64 (row g_t57_c9_fused).  Both numbers come from references alone (tests/test_convt_par_model_cpu.py measures them).
Measured on an MI355X, largest error per kernel family, of max|reference| (against float64 / against the walk model):
  walk forward        5.5e-6 / 8.5e-7      weight gradient, 36-tap pair,  T(x) image made ahead   6.9e-6 / 3.6e-7     fused   5.8e-6 / 5.1e-7
  walk data gradient  5.2e-6 / 1.6e-6      weight gradient, 48-tap pairs, T(x) image made ahead   6.9e-6 / 5.5e-7     fused   5.8e-6 / 3.3e-7
  resident forward    7.6e-6 / 7.3e-7      weight gradient, 64-tap pair,  T(x) image made ahead   6.9e-6 / 3.4e-7     fused   5.8e-6 / 2.5e-7
  resident data grad. 5.4e-6 / 8.7e-7      deterministic mode (the generic engine takes the call) 4.1e-6 / 6.0e-7
(the float64 figure of a weight-gradient row is that of the whole un-packed gradient, the walk-model figure is per pair class).
Every family is inside SPLIT_BAR, the weight gradient with its atomics over up to 144 workgroups included.
"""
from __future__ import annotations

import dataclasses
import zlib
from typing import Tuple

import numpy as np
import torch as t
import torch.nn.functional as F

from conv_fp32_cases import SENTINEL, transform_of, err_inside        # noqa: F401 (shared)
from kernel_contract_emu import EmuBackend, logical, write_logical
from corenet_amd import views as V
from corenet_amd.model import conv_geometry as G

BAR = 2e-5                  # of max|float64 reference|: the project's bar for this layer (tests/test_kernels_gpu.py)
SPLIT_MAX_F32 = 2.61e-6     # the largest difference, over all rows, between the walk model summed in float32 (torch's order) and in
                            # float64, of max|reference| (tests/test_convt_par_model_cpu.py measures it: row g_t57_c9_fused, whose
                            # sums run over 14592 positions)
SPLIT_BAR = 4 * SPLIT_MAX_F32       # the rule and the margin of tests/conv_bf3_cases.py
WOFS = 37                   # the weight sits inside a larger parameter slab
TERMS = (("h", "h"), ("h", "l"), ("l", "h"))       # (input term, weight term) of the three products
_EMU = EmuBackend()


@dataclasses.dataclass(frozen=True)
class Case:
  name: str
  op: str                            # fwd | dgrad | wgrad | ximage
  resident: bool = False             # the two-class kernels with resident weights (convt_res_kernel)
  cout: int = 2
  B: int = 1
  dims: Tuple[int, int, int] = (4, 8, 16)          # the coarse grid (x / dx); y / dy have twice the extents
  tr: str = "none"                   # none | scale | shift | pre | post | both
  bias: bool = True                  # fwd
  accumulate: bool = False           # dgrad: accumulate; wgrad: zero_first = not accumulate
  x_slack: int = 0                   # x_sB (dgrad: dx_sB) = 16 D H W + x_slack
  c_slack: int = 0                   # y_sC / dy_sC = 8 D H W + c_slack
  c0: int = 0                        # y / dy is the channel slice [c0, c0 + cout) of a wider buffer ...
  c_extra: int = 3                   # ... with c_extra channels behind it
  npad: int = 0                      # wgrad: Npad (0: 8 cout)
  ximg: str = ""                     # wgrad: ahead (crn_convt_s2k7_ximage made the operand image) | fused (null image)
  deterministic: bool = False        # wgrad: the entry steps aside, conv_wgrad(math="ct_par") lands on the generic engine
  expect: dict = dataclasses.field(default_factory=dict)     # what the host loops make of the row (resident: tiles, per, wgs;
                                                             # wgrad: ntiles, tiles_per_wg, wg_end): mirrored in Python and
                                                             # recomputed by tests/test_convt_par_model_cpu.py

  @property
  def Npad(self):
    return self.npad or 8 * self.cout


def _c(name, op, **kw):
  return Case(name, op, **kw)


def _both_stagings(name, **kw):
  return [_c(f"{name}_{s}", "wgrad", ximg=s, **kw) for s in ("ahead", "fused")]


# ------------------------------------------------------------------------------------------------ the table
# Tiles are 4 x 8 x 16 positions of the coarse grid (weight gradient: 2 x 8 x 16).  (4, 8, 16) = one tile, every halo is padding;
# (8, 16, 32) = two tiles per dimension; (12, 8, 16), (4, 24, 16), (4, 8, 48) = an interior tile in D, H, W in turn.
CASES = [
    # ---- generic forward (convt_par_fwd_kernel): one workgroup per tile
    _c("f_c1_one", "fwd", cout=1, tr="shift"),                                              # (a non-zero shift: padding must stay zero)
    _c("f_c8_two", "fwd", cout=8, dims=(8, 16, 32), tr="pre", c0=2),
    _c("f_c9_d", "fwd", cout=9, B=3, dims=(12, 8, 16), tr="both", c_slack=8),               # 9 tiles
    _c("f_c14_h", "fwd", cout=14, dims=(4, 24, 16), tr="post", bias=False, x_slack=12),     # 3 tiles
    _c("f_c16_w", "fwd", cout=16, dims=(4, 8, 48), tr="scale"),                             # 3 tiles
    _c("f_c2_b3", "fwd", cout=2, B=3, dims=(8, 8, 16), x_slack=4, c0=2, c_slack=4),         # 6 tiles, no transform
    # ---- generic data gradient (convt_par_dgrad_kernel): one or two 8-channel halves of n, full and partial
    _c("d_c1_one", "dgrad", cout=1),                                                        # dy_sC exactly 8 D H W
    _c("d_c8_two", "dgrad", cout=8, dims=(8, 16, 32), accumulate=True, c_slack=8, c0=2),
    _c("d_c9_d", "dgrad", cout=9, B=3, dims=(12, 8, 16), x_slack=12),                       # dy_sC exactly 8 D H W
    _c("d_c16_h", "dgrad", cout=16, dims=(4, 24, 16), accumulate=True, c_slack=4),
    _c("d_c9_w", "dgrad", cout=9, dims=(4, 8, 48), c_slack=16, c0=2),
    # ---- resident weights (convt_res_kernel): persistent workgroups, launch_res gives per = ceil(tiles / min(tiles, 256)) tiles each
    _c("rf_one", "fwd", resident=True, tr="none", expect=dict(tiles=1, per=1, wgs=1)),
    _c("rf_scale", "fwd", resident=True, dims=(8, 16, 32), tr="scale", c0=2, expect=dict(tiles=8, per=1, wgs=8)),
    _c("rf_shift", "fwd", resident=True, B=3, dims=(12, 8, 16), tr="shift", bias=False, x_slack=4, expect=dict(tiles=9, per=1, wgs=9)),
    _c("rf_pre", "fwd", resident=True, dims=(4, 24, 16), tr="pre", c_slack=8, expect=dict(tiles=3, per=1, wgs=3)),
    _c("rf_post", "fwd", resident=True, dims=(4, 8, 48), tr="post", expect=dict(tiles=3, per=1, wgs=3)),
    _c("rf_261", "fwd", resident=True, B=3, dims=(116, 24, 16), tr="both", c_extra=0, c_slack=4,         # a short last workgroup on a
       expect=dict(tiles=261, per=2, wgs=131)),                                                          # grid of 131 = 3 mod 8
    _c("rd_c1", "dgrad", resident=True, cout=1, dims=(8, 16, 32), expect=dict(tiles=8, per=1, wgs=8)),
    _c("rd_c1_acc", "dgrad", resident=True, cout=1, dims=(4, 8, 48), accumulate=True, c_slack=4, expect=dict(tiles=3, per=1, wgs=3)),
    _c("rd_c2", "dgrad", resident=True, cout=2, dims=(4, 24, 16), c0=2, expect=dict(tiles=3, per=1, wgs=3)),
    _c("rd_c2_acc", "dgrad", resident=True, cout=2, B=3, accumulate=True, x_slack=8, expect=dict(tiles=3, per=1, wgs=3)),
    _c("rd_261_c1", "dgrad", resident=True, cout=1, B=3, dims=(116, 24, 16), c_extra=1, expect=dict(tiles=261, per=2, wgs=131)),
    _c("rd_257_c2_acc", "dgrad", resident=True, cout=2, dims=(1028, 8, 16), accumulate=True, c_extra=0, c_slack=4,
       expect=dict(tiles=257, per=2, wgs=129)),                                                          # 129 = 1 mod 8
    # ---- weight gradient (crn_convt_s2k7_wgrad_bf3), each row with both stagings of T(x)
    *_both_stagings("g_t1_c1", cout=1, dims=(2, 8, 16), expect=dict(ntiles=1, tiles_per_wg=(1, 1, 1, 1), wg_end=(1, 2, 3, 4))),
    *_both_stagings("g_t57_c9", cout=9, dims=(38, 8, 48), tr="both", npad=80, x_slack=4,                 # pair 0: 28 workgroups of two
                    expect=dict(ntiles=57, tiles_per_wg=(2, 2, 2, 1), wg_end=(29, 58, 87, 144))),        # tiles and one of one tile
    *_both_stagings("g_c16_acc", cout=16, B=2, dims=(6, 8, 16), tr="pre", accumulate=True, c_slack=8,
                    expect=dict(ntiles=6, tiles_per_wg=(2, 2, 2, 1), wg_end=(3, 6, 9, 15))),
    *_both_stagings("g_c9_npad96", cout=9, B=3, dims=(2, 16, 16), tr="shift", npad=96, accumulate=True, c0=2,
                    expect=dict(ntiles=6, tiles_per_wg=(2, 2, 2, 1), wg_end=(3, 6, 9, 15))),
    *_both_stagings("g_c1_post", cout=1, dims=(4, 8, 32), tr="post", npad=16, c_slack=4,
                    expect=dict(ntiles=4, tiles_per_wg=(2, 2, 2, 1), wg_end=(2, 4, 6, 10))),
    *_both_stagings("g_c16_scale", cout=16, dims=(2, 8, 32), tr="scale", x_slack=8,
                    expect=dict(ntiles=2, tiles_per_wg=(2, 2, 2, 1), wg_end=(1, 2, 3, 5))),
    _c("g_det", "wgrad", cout=9, B=2, tr="pre", npad=80, deterministic=True, ximg="fused",
       expect=dict(ntiles=4, tiles_per_wg=(2, 2, 2, 1), wg_end=(2, 4, 6, 10))),
    # ---- operand image (crn_convt_s2k7_ximage): one thread per 4 positions, blocks of 256; (3, 5, 12) only has W % 4 == 0
    _c("x_none", "ximage", B=2, dims=(3, 5, 12), x_slack=4),                                # 45 threads: a partial block
    _c("x_scale", "ximage", dims=(8, 16, 12), tr="scale"),                                  # 384 threads: a full and a partial block
    _c("x_shift", "ximage", B=3, dims=(3, 5, 12), tr="shift", x_slack=8),
    _c("x_pre", "ximage", dims=(2, 8, 16), tr="pre"),                                       # 64 threads
    _c("x_post", "ximage", B=2, dims=(3, 5, 12), tr="post"),
    _c("x_both", "ximage", dims=(8, 16, 12), tr="both", x_slack=4),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------------------ host loops, mirrored
def res_deal(tiles):
  """launch_res: (tiles per workgroup, workgroups) of the resident kernels."""
  per = -(-tiles // min(tiles, 256))
  return per, -(-tiles // per)


def wgrad_deal(ntiles):
  """crn_convt_s2k7_wgrad_bf3: one round of at most 256 workgroups dealt to the four (rd, rh) pairs in proportion to the cost of a
  tile (taps per wave x 8 waves + 24 for the staging) -> (tiles_per_wg, wg_end)."""
  cost = [t_ + 24 for t_ in (40, 48, 48, 64)]
  blocks = min(256, 4 * ntiles)
  per, end, wgs = [], [], 0
  for p in range(4):
    n = min(max(1, blocks * cost[p] // sum(cost)), ntiles)
    per.append(-(-ntiles // n))
    wgs += -(-ntiles // per[-1])
    end.append(wgs)
  return tuple(per), tuple(end)


def tiles_of(c):
  D, H, W = c.dims
  td = 2 if c.op == "wgrad" else 4
  return c.B * (D // td) * (H // 8) * (W // 16)


# ------------------------------------------------------------------------------------------------ inputs
class Lay:
  """A [B, C, D, H, W] view inside a flat storage: channels [c0, c0 + C) of ctot, sC = D H W + c_slack, sB = ctot sC + b_slack,
  8 elements behind the last sample."""

  def __init__(self, B, C, dims, c0=0, ctot=None, c_slack=0, b_slack=0):
    self.B, self.C, self.dims = B, C, tuple(dims)
    D, H, W = dims
    self.sC = D * H * W + c_slack
    self.sB = (ctot or C) * self.sC + b_slack
    self.off = c0 * self.sC
    self.numel = B * self.sB + 8

  def view(self, st):
    D, H, W = self.dims
    return V.View(st, self.off, self.B, self.C, D, H, W, self.sB, self.sC, H * W, W, 1)

  def mask(self):
    """bool [numel]: the elements of the storage that the view addresses (conv_fp32_cases.inside_mask for these layouts)."""
    st = t.zeros(self.numel)
    write_logical(self.view(st), t.ones(self.B, self.C, *self.dims))
    return st != 0

  def filled(self, inside, outside):
    st = t.full((self.numel,), float(outside))
    write_logical(self.view(st), inside)
    return st


class Built:
  """The seeded CPU tensors of a case (float32)."""


def build(c: Case) -> Built:
  b = Built()
  b.case = c
  g = t.Generator().manual_seed(zlib.crc32(c.name.encode()))
  rn = lambda *s: t.randn(*s, generator=g)
  D, H, W = c.dims
  b.wshape = (16, c.cout, 7, 7, 7)
  b.w = rn(*b.wshape) / float(np.sqrt(16 * 343 / 8))
  b.params = t.cat([rn(WOFS), b.w.reshape(-1), rn(5)])
  b.bias = rn(c.cout) + 1.5 if (c.bias and c.op == "fwd") else None
  b.scale = b.shift = None
  if c.tr != "none":                    # (conv_fp32_cases.build: O(1) and mostly positive, a post-ReLU must not silence a channel)
    b.scale = t.rand(16, generator=g) + 0.5
    b.shift = t.zeros(16) if c.tr == "scale" else rn(16) * 0.7 + 0.5
  b.pre, b.post = c.tr in ("pre", "both"), c.tr in ("post", "both")
  b.xl = Lay(c.B, 16, c.dims, b_slack=c.x_slack)
  b.yl = Lay(c.B, c.cout, (2 * D, 2 * H, 2 * W), c.c0, c.c0 + c.cout + c.c_extra, c.c_slack)
  nan = float("nan")
  if c.op in ("fwd", "wgrad", "ximage"):
    b.xs = b.xl.filled(rn(c.B, 16, D, H, W), nan)
  if c.op == "fwd":
    b.y0 = t.full((b.yl.numel,), SENTINEL)
  if c.op in ("dgrad", "wgrad"):
    b.dys = b.yl.filled(rn(c.B, c.cout, 2 * D, 2 * H, 2 * W), nan)
  if c.op == "dgrad":
    b.x0 = rn(b.xl.numel) if c.accumulate else t.full((b.xl.numel,), SENTINEL)
  if c.op == "wgrad":
    n = 16 * 64 * c.Npad + 8
    b.dw0 = rn(n) if c.accumulate else t.full((n,), SENTINEL)
  return b


def image_of(b, wofs=WOFS):
  """(table, the weight image of the row's kernel as the contract emulator gathers it from the parameter slab)."""
  c = b.case
  fn = {("fwd", False): G.convt_par_fwd_table, ("dgrad", False): G.convt_par_dgrad_table,
        ("fwd", True): G.convt_res_fwd_table, ("dgrad", True): G.convt_res_dgrad_table}[(c.op, c.resident)]
  tab, nbytes = fn(b.wshape, wofs)
  img = t.zeros(nbytes, dtype=t.uint8)
  _EMU.bf3_gather_image(b.params, t.as_tensor(tab), img)
  return tab, img


# ------------------------------------------------------------------------------------------------ float64 references
def _transformed(b, x, pad_first=False):
  """T(x) in x's dtype (float32: multiply, then add, as the kernels do -- the library is built without contraction), zero-padded by
  (1, 2) per dimension: the 4^3 window z of position q reads q + z - 1.  pad_first: the transform applied to the padding too (a bug)."""
  pad = lambda v: F.pad(v, [1, 2, 1, 2, 1, 2])
  if pad_first: x = pad(x)
  if b.scale is not None:
    sh = [1, -1, 1, 1, 1]
    if b.pre: x = x.relu()
    x = x * b.scale.to(x.dtype).view(sh) + b.shift.to(x.dtype).view(sh)
    if b.post: x = x.relu()
  return x if pad_first else pad(x)


def x_logical(b, dtype):
  return logical(b.xl.view(b.xs)).to(dtype)


def dy_logical(b, dtype):
  return logical(b.yl.view(b.dys)).to(dtype)


def _crop(xp):
  return xp[:, :, 1:-2, 1:-2, 1:-2]


def ref_fwd(b, w=None):
  """conv_transpose3d(T(x), w, bias) on doubles -> [B, cout, 2D, 2H, 2W]."""
  w = b.w.double() if w is None else w
  return F.conv_transpose3d(_crop(_transformed(b, x_logical(b, t.float64))), w, None if b.bias is None else b.bias.double(),
                            stride=2, padding=3, output_padding=1)


def ref_dgrad(b, w=None):
  """Its adjoint -> [B, 16, D, H, W]."""
  return F.conv3d(dy_logical(b, t.float64), b.w.double() if w is None else w, stride=2, padding=3)


def ref_wgrad(b):
  """Autograd in float64 -> [16, cout, 7, 7, 7]."""
  with t.enable_grad():
    w = b.w.double().clone().requires_grad_(True)
    y = F.conv_transpose3d(_crop(_transformed(b, x_logical(b, t.float64))), w, None, stride=2, padding=3, output_padding=1)
    (gw,) = t.autograd.grad(y, w, dy_logical(b, t.float64))
  return gw


def ref_ximage(b):
  """bf16 hi / lo of the float32 T(x): int16 [B][region = chunk * 2 + (hi, lo)][position][8 channels of the chunk]."""
  tx = _crop(_transformed(b, x_logical(b, t.float32)))
  hi = tx.to(t.bfloat16)
  lo = (tx - hi.float()).to(t.bfloat16)
  B = b.case.B
  img = t.stack([hi[:, :8], lo[:, :8], hi[:, 8:], lo[:, 8:]], 1).reshape(B, 4, 8, -1).permute(0, 1, 3, 2).contiguous()
  return img.view(t.int16)


# ------------------------------------------------------------------------------------------------ the walk model
PARITIES = [(rd, rh, rw) for rd in range(2) for rh in range(2) for rw in range(2)]       # column blocks in this order


def _split(v):
  """hi = bf16(v), lo = bf16(v - hi) of a float32 tensor, as float32 (round to nearest even, split8 of csrc/bf3_common.h)."""
  hi = v.to(t.bfloat16).float()
  return hi, (v - hi).to(t.bfloat16).float()


class Windows:
  """What a weight image holds, read the way the kernel reads it: per output parity r = (rd, rh, rw) the 4^3 window of weights
  k[term][r] = float64 [out channels][in channels][zd][zh][zw] (term 0 = hi, 1 = lo; zero where the walk has no step), and
  `read`: which bf16 elements of the image the walk multiplies into a real output."""

  def __init__(self, img, n_out, n_in):
    self.ent = img.view(t.int16).view(-1, 8).view(t.bfloat16).double()         # entries of 8 bf16
    self.read = t.zeros(self.ent.shape, dtype=t.bool)
    self.k = [{r: t.zeros(n_out, n_in, 4, 4, 4, dtype=t.float64) for r in PARITIES} for _ in range(2)]

  def take(self, e_hi, e_lo, n, ch=slice(0, 8)):
    """n consecutive entries from e_hi / e_lo, their channels ch -> ([n, len(ch)] hi, lo)."""
    self.read[e_hi:e_hi + n, ch] = True
    self.read[e_lo:e_lo + n, ch] = True
    return self.ent[e_hi:e_hi + n, ch], self.ent[e_lo:e_lo + n, ch]

  def unread_max(self):
    """The largest |element| the walk never uses for a real output: the kernel multiplies most of them, so they must be zero."""
    return float(t.where(self.read, t.zeros(()).double(), self.ent).abs().max())


def windows_walk_fwd(img, cout):
  """Forward walk (convt_par_fwd_kernel): steps = (rd, rh) pairs x 8-channel chunks of the input x window planes zd < 3 + rd; a step
  = hi[3 + rh rows zh][4 taps zw][32 columns] then lo[...]; column = rw * 16 + n; entry = the chunk's 8 input channels; the weight
  at window position z of output parity r is tap k = 5 - 2 z + r."""
  wd = Windows(img, cout, 16)
  off = 0
  for rd in range(2):
    for rh in range(2):
      rows = 3 + rh
      for ch in range(2):
        for zd in range(3 + rd):
          hi0, lo0 = off, off + rows * 128
          for zh in range(rows):
            for zw in range(4):
              for rw in range(2):
                if 5 - 2 * zw + rw < 0: continue
                e = (zh * 4 + zw) * 32 + rw * 16
                h, l = wd.take(hi0 + e, lo0 + e, cout)                          # [n][8 channels of the chunk]
                wd.k[0][(rd, rh, rw)][:, ch * 8:ch * 8 + 8, zd, zh, zw] = h
                wd.k[1][(rd, rh, rw)][:, ch * 8:ch * 8 + 8, zd, zh, zw] = l
          off += rows * 256
  return wd


def windows_walk_dgrad(img, cout):
  """Data-gradient walk (convt_par_dgrad_kernel): steps = (rd, rh) pairs x 8-channel halves of n x window planes zd in [1 - rd, 4);
  rows zh in [1 - rh, 4); column = rw * 16 + c; entry = 8 output channels n of the half; window position z of parity r (the dy
  position 2 (q + z - 2) + r) meets tap k = 2 z - 1 + r."""
  wd = Windows(img, 16, cout)
  off = 0
  for rd in range(2):
    for rh in range(2):
      rows = 3 + rh
      for nh in range((cout + 7) // 8):
        nn = min(8, cout - nh * 8)
        for zd in range(1 - rd, 4):
          hi0, lo0 = off, off + rows * 128
          for zi in range(rows):
            zh = 1 - rh + zi
            for zw in range(4):
              for rw in range(2):
                if 2 * zw - 1 + rw < 0: continue
                e = (zi * 4 + zw) * 32 + rw * 16
                h, l = wd.take(hi0 + e, lo0 + e, 16, slice(0, nn))              # [c][n of the half]
                wd.k[0][(rd, rh, rw)][:, nh * 8:nh * 8 + nn, zd, zh, zw] = h
                wd.k[1][(rd, rh, rw)][:, nh * 8:nh * 8 + nn, zd, zh, zw] = l
          off += rows * 256
  return wd


def windows_res_fwd(img, cout=2):
  """Resident forward (convt_res_kernel<false>): hi[chunk][zd][zh][tap zw][16 columns], lo 2048 entries behind; column = ((rd * 2 +
  rh) * 2 + rw) * 2 + n; entry = the chunk's 8 input channels; k = 5 - 2 z + r."""
  wd = Windows(img, 2, 16)
  for ch in range(2):
    for zd in range(4):
      for zh in range(4):
        for zw in range(4):
          for r in PARITIES:
            if min(5 - 2 * zd + r[0], 5 - 2 * zh + r[1], 5 - 2 * zw + r[2]) < 0: continue
            e = ((ch * 4 + zd) * 4 + zh) * 64 + zw * 16 + ((r[0] * 2 + r[1]) * 2 + r[2]) * 2
            h, l = wd.take(e, 2048 + e, 2)
            wd.k[0][r][:, ch * 8:ch * 8 + 8, zd, zh, zw] = h
            wd.k[1][r][:, ch * 8:ch * 8 + 8, zd, zh, zw] = l
  return wd


def windows_res_dgrad(img, cout):
  """Resident data gradient (convt_res_kernel<true>): hi[chunk = rd][zd][zh][tap zw][16 columns = input channels c]; the 8 channels
  of an entry are (rh, rw, n) of dy; k = 2 z - 1 + r."""
  wd = Windows(img, 16, cout)
  for rd in range(2):
    for zd in range(4):
      for zh in range(4):
        for zw in range(4):
          e = ((rd * 4 + zd) * 4 + zh) * 64 + zw * 16
          for rh in range(2):
            for rw in range(2):
              if min(2 * zd - 1 + rd, 2 * zh - 1 + rh, 2 * zw - 1 + rw) < 0: continue
              j = rh * 4 + rw * 2
              h, l = wd.take(e, 2048 + e, 16, slice(j, j + cout))               # [c][n]
              wd.k[0][(rd, rh, rw)][:, :, zd, zh, zw] = h
              wd.k[1][(rd, rh, rw)][:, :, zd, zh, zw] = l
  return wd


def windows_of(b, img):
  c = b.case
  return {("fwd", False): windows_walk_fwd, ("dgrad", False): windows_walk_dgrad,
          ("fwd", True): windows_res_fwd, ("dgrad", True): windows_res_dgrad}[(c.op, c.resident)](img, c.cout)


def _operands(v32, v64, acc, split):
  """{term: tensor in acc}: the bf16 hi / lo of the float32 operand, or (split = False) the float64 operand whole."""
  if not split:
    return {"h": v64}
  h, l = _split(v32)
  return {"h": h.to(acc), "l": l.to(acc)}


def walk_fwd(b, wd, acc=t.float64, split=True, terms=TERMS, pad_first=False):
  """y [B, cout, 2D, 2H, 2W] without the bias: per output parity the correlation of the padded T(x) with that parity's window, the
  three products of the split operands summed in acc.  split = False: float64 T(x) whole against hi + lo of the image."""
  c = b.case
  D, H, W = c.dims
  X = _operands(_transformed(b, x_logical(b, t.float32), pad_first), None if split else _transformed(b, x_logical(b, t.float64), pad_first),
                acc, split)
  K = {"h": t.cat([wd.k[0][r] for r in PARITIES]).to(acc), "l": t.cat([wd.k[1][r] for r in PARITIES]).to(acc)}
  if not split: terms = (("h", "h"), ("h", "l"))
  s = None
  for a, w_ in terms:
    p = F.conv3d(X[a], K[w_])
    s = p if s is None else s + p
  y = t.zeros(c.B, c.cout, 2 * D, 2 * H, 2 * W, dtype=acc)
  for i, (rd, rh, rw) in enumerate(PARITIES):
    y[:, :, rd::2, rh::2, rw::2] = s[:, i * c.cout:(i + 1) * c.cout]
  return y


def walk_dgrad(b, wd, acc=t.float64, split=True, terms=TERMS):
  """dx [B, 16, D, H, W]: the stride-1 correlation over the space-to-depth channels (r, n) of dy, origin q - 2."""
  c = b.case
  s2d = lambda dy: F.pad(t.cat([dy[:, :, rd::2, rh::2, rw::2] for rd, rh, rw in PARITIES], 1), [2, 1, 2, 1, 2, 1])
  Y = _operands(s2d(dy_logical(b, t.float32)), None if split else s2d(dy_logical(b, t.float64)), acc, split)
  K = {"h": t.cat([wd.k[0][r] for r in PARITIES], 1).to(acc), "l": t.cat([wd.k[1][r] for r in PARITIES], 1).to(acc)}
  if not split: terms = (("h", "h"), ("h", "l"))
  s = None
  for a, w_ in terms:
    p = F.conv3d(Y[a], K[w_])
    s = p if s is None else s + p
  return s


def wgrad_real(cout, npad):
  """bool [16][64 window taps][npad]: the entries of the packed gradient that hold a tap, from the kernel's geometry: pair (rd, rh)
  owns window planes zd < 3 + rd and rows zh < 3 + rh, column block rw the taps zw < 3 + rw (k = 5 - 2 z + r >= 0); column =
  ((rd * 2 + rh) * 2 + rw) * cout + n."""
  m = t.zeros(4, 4, 4, npad, dtype=t.bool)
  for i, (rd, rh, rw) in enumerate(PARITIES):
    m[:3 + rd, :3 + rh, :3 + rw, i * cout:(i + 1) * cout] = True
  return m.reshape(1, 64, npad).expand(16, 64, npad)


def pair_class(cout, npad):
  """int [16][64][npad]: 0 / 1 / 2 for the entries of the 36-tap pair, the two 48-tap pairs and the 64-tap pair."""
  k = t.zeros(npad, dtype=t.long)
  for i, (rd, rh, rw) in enumerate(PARITIES):
    k[i * cout:(i + 1) * cout] = rd + rh
  return k.view(1, 1, npad).expand(16, 64, npad)


def walk_wgrad(b, acc=t.float64, terms=TERMS, pad_first=False, q_keep=None):
  """The packed gradient [16][64][Npad] (zero where no tap is): per parity r the correlation D_z[c][n] = sum over (b, q) of
  T(x)[b, c, q + z - 1] * dy[b, n, 2 q + r], both operands split.  q_keep(pair) -> [B, 1, D, H, W] 0 / 1: the positions whose
  tiles the pair's workgroups do walk (a knob of the sensitivity test)."""
  c = b.case
  X = _operands(_transformed(b, x_logical(b, t.float32), pad_first), None, acc, True)
  dy = dy_logical(b, t.float32)
  parts = []
  for rd, rh, rw in PARITIES:
    d = dy[:, :, rd::2, rh::2, rw::2]
    if q_keep is not None: d = d * q_keep(rd * 2 + rh)
    parts.append(d)
  Y = _operands(t.cat(parts, 1), None, acc, True)
  s = None
  for a, d_ in terms:
    p = F.conv3d(X[a].transpose(0, 1).contiguous(), Y[d_].transpose(0, 1).contiguous())          # [16][8 cout][4][4][4]
    s = p if s is None else s + p
  out = t.zeros(16, 64, c.Npad, dtype=acc)
  out[:, :, :8 * c.cout] = s.permute(0, 2, 3, 4, 1).reshape(16, 64, 8 * c.cout)
  return out * wgrad_real(c.cout, c.Npad)


def packed_index(b):
  """conv_geometry.convt_fwd's index of the layer's packed gradient at the row's Npad: long [16][64][Npad], -1 = no weight."""
  geo = G.convt_fwd(b.wshape, 3)
  assert geo.window == (4, 4, 4) and geo.pad_lo == (1, 1, 1)
  idx = t.full((16, 64, b.case.Npad), -1, dtype=t.long)
  idx[:, :, :8 * b.case.cout] = t.as_tensor(geo.index).long().view(16, 64, geo.npad)[:, :, :8 * b.case.cout]
  return idx


def unpack(b, packed):
  """[16][64][Npad] -> [16, cout, 7, 7, 7] through conv_geometry.convt_fwd(...).index."""
  idx = packed_index(b)
  gw = t.zeros(b.w.numel(), dtype=packed.dtype)
  gw[idx[idx >= 0]] = packed.reshape(16, 64, -1)[idx >= 0]
  return gw.view(b.wshape)


# ------------------------------------------------------------------------------------------------ references of a row
class Ref:
  """The float64 reference of a row, the walk model on the emulator's image, and the storage the call must leave."""

  def __init__(self, b, f32=False):
    c = b.case
    self.f32_vs_split = None
    if c.op == "wgrad":
      self.grad = ref_wgrad(b)                                                  # [16, cout, 7, 7, 7]
      self.range = float(self.grad.abs().max())
      self.model = walk_wgrad(b)
      self.real = wgrad_real(c.cout, c.Npad).reshape(-1)
      self.base = b.dw0[:-8].double() if c.accumulate else t.zeros(self.real.numel(), dtype=t.float64)
      self.split_vs_f64 = float((unpack(b, self.model) - self.grad).abs().max()) / self.range
      if f32: self.f32_vs_split = float((walk_wgrad(b, t.float32).double() - self.model).abs().max()) / self.range
      return
    self.tab, self.img = image_of(b)
    wd = windows_of(b, self.img)
    if c.op == "fwd":
      bias = 0.0 if b.bias is None else b.bias.double().view(1, -1, 1, 1, 1)
      conv, model, walk, lay, base = ref_fwd(b), walk_fwd(b, wd) + bias, walk_fwd, b.yl, b.y0
    else:
      conv, model, walk, lay, base = ref_dgrad(b), walk_dgrad(b, wd), walk_dgrad, b.xl, b.x0
    self.conv, self.model = conv, model
    self.range = float(conv.abs().max())
    self.mask = lay.mask()
    self.want = self.storage(b, conv)
    self.want_model = self.storage(b, model)
    self.split_vs_f64 = float((model - conv).abs().max()) / self.range
    if f32:
      m32 = walk(b, wd, t.float32).double() + (bias if c.op == "fwd" else 0.0)
      self.f32_vs_split = float((m32 - model).abs().max()) / self.range

  def storage(self, b, val, accumulate=None):
    """float64 storage: what the buffer held outside the view, (that +) val inside."""
    c = b.case
    acc = c.accumulate if accumulate is None else accumulate
    lay, base = (b.yl, b.y0) if c.op == "fwd" else (b.xl, b.x0)
    st = base.double().clone()
    write_logical(lay.view(st), val, acc)
    return st

  def check(self, b, got):
    """fwd / dgrad -> (error inside the view against float64 / range, against the walk model, NaN-free, outside bit-identical)."""
    got = got.detach().cpu()
    base = b.y0 if b.case.op == "fwd" else b.x0
    nan_free = not bool(got.isnan().any())
    outside = bool(t.equal(got[~self.mask].view(t.int32), base[~self.mask].view(t.int32)))
    return err_inside(got, self.want, self.mask, self.range), err_inside(got, self.want_model, self.mask, self.range), nan_free, outside

  def check_wgrad(self, b, got, real_only=False):
    """-> (error of the un-packed gradient against float64 autograd / range, {pair class: error of the real entries against the walk
    model}, NaN-free, everything that holds no tap right: zero after a zero_first call, else the bits it held; the 8 elements
    behind the buffer always).  real_only: the generic engine ran (entries of real columns at structural zeros are its own)."""
    c = b.case
    got = got.detach().cpu()
    body, tail = got[:-8], got[-8:]
    delta = (body.double() - self.base).view(16, 64, c.Npad)
    e64 = float((unpack(b, delta) - self.grad).abs().max()) / self.range
    d = (delta - self.model).abs().reshape(-1)
    cls = pair_class(c.cout, c.Npad).reshape(-1)
    emod = {k: float(d[self.real & (cls == k)].max()) / self.range for k in range(3)}
    rest = ~self.real
    if real_only: rest = rest & (t.arange(c.Npad) >= 8 * c.cout).expand(16, 64, c.Npad).reshape(-1)
    held = b.dw0[:-8][rest] if c.accumulate else t.zeros(int(rest.sum()))
    rest_ok = bool(t.equal(body[rest].view(t.int32), held.view(t.int32))) and bool(t.equal(tail.view(t.int32), b.dw0[-8:].view(t.int32)))
    return e64, emod, not bool(got.isnan().any()), rest_ok


# ------------------------------------------------------------------------------------------------ running a row on the GPU
def _raw(rc, what):
  assert rc == 0, f"{what}: status {rc}"


def run_fwd(be, b, dev, wimg):
  """The row's crn_convt_s2k7_fwd_bf3 / _c2_fwd_bf3 call -> the output storage.  Through HipBackend.convt_par_fwd where the output
  is dense inside a sample, through the raw C entry where y_sC is larger than a volume (the wrapper's assert would refuse it)."""
  from corenet_amd import _lib
  from corenet_amd.backend import _ctr
  c = b.case
  xs, y = b.xs.to(dev), b.y0.to(dev).clone()
  tr = transform_of(b, dev)
  bias = None if b.bias is None else b.bias.to(dev)
  xv, yv = b.xl.view(xs), b.yl.view(y)
  D, H, W = c.dims
  if c.c_slack == 0:
    be.convt_par_fwd(logical(xv), tr, wimg, bias, logical(yv), c.cout, resident=c.resident)
  else:
    fn = be.lib._crn_convt_s2k7_c2_fwd_bf3 if c.resident else be.lib._crn_convt_s2k7_fwd_bf3
    _raw(fn(xs.data_ptr(), xv.sB, c.B, D, H, W, _ctr(tr), wimg.data_ptr(), None if bias is None else bias.data_ptr(),
            y.data_ptr() + 4 * yv.offset, yv.sB, yv.sC, c.cout, _lib.stream()), c.name)
  return y


def run_dgrad(be, b, dev, wimg):
  from corenet_amd import _lib
  c = b.case
  dys, dx = b.dys.to(dev), b.x0.to(dev).clone()
  xv, yv = b.xl.view(dx), b.yl.view(dys)
  D, H, W = c.dims
  if c.c_slack == 0:
    be.convt_par_dgrad(logical(yv), c.cout, wimg, logical(xv), c.accumulate, resident=c.resident)
  else:
    fn = be.lib._crn_convt_s2k7_c2_dgrad_bf3 if c.resident else be.lib._crn_convt_s2k7_dgrad_bf3
    _raw(fn(dys.data_ptr() + 4 * yv.offset, yv.sB, yv.sC, c.cout, c.B, D, H, W, wimg.data_ptr(), dx.data_ptr(), xv.sB,
            int(c.accumulate), _lib.stream()), c.name)
  return dx


def run_ximage(be, b, dev):
  """-> (the image buffer: crn_convt_s2k7_ximage_bytes + 64 bytes that held 0xA5, the image's size)."""
  from corenet_amd import _lib
  from corenet_amd.backend import _ctr
  c = b.case
  D, H, W = c.dims
  xs = b.xs.to(dev)
  tr = transform_of(b, dev)
  nb = be.lib.crn_convt_s2k7_ximage_bytes(c.B, D, H, W)
  img = t.full((nb + 64,), 0xA5, dtype=t.uint8, device=dev)
  _raw(be.lib._crn_convt_s2k7_ximage(xs.data_ptr(), b.xl.sB, c.B, D, H, W, _ctr(tr), img.data_ptr(), nb, _lib.stream()), c.name)
  return img, nb


def run_wgrad(be, b, dev, want_rc=0):
  """The row's crn_convt_s2k7_wgrad_bf3 call (the raw C entry: only it takes a null operand image) -> the gradient storage."""
  from corenet_amd import _lib
  from corenet_amd.backend import _ctr
  c = b.case
  D, H, W = c.dims
  xs, dys, dw = b.xs.to(dev), b.dys.to(dev), b.dw0.to(dev).clone()
  tr = transform_of(b, dev)
  yv = b.yl.view(dys)
  img = run_ximage(be, b, dev)[0] if c.ximg == "ahead" else None
  rc = be.lib._crn_convt_s2k7_wgrad_bf3(xs.data_ptr(), b.xl.sB, c.B, D, H, W, _ctr(tr), dys.data_ptr() + 4 * yv.offset, yv.sB, yv.sC,
                                        c.cout, dw.data_ptr(), c.Npad, int(not c.accumulate), None if img is None else img.data_ptr(),
                                        _lib.stream())
  assert rc == want_rc, f"{c.name}: status {rc}"
  return dw


def run_wgrad_dispatch(be, b, dev):
  """conv_wgrad(math="ct_par") on the row's views, as the engine calls it (the space-to-depth view of dy's own storage)."""
  c = b.case
  assert c.c0 == 0
  D, H, W = c.dims
  xs, dys, dw = b.xs.to(dev), b.dys.to(dev), b.dw0.to(dev).clone()
  geo = G.convt_fwd(b.wshape, 3)
  assert geo.npad == c.Npad
  ds = t.as_strided(dys, (c.B, c.cout + c.c_extra, 2 * D, 2 * H, 2 * W), (b.yl.sB, b.yl.sC, 4 * H * W, 2 * W, 1))
  dyv = V.space_to_depth_view(V.view_of(ds).channels(0, c.cout), (2, 2, 2), parity_major=True)
  be.conv_wgrad(b.xl.view(xs), transform_of(b, dev), dyv, dw, c.Npad, geo.window, geo.pad_lo, not c.accumulate,
                boxes=(geo.n_boxes, geo.c_boxes), math="ct_par")
  return dw
