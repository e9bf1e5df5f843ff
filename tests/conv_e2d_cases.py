"""The case table of the encoder convolution engine (csrc/conv_e2d.hip) and what its tests share.  TEST INFRASTRUCTURE ONLY.

One row = one crn_conv2d_bf3 or crn_conv_wgrad_2d_bf3 call on views of seeded tensors, and the kernel variant the row is there for
(`expect`: fields of the plan query crn_conv2d_bf3_plan / crn_conv_wgrad_2d_bf3_plan).  The Case dataclass, the view kinds, the
seeded inputs, the float64 references and the sentinel discipline are those of tests/conv_fp32_cases.py; the split model and the
reference classes those of tests/conv_bf3_cases.py.  tests/test_conv_e2d_plan_cpu.py asks the queries on the CPU and proves what
the table reaches; tests/test_conv_e2d_gpu.py runs every row on the GPU.

Shapes were worked out from the selection arithmetic (kFill = 256 forward, 512 weight gradient), smallest first: 12 x 48 = 3 x 3
tiles of 4 x 16 (one tile touches no border); 24 x 24 = 3 x 3 tiles of 8 x 8; 32 x 32 at batch 4 with 256 output columns (24 x 24
with 512) = 256 workgroups or more, so three chunks run in ONE split through both LDS buffers.  No tensor has more than about 2M
elements.

Bars.  Against float64: BAR = 2e-5 of max|reference| (the project's bar for the split-bf16 engines).  Against the split model:
SPLIT_BAR = 4 x SPLIT_MAX_F32, four times the largest difference between float32 and float64 summation of the split model over all
rows.  Measured on an MI355X, largest error per kernel family, of max|reference| (against float64 / against the split model):
  forward 1x1, store / accumulate / split         5.9e-6 / 2.4e-7   5.8e-6 / 2.9e-7   5.5e-6 / 2.7e-7
  forward 3x3 on 4 x 16 tiles, the same three    5.8e-6 / 3.7e-7   4.7e-6 / 4.7e-7   4.4e-6 / 2.3e-7
  forward 3x3 on 8 x 8 tiles, the same three     5.4e-6 / 4.7e-7   5.2e-6 / 5.0e-7   4.9e-6 / 2.4e-7
  weight gradient 1x1, one block / split over K  6.8e-6 / 2.6e-7   4.9e-6 / 1.7e-7
  weight gradient 3x3, one block / split over K  7.2e-6 / 2.0e-7   5.9e-6 / 1.1e-7
The operand split alone (the split model summed in float64) is within 2.5e-6 .. 7.2e-6 of float64 on the rows here; SPLIT_BAR = 4 x 4.62e-7.
The operand table of operand_layers() came out bit-identical to the contract emulator's.
"""
from __future__ import annotations

import zlib

import torch as t

import conv_bf3_cases as KB
import conv_fp32_cases as K32
from conv_bf3_cases import Case, BAR, make_ref, expected_y, bias_logical, split_fwd, split_wgrad       # noqa: F401 (shared)
from conv_fp32_cases import SENTINEL, make_view, view_numel, inside_mask, xview, yview, transform_of    # noqa: F401 (shared)
from kernel_contract_emu import EmuBackend
from corenet_amd.model import conv_geometry as G

SPLIT_MAX_F32 = 4.62e-7     # the largest difference, over all rows, between the split model summed in float32 (torch's order) and
                            # in float64, of max|reference| (tests/test_conv_e2d_plan_cpu.py measures it: row g1_det_k24)
SPLIT_BAR = 4 * SPLIT_MAX_F32     # the kernel against the split model: only the order of the float32 sums differs (32-deep MFMA
                                  # blocks, two accumulator sets, split-K partial sums, atomics in the weight gradient)
_EMU = EmuBackend()
K3, K1 = (1, 3, 3), (1, 1, 1)
P1 = (0, 1, 1)


def _f(name, expect, **kw):
  return Case(name, expect, **kw)


def _g(name, expect, **kw):
  kw.setdefault("bias", False)
  return Case(name, expect, op="wgrad", **kw)


# ------------------------------------------------------------------------------------------------ the table
# expect = what the plan query says for the row; a retune that moves a row fails tests/test_conv_e2d_plan_cpu.py, and the row then
# gets another shape (smallest first), never another expectation.
CASES = [
    # ---- 3x3 on tiles of 4 x 16: 12 x 48 = 3 x 3 tiles; splits of 1, 2 + 1, 2 + 2 + 1, 16 x 1 and (over the cap of 16) 8 x 2 + 1
    _f('a_c32', dict(kernel='k3w16', tiles=9, nblk=1, nchunks=1, per_split=1, splits=1, mode=0, tab=32, grid_x=9, grid_y=1, grid_z=1),
       cin=32, cout=64, k=K3, pad=P1, odims=(1, 12, 48), tr='pre'),
    _f('a_c96_b2', dict(kernel='k3w16', nchunks=3, per_split=2, splits=2, mode=3, tab=64, grid_x=18),
       B=2, cin=96, cout=64, k=K3, pad=P1, odims=(1, 12, 48), tr='both', bias_b=True, xview='slice', yview='slice'),
    _f('a_c160', dict(kernel='k3w16', nchunks=5, per_split=2, splits=3, mode=3, tab=64),
       cin=160, cout=64, k=K3, pad=P1, odims=(1, 12, 48), tr='post', bias=False, accumulate=True, xview='nc', yview='nc'),
    _f('a_c512', dict(kernel='k3w16', nchunks=16, per_split=1, splits=16, mode=3, tab=0, grid_z=16),
       cin=512, cout=64, k=K3, pad=P1, odims=(1, 12, 48)),
    _f('a_c544', dict(kernel='k3w16', nchunks=17, per_split=2, splits=9, mode=3, tab=64, grid_y=2, grid_z=9),
       cin=544, cout=128, k=K3, pad=P1, odims=(1, 12, 48), tr='shift'),
    _f('a_4x16', dict(kernel='k3w16', tiles=1, nchunks=2, per_split=1, splits=2, mode=3, tab=32),       # one tile holding all four borders
       B=3, cin=64, cout=64, k=K3, pad=P1, odims=(1, 4, 16), tr='pre', bias_b=True, accumulate=True),
    # three chunks in one split (both LDS buffers, the steady-state vmcnt counts), store and accumulate
    _f('a_3ch_m0', dict(kernel='k3w16', tiles=16, nchunks=3, per_split=3, splits=1, mode=0, tab=0, grid_x=64, grid_y=4),
       B=4, cin=96, cout=256, k=K3, pad=P1, odims=(1, 32, 32)),
    _f('a_3ch_m1', dict(kernel='k3w16', tiles=16, nchunks=3, per_split=3, splits=1, mode=1, tab=96),
       B=4, cin=96, cout=256, k=K3, pad=P1, odims=(1, 32, 32), tr='both', bias_b=True, accumulate=True, yview='slice'),
    _f('a_dgrad', dict(kernel='k3w16', nchunks=1, splits=1, mode=1, tab=0),
       cin=32, cout=64, k=K3, pad=P1, odims=(1, 12, 48), geom='dgrad', bias=False, accumulate=True),
    # pads 0 .. 2 per axis (8 x 32 = 2 x 2 tiles)
    _f('a_pad00', dict(kernel='k3w16', tiles=4, splits=1, mode=0, tab=32), cin=32, cout=64, k=K3, pad=(0, 0, 0), odims=(1, 8, 32), tr='pre'),
    _f('a_pad22', dict(kernel='k3w16', tiles=4, splits=2, mode=3, tab=32), cin=64, cout=64, k=K3, pad=(0, 2, 2), odims=(1, 8, 32), tr='both'),
    _f('a_pad02', dict(kernel='k3w16', tiles=4, splits=2, mode=3, tab=0), cin=64, cout=64, k=K3, pad=(0, 0, 2), odims=(1, 8, 32)),
    _f('a_pad10', dict(kernel='k3w16', tiles=4, splits=1, mode=0, tab=32), cin=32, cout=64, k=K3, pad=(0, 1, 0), odims=(1, 8, 32), tr='post'),
    # ---- 3x3 on tiles of 8 x 8: 24 x 24 = 3 x 3 tiles, 8 x 8 = one tile, 8 x 40 = five in a row
    _f('b_24_c96', dict(kernel='k3w8', tiles=9, nchunks=3, per_split=2, splits=2, mode=3, tab=64),
       cin=96, cout=64, k=K3, pad=P1, odims=(1, 24, 24), tr='pre'),
    _f('b_8x8_c32_b2', dict(kernel='k3w8', tiles=1, nchunks=1, splits=1, mode=0, tab=32, grid_x=2),
       B=2, cin=32, cout=64, k=K3, pad=P1, odims=(1, 8, 8), tr='shift', bias_b=True),
    _f('b_8x40_c160', dict(kernel='k3w8', tiles=5, nchunks=5, per_split=2, splits=3, mode=3, tab=64),
       cin=160, cout=64, k=K3, pad=P1, odims=(1, 8, 40), tr='both', accumulate=True, xview='slice', yview='slice'),
    _f('b_3ch_m0', dict(kernel='k3w8', tiles=9, nchunks=3, per_split=3, splits=1, mode=0, tab=96, grid_x=36, grid_y=8),
       B=4, cin=96, cout=512, k=K3, pad=P1, odims=(1, 24, 24), tr='post'),
    _f('b_3ch_m1', dict(kernel='k3w8', tiles=9, nchunks=3, per_split=3, splits=1, mode=1, tab=96),
       B=4, cin=96, cout=512, k=K3, pad=P1, odims=(1, 24, 24), tr='both', bias=False, accumulate=True, xview='nc'),
    _f('b_dgrad', dict(kernel='k3w8', nchunks=2, per_split=1, splits=2, mode=3, tab=0),
       cin=64, cout=64, k=K3, pad=P1, odims=(1, 24, 24), geom='dgrad', bias=False, accumulate=True),
    _f('b_dgrad_m1', dict(kernel='k3w8', nchunks=1, splits=1, mode=1, tab=0),
       B=2, cin=32, cout=64, k=K3, pad=P1, odims=(1, 8, 8), geom='dgrad', bias=False, accumulate=True),
    _f('b_c32_notr', dict(kernel='k3w8', tiles=5, nchunks=1, splits=1, mode=0, tab=0), cin=32, cout=64, k=K3, pad=P1, odims=(1, 8, 40)),
    _f('b_nc', dict(kernel='k3w8', tiles=6, nchunks=2, per_split=1, splits=2, mode=3, tab=32, grid_y=2),
       B=2, cin=64, cout=128, k=K3, pad=P1, odims=(1, 16, 24), tr='pre', bias=False, xview='nc', yview='nc'),
    _f('b_c544', dict(kernel='k3w8', tiles=1, nchunks=17, per_split=2, splits=9, mode=3, tab=64),
       cin=544, cout=64, k=K3, pad=P1, odims=(1, 8, 8), tr='post'),
    _f('b_pad00', dict(kernel='k3w8', tiles=6, splits=1, mode=0, tab=32), cin=32, cout=64, k=K3, pad=(0, 0, 0), odims=(1, 16, 24), tr='both'),
    _f('b_pad22', dict(kernel='k3w8', tiles=6, splits=2, mode=3, tab=32), cin=64, cout=64, k=K3, pad=(0, 2, 2), odims=(1, 16, 24), tr='pre'),
    _f('b_pad02', dict(kernel='k3w8', tiles=6, splits=1, mode=0, tab=0), cin=32, cout=64, k=K3, pad=(0, 0, 2), odims=(1, 16, 24)),
    _f('b_pad10', dict(kernel='k3w8', tiles=6, splits=2, mode=3, tab=32), cin=64, cout=64, k=K3, pad=(0, 1, 0), odims=(1, 16, 24), tr='shift'),
    # ---- 1x1: chunks of four 32-channel blocks, one per wave
    _f('c_c32', dict(kernel='k1', tiles=1, nblk=1, nchunks=1, splits=1, mode=0, tab=128, grid_x=2),       # three dead waves while staging
       B=2, cin=32, cout=64, odims=(1, 8, 8), tr='pre'),
    _f('c_c128', dict(kernel='k1', nblk=4, nchunks=1, splits=1, mode=0, tab=0), cin=128, cout=64, odims=(1, 8, 8), bias_b=True),
    _f('c_c160_s192', dict(kernel='k1', tiles=3, nblk=5, nchunks=2, per_split=1, splits=2, mode=3, tab=128),     # split 1: one live block, table
       cin=160, cout=64, odims=(1, 8, 24), tr='both'),                                                           # origin 128: the clamp
    _f('c_c160_acc', dict(kernel='k1', tiles=3, nblk=5, nchunks=2, per_split=1, splits=2, mode=3, tab=128, grid_x=6),
       B=2, cin=160, cout=64, odims=(1, 8, 24), tr='post', bias_b=True, accumulate=True, xview='slice', yview='slice'),
    _f('c_c288_m0', dict(kernel='k1', tiles=16, nblk=9, nchunks=3, per_split=3, splits=1, mode=0, tab=384, grid_x=64, grid_y=4),
       B=4, cin=288, cout=256, odims=(1, 32, 32), tr='shift'),                                                   # last chunk: one block
    _f('c_c288_m1', dict(kernel='k1', tiles=16, nblk=9, nchunks=3, per_split=3, splits=1, mode=1, tab=384),
       B=4, cin=288, cout=256, odims=(1, 32, 32), tr='pre', bias=False, accumulate=True, xview='slice', yview='slice'),
    _f('c_dgrad_m1', dict(kernel='k1', nchunks=1, splits=1, mode=1, tab=0),
       cin=64, cout=64, odims=(1, 8, 8), geom='dgrad', bias=False, accumulate=True),
    _f('c_c2176', dict(kernel='k1', nblk=68, nchunks=17, per_split=2, splits=9, mode=3, tab=256, grid_z=9),
       cin=2176, cout=64, odims=(1, 8, 8), tr='post', bias=False),
    _f('c_vol', dict(kernel='k1', tiles=3, nchunks=1, splits=1, mode=0, tab=128, grid_x=6, grid_y=2),
       B=2, cin=64, cout=128, odims=(3, 8, 8), tr='pre', xview='nc', yview='nc'),
    _f('c_nc_split', dict(kernel='k1', nchunks=2, per_split=1, splits=2, mode=3, tab=0), cin=256, cout=64, odims=(1, 8, 8), xview='nc', yview='nc'),
    _f('c_dgrad_split', dict(kernel='k1', tiles=2, nblk=9, nchunks=3, per_split=2, splits=2, mode=3, tab=0),
       cin=288, cout=64, odims=(1, 8, 16), geom='dgrad', bias=False, accumulate=True),
    # ---- weight gradient 1x1: tiles of 64 channels x 32 columns, K steps of 32 positions, every fourth per wave
    _g('g1_c67_n12_k1', dict(kernel='wg1', row_tiles=2, col_tiles=1, ksteps=1, per_block=1, splits=1),         # three idle waves
       cin=67, cout=12, odims=(1, 4, 8), tr='both'),
    _g('g1_c35_n40_k5', dict(kernel='wg1', row_tiles=1, col_tiles=2, ksteps=5, per_block=5, splits=1),
       cin=35, cout=40, odims=(1, 8, 20), tr='post', accumulate=True),
    _g('g1_c64_n64_k9', dict(kernel='wg1', row_tiles=1, col_tiles=2, ksteps=9, per_block=9, splits=1),         # steps 3 and 6 start a sample
       B=3, cin=64, cout=64, odims=(1, 8, 12)),
    _g('g1_k19', dict(kernel='wg1', row_tiles=2, col_tiles=1, ksteps=19, per_block=10, splits=2),
       cin=67, cout=12, odims=(1, 19, 32), tr='both', accumulate=True, xview='slice', yview='slice'),
    _g('g1_k24', dict(kernel='wg1', row_tiles=1, col_tiles=1, ksteps=24, per_block=8, splits=3),
       B=2, cin=35, cout=12, odims=(1, 16, 24), tr='post'),
    _g('g1_vol', dict(kernel='wg1', row_tiles=2, col_tiles=2, ksteps=9, per_block=9, splits=1),
       B=3, cin=67, cout=40, odims=(3, 8, 4), accumulate=True),
    _g('g1_det_k19', dict(kernel='wg1', ksteps=19, per_block=19, splits=1), cin=67, cout=12, odims=(1, 19, 32), tr='both', deterministic=True),
    _g('g1_det_k24', dict(kernel='wg1', ksteps=24, per_block=24, splits=1), B=2, cin=35, cout=40, odims=(1, 16, 24), accumulate=True,
       deterministic=True),
    # ---- weight gradient 3x3: tiles of 32 (c, zh) pairs x 32 columns
    _g('g3_4x8_c5_k1', dict(kernel='wg3', row_tiles=1, col_tiles=1, ksteps=1, per_block=1, splits=1),          # second lane group past 3*C
       cin=5, cout=12, k=K3, pad=P1, odims=(1, 4, 8), tr='both'),
    _g('g3_8x8_c11', dict(kernel='wg3', row_tiles=2, col_tiles=2, ksteps=10, per_block=10, splits=1),          # second row tile: one row
       B=5, cin=11, cout=40, k=K3, pad=P1, odims=(1, 8, 8), tr='post', accumulate=True),
    _g('g3_4x16_c32', dict(kernel='wg3', row_tiles=3, col_tiles=2, ksteps=6, per_block=6, splits=1),
       B=3, cin=32, cout=64, k=K3, pad=P1, odims=(1, 4, 16)),
    _g('g3_4x24_c11', dict(kernel='wg3', row_tiles=2, col_tiles=1, ksteps=9, per_block=9, splits=1),
       B=3, cin=11, cout=12, k=K3, pad=P1, odims=(1, 4, 24), tr='both', xview='slice', yview='slice'),
    _g('g3_8x32_c5', dict(kernel='wg3', row_tiles=1, col_tiles=2, ksteps=16, per_block=8, splits=2),
       B=2, cin=5, cout=40, k=K3, pad=P1, odims=(1, 8, 32), tr='post'),
    _g('g3_k19', dict(kernel='wg3', row_tiles=2, col_tiles=1, ksteps=19, per_block=10, splits=2),
       B=19, cin=11, cout=12, k=K3, pad=P1, odims=(1, 4, 8), tr='both', accumulate=True),
    _g('g3_k24', dict(kernel='wg3', row_tiles=1, col_tiles=1, ksteps=24, per_block=8, splits=3),
       B=3, cin=5, cout=12, k=K3, pad=P1, odims=(1, 8, 32)),
    _g('g3_k5', dict(kernel='wg3', row_tiles=3, col_tiles=2, ksteps=5, per_block=5, splits=1),
       B=5, cin=32, cout=64, k=K3, pad=P1, odims=(1, 4, 8), tr='post', accumulate=True, xview='slice', yview='slice'),
    _g('g3_det_k19', dict(kernel='wg3', ksteps=19, per_block=19, splits=1), B=19, cin=11, cout=12, k=K3, pad=P1, odims=(1, 4, 8), tr='both',
       deterministic=True),
    _g('g3_det_k24', dict(kernel='wg3', ksteps=24, per_block=24, splits=1), B=3, cin=5, cout=40, k=K3, pad=P1, odims=(1, 8, 32), accumulate=True,
       deterministic=True),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
DET_FIELDS = ("splits", "per_block", "grid_z")      # what CRN_DETERMINISTIC=1 changes in a weight-gradient plan


# ------------------------------------------------------------------------------------------------ inputs
def build(c: Case):
  """The seeded CPU tensors of a case (conv_fp32_cases.build) plus what only this engine takes: the operand blocks of the packed
  weights (forward), one bias row per sample; a 'shift' transform has scale 1."""
  b = K32.build(c)
  g = t.Generator().manual_seed(zlib.crc32(c.name.encode()) ^ 0xe2d)
  if c.tr == "shift": b.scale = t.ones(c.cin)
  b.wop = None
  if c.op == "fwd":
    desc, blocks = G.operand_table([(0, 0, b.geo)])
    b.wop = t.zeros(G.operand_entries(b.geo) * 32, dtype=t.uint8)
    _EMU.bf3_operands(b.wp, (t.as_tensor(desc), blocks), b.wop)
  KB.sample_bias(b, g)
  return b


def query_plan(be, b, xs, ys, wop=None, dw=None):
  """The plan of the case's call on these storages (be: HipBackend; any device, CPU included)."""
  c = b.case
  tr = transform_of(b, xs.device)
  if c.op == "fwd":
    return be.conv2d_bf3_plan(xview(b, xs), tr, wop, b.npad, None if b.bp is None else wop, b.bias_sB, yview(b, ys), b.window,
                              b.pad_lo, c.accumulate)
  return be.conv_wgrad_2d_bf3_plan(xview(b, xs), tr, yview(b, ys), dw, b.npad, b.window, b.pad_lo, not c.accumulate)


def run_fwd(be, b, dev):
  c = b.case
  y = b.y0.to(dev).clone()
  be.conv2d_bf3(xview(b, b.xs.to(dev)), transform_of(b, dev), b.wop.to(dev), b.npad, None if b.bp is None else b.bp.to(dev),
                b.bias_sB, yview(b, y), b.window, b.pad_lo, c.accumulate)
  return y


def run_wgrad(be, b, dev):
  c = b.case
  dw = b.dw0.to(dev).clone()
  be.conv_wgrad(xview(b, b.xs.to(dev)), transform_of(b, dev), yview(b, b.dys.to(dev)), dw, b.npad, b.window, b.pad_lo,
                not c.accumulate, math="bf16x3_2d")
  return dw


# ------------------------------------------------------------------------------------------------ the operand table
OPERAND_SENTINEL = 0xA5
OPERAND_SLACK = 4096


def operand_layers():
  """One crn_bf3_operands launch over five layers that sit out of size order, in the table and in the output: encoder order at Npad
  16 (64 entries: a quarter of a workgroup), at Npad 48 with 9 taps (13.5 workgroups), at Npad 64 (exactly one), a slab-order layer
  (13 channels: a partial chunk of 8; 12 tap slots), and one more encoder-order layer behind it.  -> (packed weights with gaps between
  the layers, desc int64 [5, 7], workgroups, bytes of the output without its slack)."""
  geos = [(G.conv_fwd((48, 64, 1, 3, 3), (0, 1, 1)), False), (G.conv_fwd((12, 32, 1, 1, 1), (0, 0, 0)), False),
          (G.conv_fwd((20, 13, 2, 3, 3), (1, 1, 1)), True), (G.conv_fwd((64, 32, 1, 1, 1), (0, 0, 0)), False),
          (G.conv_fwd((128, 96, 1, 3, 3), (0, 1, 1)), False)]
  assert [g.npad for g, _ in geos] == [48, 16, 32, 64, 128]
  ent = [G.slab_entries(g) if slab else G.operand_entries(g) for g, slab in geos]
  order = [3, 0, 4, 1, 2]                               # where the layers lie in the output: not in table order
  dst, at = {}, 0
  for i in order:
    dst[i] = at
    at += ent[i]
  gen = t.Generator().manual_seed(0xe2d0)
  src, layers, chunks = 0, [], []
  for i, (g, slab) in enumerate(geos):
    n = g.cin * g.taps * g.npad
    chunks.append(t.randn(n + 7 + i, generator=gen))    # (+ a gap: a layer does not start where the one before ended)
    layers.append((src, dst[i], g, slab))
    src += n + 7 + i
  desc, blocks = G.operand_table(layers)
  assert any(e % 256 for e in ent) and any(e % 256 == 0 for e in ent)
  return t.cat(chunks), desc, blocks, at * 32


# ------------------------------------------------------------------------------------------------ rejections
def rejections(accepted=False):
  """[(what is wrong, fwd | wgrad, make(dev), launch?)]: the good call -- forward: B 1, 32 -> 64 channels, 3x3 with pads 1 (or 1x1) on
  plain views of 8 x 16; weight gradient: 32 channels, 12 columns in Npad 16 on 4 x 8 -- with ONE thing wrong per row, one row per
  rejection of e2d_fwd_select / e2d_wg_select (csrc/conv_e2d.hip).  make(dev) -> dict(args: the C arguments without the stream /
  the plan, out: the output storage, full of SENTINEL).  Buffers have one sample of slack.  launch False: query only -- the views
  lie over small storage that nothing touches.  accepted=True: accepted calls next to them instead."""
  import ctypes as C
  from corenet_amd.backend import _cview
  from corenet_amd import views as V

  def big(st, B, Cn, dims, sC=None):                    # a dense view far larger than its storage: for the queries only
    D, H, W = dims
    S = D * H * W
    sC = S if sC is None else sC
    return V.View(st, 0, B, Cn, D, H, W, Cn * sC, sC, H * W, W, 1)

  def mk(op, dev, B=1, xB=None, cin=32, cout=None, npad=None, k=None, pad=None, dims=None, xd=None, xkind="plain", ykind="plain",
         tr=False, huge=None):
    fwd = op == "fwd"
    cout = cout if cout is not None else (64 if fwd else 12)
    npad = npad if npad is not None else (64 if fwd else 16)
    k = k or (3, 3)
    pad = pad if pad is not None else ((1, 1) if k == (3, 3) else (0, 0))
    dims = dims or ((1, 8, 16) if fwd else (1, 4, 8))
    xd = xd or dims
    slack = lambda Cn, d: Cn * d[0] * d[1] * d[2] + 8
    if huge:
      xs = t.zeros(64, device=dev); ys = t.full((64,), SENTINEL if fwd else 0.5, device=dev)
      xv, yv = _cview(big(xs, B, cin, xd, huge.get("sC"))), _cview(big(ys, B, cout, dims))
    else:
      xs = t.zeros(view_numel(xkind, xB or B, cin, xd) + slack(cin, xd), device=dev)
      ys = t.full((view_numel(ykind, B, cout, dims) + slack(cout, dims),), SENTINEL if fwd else 0.5, device=dev)
      xv, yv = _cview(make_view(xkind, xs, xB or B, cin, xd)), _cview(make_view(ykind, ys, B, cout, dims))
    w = t.zeros(max(64, 0 if huge else cin * k[0] * k[1] * npad), device=dev)
    trs = None
    if tr:
      sc = t.ones(64, device=dev)
      from corenet_amd import _lib
      trs = _lib.CrnInTransform(sc.data_ptr(), sc.data_ptr(), 0, 0)
    trp = None if trs is None else C.byref(trs)
    if fwd:
      return dict(args=(C.byref(xv), trp, w.data_ptr(), npad, None, 0, C.byref(yv), *k, *pad, 0), out=ys, keep=(xs, xv, yv, w, trs))
    dw = t.full((max(cin, 1) * 9 * max(npad, 16) * 2,), SENTINEL, device=dev)
    return dict(args=(C.byref(xv), trp, C.byref(yv), dw.data_ptr(), npad, *k, *pad, 1), out=dw, keep=(xs, ys, xv, yv, trs))

  R, A = [], []
  add = lambda name, op, launch=True, **kw: R.append((f"{op}: {name}", op, lambda dev, op=op, kw=kw: mk(op, dev, **kw), launch))
  ok = lambda name, op, launch=True, **kw: A.append((f"{op}: {name}", op, lambda dev, op=op, kw=kw: mk(op, dev, **kw), launch))
  for op in ("fwd", "wgrad"):
    add("batch mismatch", op, xB=2)
    for kind in ("off1", "sb2", "s2", "s2co", "cl"):
      add(f"x {kind}", op, xkind=kind)
      add(f"y {kind}", op, ykind=kind)
    add("extents differ", op, xd=(1, 8, 32) if op == "fwd" else (1, 4, 16))
    add("window 2x2", op, k=(2, 2), pad=(0, 0))
    add("window 5x5", op, k=(5, 5), pad=(2, 2))
    add("window 3x1", op, k=(3, 1), pad=(1, 0))
    add("1x1 with a pad", op, k=(1, 1), pad=(0, 1))
    add("3x3 over a volume", op, dims=(2, 8, 16))
    add("3x3 with W 12", op, dims=(1, 8, 12))
    add("no channels", op, cin=0)
  # ---- forward only
  add("Cin 48", "fwd", cin=48)
  add("Cout 96", "fwd", cout=96, npad=96)
  add("Npad 128 over 64 columns", "fwd", npad=128)
  for p in ((-1, 1), (1, -1), (3, 1), (1, 3)):
    add(f"3x3 pads {p}", "fwd", pad=p)
  add("3x3 on 14 x 16: H % 4", "fwd", dims=(1, 14, 16))
  add("3x3 on 6 x 8: H % 8", "fwd", dims=(1, 6, 8))
  add("1x1 over 32 positions", "fwd", k=(1, 1), dims=(1, 4, 8))
  add("a sample of 2 GiB", "fwd", launch=False, k=(1, 1), dims=(1, 4096, 4096), huge={})
  add("a sample that ends at 2 GiB through its channel stride", "fwd", launch=False, k=(1, 1), cin=64, dims=(1, 64, 64),
      huge=dict(sC=1 << 24))
  add("operand blocks of 2 GiB", "fwd", launch=False, cin=8192, cout=8192, npad=8192, huge={})
  add("3x3: tables of 16288 channels in one split past the LDS bound", "fwd", launch=False, B=4, cin=16288, dims=(1, 64, 64), tr=True, huge={})
  add("1x1: tables of 11808 channels in one split past the LDS bound", "fwd", launch=False, B=4, k=(1, 1), cin=11808, dims=(1, 128, 128),
      tr=True, huge={})
  # ---- weight gradient only
  add("x nc", "wgrad", xkind="nc")
  add("dy nc", "wgrad", ykind="nc")
  add("Npad 24", "wgrad", npad=24)
  add("Npad 0", "wgrad", npad=0)
  add("dy->C 17 > Npad", "wgrad", cout=17)
  add("3x3 pads (0, 1)", "wgrad", pad=(0, 1))
  add("3x3 pads (1, 2)", "wgrad", pad=(1, 2))
  add("1x1 over 16 positions", "wgrad", k=(1, 1), dims=(1, 4, 4))
  add("a sample of x of 2 GiB", "wgrad", launch=False, k=(1, 1), dims=(1, 4096, 4096), huge={})
  add("a sample of dy of 2 GiB", "wgrad", launch=False, k=(1, 1), cin=8, cout=32, npad=32, dims=(1, 4096, 4096), huge={})
  # ---- accepted, next to the bounds
  ok("the good call", "fwd"); ok("the good call", "wgrad")
  ok("1x1", "fwd", k=(1, 1)); ok("1x1", "wgrad", k=(1, 1))
  for p in ((0, 0), (2, 2), (0, 2), (2, 1)):
    ok(f"3x3 pads {p}", "fwd", pad=p)
  ok("3x3 on 12 x 16", "fwd", dims=(1, 12, 16)); ok("3x3 on 8 x 8", "fwd", dims=(1, 8, 8)); ok("3x3 on 16 x 24", "fwd", dims=(1, 16, 24))
  ok("1x1 over a volume", "fwd", k=(1, 1), dims=(2, 8, 16)); ok("1x1 over a volume", "wgrad", k=(1, 1), dims=(2, 8, 16))
  ok("x nc", "fwd", xkind="nc"); ok("y nc", "fwd", ykind="nc"); ok("x slice", "wgrad", xkind="slice"); ok("dy slice", "wgrad", ykind="slice")
  ok("dy->C 16 = Npad", "wgrad", cout=16); ok("Npad 32 over 12 columns", "wgrad", npad=32)
  ok("a sample one channel plane short of 2 GiB", "fwd", launch=False, k=(1, 1), cin=32, dims=(1, 4096, 4064), huge={})
  ok("3x3: tables of 16256 channels", "fwd", launch=False, B=4, cin=16256, dims=(1, 64, 64), tr=True, huge={})
  ok("1x1: tables of 11776 channels", "fwd", launch=False, B=4, k=(1, 1), cin=11776, dims=(1, 128, 128), tr=True, huge={})
  ok("3x3: 16288 channels without a transform", "fwd", launch=False, B=4, cin=16288, dims=(1, 64, 64), huge={})
  return A if accepted else R
