"""The case table of the fp32 convolution engine (csrc/conv_igemm.hip, csrc/conv_kernels.h) and what its tests share.
TEST INFRASTRUCTURE ONLY.

One row = one crn_conv_fwd or crn_conv_wgrad call: the window correlation
  y[b, n, o] = bias[n] + sum_{c, t} T(x)[b, c, o - pad + t] * w[n, c, t]
over views of seeded tensors, and the kernel variant the row is there for (`expect`: fields of the plan query
crn_conv_fwd_plan / crn_conv_wgrad_plan).  tests/test_conv_plan_cpu.py asks the query on the CPU and proves what the table
reaches; tests/test_conv_fp32_gpu.py runs every row on the GPU against the float64 references built here.

Shapes were found with the query, smallest first (W in 1, 2, 3, 4, 5, 8, 12, 16, 20; H <= 16; D <= 8; Cin <= 130;
Npad <= 128; k in 1..5): no tensor of the table has more than about 4M elements.
"""
from __future__ import annotations

import dataclasses
import zlib
from typing import Optional, Tuple

import numpy as np
import torch as t
import torch.nn.functional as F

from corenet_amd import views as V
from corenet_amd.model import conv_geometry as G
from kernel_contract_emu import logical, write_logical

SENTINEL = -1234.5          # what every output buffer holds before a non-accumulating call
BAR_FWD, BAR_WGRAD = 3e-5, 5e-5     # of max|reference|: the project's bars (tests/test_kernels_gpu.py), now against float64


@dataclasses.dataclass(frozen=True)
class Case:
  name: str
  expect: dict                       # plan fields this row is there for (path always; the generic tile where it matters)
  B: int = 1
  cin: int = 1
  cout: int = 16
  k: Tuple[int, int, int] = (1, 1, 1)
  pad: Tuple[int, int, int] = (0, 0, 0)          # low pads; the high pads follow from the extents
  odims: Tuple[int, int, int] = (1, 1, 1)        # extent of y (wgrad: of dy)
  xdims: Optional[Tuple[int, int, int]] = None   # extent of x; default = odims
  op: str = "fwd"                    # fwd | wgrad
  geom: str = "conv"                 # conv: the correlation above, w [cout, cin, k]; convT: ConvTranspose3d(k, stride 2, pad[0],
                                     # output_padding 1) onto the parity-major view of y; dgrad / convT_dgrad: the data gradient
                                     # of Conv3d(cout -> cin, k, padding pad) / of that ConvTranspose3d(cout -> cin), x = dy
  xview: str = "plain"               # plain | slice | off1 | sb2 | s2 | s2co | s2d
  yview: str = "plain"               # plain | slice | off1 | sb2 | co | s2d | cl | nc      (wgrad: the view of dy)
  tr: str = ""                       # "" | shift | pre | post | both | scale
  bias: bool = True
  accumulate: bool = False           # wgrad: zero_first = not accumulate
  splits: int = 0
  boxes: str = ""                    # "" | geom (the geometry's tap boxes) | odd (groups that do not divide the channels)
  deterministic: bool = False

  @property
  def xd(self):
    return self.xdims or self.odims

  @property
  def npad(self):
    return G.pad16(self.cout * (8 if self.geom == "convT" else 1))


# ------------------------------------------------------------------------------------------------ the table
# expect = what the plan query says for the row; a retune of a cost constant that moves a row to another kernel fails
# tests/test_conv_plan_cpu.py, and the row then gets another shape (found with the query), never another expectation.
# Trailing comments: the rest of the plan when the row was written (position tile, sub-tile width, channels per chunk,
# channel chunks / position tiles, LDS bytes) -- information, not asserted.
CASES = [
    # ---- one row per instantiated forward kernel: (MSUB, NSUB) x staging of x (0 scalars, 1 float4 units, 2 position pairs).
    # Every row has partial tiles; pads, transforms, views, bias / accumulate rotate through the rows of a staging form.
    Case('f_m1n1_x0', dict(path='generic', msub=1, nsub=1, xstage=0, forced=0, splits=1, vec_store=1),
         B=2, cin=66, cout=64, k=(2, 2, 2), odims=(5, 5, 20), xview='off1', tr='shift'),   # tile 2x2x16 mw 16 cc 32, 3 chunks, lds 42496
    Case('f_m1n1_x1', dict(path='generic', msub=1, nsub=1, xstage=1, forced=0, splits=3, vec_store=1),
         cin=66, k=(3, 3, 3), pad=(1, 1, 0), odims=(5, 5, 20), tr='shift'),   # tile 2x2x16 mw 16 cc 16, 5 chunks, lds 50688
    Case('f_m1n1_x2', dict(path='generic', msub=1, nsub=1, xstage=2, forced=0, splits=6, vec_store=1),
         cin=66, cout=40, k=(5, 5, 5), pad=(2, 2, 0), odims=(5, 5, 20), xview='s2', tr='shift'),   # tile 2x2x16 mw 16 cc 4, 17 chunks, lds 45056
    Case('f_m1n2_x0', dict(path='generic', msub=1, nsub=2, xstage=0, forced=0, splits=5, vec_store=1),
         cin=66, cout=24, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 5, 20), xview='sb2', yview='slice', tr='pre', bias=False, accumulate=True),   # tile 2x2x16 mw 16 cc 8, 9 chunks, lds 39424
    Case('f_m1n2_x1', dict(path='generic', msub=1, nsub=2, xstage=1, forced=0, splits=5, vec_store=1),
         cin=66, cout=24, k=(3, 3, 3), pad=(1, 1, 1), odims=(3, 5, 12), xview='slice', yview='slice', tr='pre', bias=False, accumulate=True),   # tile 2x2x16 mw 8 cc 8, 9 chunks, lds 42496
    Case('f_m1n2_x2', dict(path='generic', msub=1, nsub=2, xstage=2, forced=0, splits=1, vec_store=1),
         B=2, cin=3, cout=120, k=(2, 2, 2), pad=(0, 0, 1), odims=(5, 5, 20), xview='s2', yview='slice', tr='pre', bias=False, accumulate=True),   # tile 2x2x16 mw 16 cc 4, 1 chunks, lds 8704
    Case('f_m1n4_x0', dict(path='generic', msub=1, nsub=4, xstage=0, forced=0, splits=9, vec_store=0),
         cin=66, cout=64, k=(3, 3, 3), pad=(1, 1, 2), odims=(3, 5, 5), xview='s2', yview='co', tr='post', accumulate=True),   # tile 4x4x4 mw 4 cc 4, 17 chunks, lds 33280
    Case('f_m1n4_x1', dict(path='generic', msub=1, nsub=4, xstage=1, forced=0, splits=9, vec_store=1),
         cin=66, cout=64, k=(3, 3, 3), pad=(1, 1, 2), odims=(5, 3, 12), yview='co', tr='post', accumulate=True),   # tile 2x4x8 mw 8 cc 4, 17 chunks, lds 34304
    Case('f_m1n4_x2', dict(path='generic', msub=1, nsub=4, xstage=2, forced=0, splits=17, vec_store=1),
         B=2, cin=130, cout=120, k=(3, 3, 3), pad=(1, 1, 2), odims=(3, 1, 12), xview='s2', yview='co', tr='post', accumulate=True),   # tile 4x2x8 mw 8 cc 4, 33 chunks, lds 33280
    Case('f_m2n1_x0', dict(path='generic', msub=2, nsub=1, xstage=0, forced=0, splits=9, vec_store=1),
         cin=66, k=(5, 5, 5), pad=(2, 2, 3), odims=(5, 5, 20), xview='off1', yview='off1', tr='both', bias=False),   # tile 2x4x16 mw 16 cc 4, 17 chunks, lds 49152
    Case('f_m2n1_x1', dict(path='generic', msub=2, nsub=1, xstage=1, forced=0, splits=9, vec_store=1),
         cin=66, k=(5, 5, 5), pad=(2, 2, 3), odims=(5, 5, 20), xview='slice', yview='off1', tr='both', bias=False),   # tile 2x2x32 mw 16 cc 4, 17 chunks, lds 56832
    Case('f_m2n1_x2', dict(path='generic', msub=2, nsub=1, xstage=2, forced=0, splits=9, vec_store=1),
         cin=66, k=(4, 4, 4), pad=(1, 1, 3), odims=(3, 3, 20), xview='s2', yview='off1', tr='both', bias=False),   # tile 2x4x16 mw 16 cc 4, 17 chunks, lds 29696
    Case('f_m2n2_x0', dict(path='generic', msub=2, nsub=2, xstage=0, forced=0, splits=9, vec_store=1),
         B=2, cin=130, cout=40, k=(3, 3, 3), pad=(1, 1, 0), odims=(3, 3, 20), xview='off1', yview='sb2', tr='scale', boxes='odd'),   # tile 2x4x16 mw 16 cc 8, 17 chunks, lds 43520
    Case('f_m2n2_x1', dict(path='generic', msub=2, nsub=2, xstage=1, forced=0, splits=9, vec_store=1),
         cin=66, cout=24, k=(4, 4, 4), pad=(1, 1, 0), odims=(5, 5, 20), yview='sb2', tr='scale'),   # tile 2x2x32 mw 16 cc 4, 17 chunks, lds 49152
    Case('f_m2n2_x2', dict(path='generic', msub=2, nsub=2, xstage=2, forced=0, splits=9, vec_store=1),
         cin=130, cout=24, k=(2, 2, 2), odims=(5, 5, 20), xview='s2co', yview='sb2', tr='scale'),   # tile 2x2x32 mw 16 cc 8, 17 chunks, lds 20992
    Case('f_m2n4_x0', dict(path='generic', msub=2, nsub=4, xstage=0, forced=0, splits=9, vec_store=1),
         cin=66, cout=64, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 5, 20), xview='sb2', bias=False, accumulate=True),   # tile 2x2x32 mw 16 cc 4, 17 chunks, lds 38400
    Case('f_m2n4_x1', dict(path='generic', msub=2, nsub=4, xstage=1, forced=0, splits=9, vec_store=1),
         cin=66, cout=64, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 5, 20), xview='slice', bias=False, accumulate=True),   # tile 2x2x32 mw 16 cc 4, 17 chunks, lds 39936
    Case('f_m2n4_x2', dict(path='generic', msub=2, nsub=4, xstage=2, forced=0, splits=9, vec_store=1),
         cin=130, cout=64, k=(2, 2, 2), pad=(0, 0, 1), odims=(5, 5, 20), xview='s2', bias=False, accumulate=True),   # tile 2x2x32 mw 16 cc 8, 17 chunks, lds 29184
    Case('f_m4n1_x0', dict(path='generic', msub=4, nsub=1, xstage=0, forced=0, splits=17, vec_store=1),
         cin=130, k=(4, 4, 4), pad=(1, 1, 2), odims=(5, 5, 20), xview='off1', tr='shift', accumulate=True),   # tile 2x8x16 mw 16 cc 4, 33 chunks, lds 35328
    Case('f_m4n1_x1', dict(path='generic', msub=4, nsub=1, xstage=1, forced=0, splits=17, vec_store=1),
         cin=130, k=(4, 4, 4), pad=(1, 1, 2), odims=(5, 5, 20), tr='shift', accumulate=True),   # tile 2x8x16 mw 16 cc 4, 33 chunks, lds 39424
    Case('f_m4n1_x2', dict(path='generic', msub=4, nsub=1, xstage=2, forced=0, splits=9, vec_store=1),
         cin=66, k=(3, 3, 3), pad=(1, 1, 2), odims=(5, 5, 20), xview='s2', tr='shift', accumulate=True),   # tile 2x8x16 mw 16 cc 4, 17 chunks, lds 19968
    Case('f_m4n2_x0', dict(path='generic', msub=4, nsub=2, xstage=0, forced=0, splits=9, vec_store=1),
         B=2, cin=130, cout=24, k=(3, 3, 3), pad=(1, 1, 3), odims=(5, 5, 20), xview='off1', yview='slice', tr='pre', bias=False),   # tile 2x8x16 mw 16 cc 8, 17 chunks, lds 52736
    Case('f_m4n2_x1', dict(path='generic', msub=4, nsub=2, xstage=1, forced=0, splits=17, vec_store=1),
         cin=130, cout=24, k=(4, 4, 4), pad=(1, 1, 3), odims=(5, 5, 20), xview='slice', yview='slice', tr='pre', bias=False),   # tile 2x8x16 mw 16 cc 4, 33 chunks, lds 52224
    Case('f_m4n2_x2', dict(path='generic', msub=4, nsub=2, xstage=2, forced=0, splits=17, vec_store=1),
         cin=130, cout=24, k=(3, 3, 3), pad=(1, 1, 3), odims=(5, 5, 20), xview='s2co', yview='slice', tr='pre', bias=False),   # tile 2x8x16 mw 16 cc 4, 33 chunks, lds 28672
    Case('f_m8n1_x0', dict(path='generic', msub=8, nsub=1, xstage=0, forced=0, splits=9, vec_store=0),
         cin=66, k=(2, 2, 2), odims=(5, 12, 5), xview='off1', yview='co', tr='post'),   # tile 8x8x8 mw 4 cc 4, 17 chunks, lds 15872
    Case('f_m8n1_x1', dict(path='generic', msub=8, nsub=1, xstage=1, forced=0, splits=9, vec_store=1),
         B=2, cin=130, cout=64, k=(2, 2, 2), odims=(5, 5, 12), yview='co', tr='post'),   # tile 4x8x16 mw 8 cc 8, 17 chunks, lds 35328
    Case('f_m8n1_x2', dict(path='generic', msub=8, nsub=1, xstage=2, forced=0, splits=17, vec_store=1),
         B=2, cin=130, k=(2, 2, 2), odims=(5, 5, 20), xview='s2', yview='co', tr='post'),   # tile 2x8x32 mw 16 cc 4, 33 chunks, lds 18944
    # ---- one row per instantiated weight-gradient kernel: (RSUB, NSUB) x staging (x scalars | x float4, dy scalars |
    # x float4, dy float4 | x float4, dy position pairs)
    Case('w_r1n1_x0d0', dict(path='generic', msub=1, nsub=1, xstage=0, dystage=0, splits=8, balanced=0),
         cin=66, odims=(5, 3, 20), op='wgrad', xview='off1', tr='shift'),   # tile 4x2x16 mw 0 cc 64, 8 chunks, lds 43008
    Case('w_r1n1_x1d0', dict(path='generic', msub=1, nsub=1, xstage=1, dystage=0, splits=8, balanced=0),
         cin=66, odims=(3, 5, 20), op='wgrad', yview='off1', tr='shift'),   # tile 2x4x16 mw 0 cc 64, 8 chunks, lds 46848
    Case('w_r1n1_x1d1', dict(path='generic', msub=1, nsub=1, xstage=1, dystage=1, splits=8, balanced=0),
         cin=66, odims=(3, 5, 20), op='wgrad', tr='shift'),   # tile 2x4x16 mw 0 cc 64, 8 chunks, lds 46848
    Case('w_r1n1_x1d2', dict(path='generic', msub=1, nsub=1, xstage=1, dystage=2, splits=8, balanced=0),
         cin=66, odims=(3, 5, 20), op='wgrad', yview='co', tr='shift'),   # tile 2x4x16 mw 0 cc 64, 8 chunks, lds 46848
    Case('w_r1n2_x0d0', dict(path='generic', msub=1, nsub=2, xstage=0, dystage=0, splits=8, balanced=0),
         cin=66, cout=24, pad=(0, 0, 1), odims=(5, 3, 20), op='wgrad', xview='sb2', tr='pre', accumulate=True),   # tile 4x2x16 mw 0 cc 64, 8 chunks, lds 51456
    Case('w_r1n2_x1d0', dict(path='generic', msub=1, nsub=2, xstage=1, dystage=0, splits=8, balanced=0),
         cin=66, cout=24, pad=(0, 0, 1), odims=(5, 3, 20), op='wgrad', xview='slice', yview='off1', tr='pre', accumulate=True),   # tile 3x2x16 mw 0 cc 64, 8 chunks, lds 51200
    Case('w_r1n2_x1d1', dict(path='generic', msub=1, nsub=2, xstage=1, dystage=1, splits=8, balanced=0),
         cin=66, cout=24, pad=(0, 0, 1), odims=(5, 3, 20), op='wgrad', xview='slice', tr='pre', accumulate=True),   # tile 3x2x16 mw 0 cc 64, 8 chunks, lds 51200
    Case('w_r1n2_x1d2', dict(path='generic', msub=1, nsub=2, xstage=1, dystage=2, splits=8, balanced=0),
         cin=66, cout=24, pad=(0, 0, 1), odims=(5, 3, 20), op='wgrad', xview='slice', yview='co', tr='pre', accumulate=True),   # tile 3x2x16 mw 0 cc 64, 8 chunks, lds 51200
    Case('w_r1n4_x0d0', dict(path='generic', msub=1, nsub=4, xstage=0, dystage=0, splits=8, balanced=0),
         cin=3, cout=64, k=(3, 3, 3), pad=(1, 1, 2), odims=(5, 3, 20), op='wgrad', xview='s2', tr='post', accumulate=True),   # tile 4x2x16 mw 0 cc 2, 8 chunks, lds 38792
    Case('w_r1n4_x1d0', dict(path='generic', msub=1, nsub=4, xstage=1, dystage=0, splits=8, balanced=0),
         cin=3, cout=64, k=(2, 2, 2), pad=(0, 0, 2), odims=(5, 3, 20), op='wgrad', yview='off1', tr='post', accumulate=True),   # tile 4x2x16 mw 0 cc 3, 8 chunks, lds 38976
    Case('w_r1n4_x1d1', dict(path='generic', msub=1, nsub=4, xstage=1, dystage=1, splits=8, balanced=0),
         cin=3, cout=64, k=(3, 3, 3), pad=(1, 1, 2), odims=(5, 3, 20), op='wgrad', tr='post', accumulate=True),   # tile 4x2x16 mw 0 cc 2, 8 chunks, lds 39296
    Case('w_r1n4_x1d2', dict(path='generic', msub=1, nsub=4, xstage=1, dystage=2, splits=8, balanced=0),
         cin=3, cout=64, k=(2, 2, 2), pad=(0, 0, 2), odims=(3, 3, 20), op='wgrad', yview='co', tr='post', accumulate=True),   # tile 2x2x16 mw 0 cc 3, 8 chunks, lds 21440
    Case('w_r2n1_x0d0', dict(path='generic', msub=2, nsub=1, xstage=0, dystage=0, splits=8, balanced=0),
         cin=3, k=(4, 4, 4), pad=(1, 1, 3), odims=(5, 12, 20), op='wgrad', xview='off1', tr='both'),   # tile 4x8x16 mw 0 cc 2, 8 chunks, lds 46272
    Case('w_r2n1_x1d0', dict(path='generic', msub=2, nsub=1, xstage=1, dystage=0, splits=8, balanced=0),
         cin=3, k=(3, 3, 3), pad=(1, 1, 3), odims=(5, 12, 20), op='wgrad', xview='slice', yview='off1', tr='both'),   # tile 4x8x16 mw 0 cc 3, 8 chunks, lds 48960
    Case('w_r2n1_x1d1', dict(path='generic', msub=2, nsub=1, xstage=1, dystage=1, splits=8, balanced=0),
         cin=3, k=(4, 4, 4), pad=(1, 1, 3), odims=(5, 12, 20), op='wgrad', xview='slice', tr='both'),   # tile 4x8x16 mw 0 cc 2, 8 chunks, lds 46976
    Case('w_r2n1_x1d2', dict(path='generic', msub=2, nsub=1, xstage=1, dystage=2, splits=8, balanced=0),
         cin=3, k=(4, 4, 4), pad=(1, 1, 3), odims=(5, 5, 20), op='wgrad', xview='slice', yview='co', tr='both'),   # tile 4x4x16 mw 0 cc 2, 8 chunks, lds 26240
    Case('w_r2n2_x0d0', dict(path='generic', msub=2, nsub=2, xstage=0, dystage=0, splits=8, balanced=0),
         cin=3, cout=24, k=(4, 4, 4), pad=(1, 1, 0), odims=(5, 5, 20), op='wgrad', xview='off1', tr='scale'),   # tile 4x4x16 mw 0 cc 2, 8 chunks, lds 42272
    Case('w_r2n2_x1d0', dict(path='generic', msub=2, nsub=2, xstage=1, dystage=0, splits=8, balanced=0),
         cin=3, cout=24, k=(3, 3, 3), pad=(1, 1, 0), odims=(5, 5, 20), op='wgrad', yview='off1', tr='scale'),   # tile 4x4x16 mw 0 cc 3, 8 chunks, lds 43456
    Case('w_r2n2_x1d1', dict(path='generic', msub=2, nsub=2, xstage=1, dystage=1, splits=8, balanced=0),
         cin=3, cout=24, k=(4, 4, 4), pad=(1, 1, 0), odims=(5, 5, 20), op='wgrad', tr='scale'),   # tile 4x4x16 mw 0 cc 2, 8 chunks, lds 42880
    Case('w_r2n2_x1d2', dict(path='generic', msub=2, nsub=2, xstage=1, dystage=2, splits=8, balanced=0),
         cin=3, cout=24, k=(4, 4, 4), pad=(1, 1, 0), odims=(3, 5, 20), op='wgrad', yview='co', tr='scale'),   # tile 2x4x16 mw 0 cc 2, 8 chunks, lds 24192
    Case('w_r2n4_x0d0', dict(path='generic', msub=2, nsub=4, xstage=0, dystage=0, splits=8, balanced=0),
         cin=3, cout=64, k=(4, 4, 4), pad=(1, 1, 1), odims=(5, 3, 20), op='wgrad', xview='sb2', accumulate=True),   # tile 4x2x16 mw 0 cc 2, 8 chunks, lds 40656
    Case('w_r2n4_x1d0', dict(path='generic', msub=2, nsub=4, xstage=1, dystage=0, splits=4, balanced=0),
         cin=3, cout=64, k=(4, 4, 4), pad=(1, 1, 1), odims=(5, 1, 20), op='wgrad', xview='slice', yview='off1', accumulate=True),   # tile 4x1x16 mw 0 cc 2, 4 chunks, lds 24448
    Case('w_r2n4_x1d1', dict(path='generic', msub=2, nsub=4, xstage=1, dystage=1, splits=8, balanced=0),
         cin=3, cout=64, k=(4, 4, 4), pad=(1, 1, 1), odims=(5, 3, 20), op='wgrad', xview='slice', accumulate=True),   # tile 4x2x16 mw 0 cc 2, 8 chunks, lds 42112
    Case('w_r2n4_x1d2', dict(path='generic', msub=2, nsub=4, xstage=1, dystage=2, splits=8, balanced=0),
         cin=3, cout=64, k=(4, 4, 4), pad=(1, 1, 1), odims=(3, 3, 20), op='wgrad', xview='slice', yview='co', accumulate=True),   # tile 2x2x16 mw 0 cc 2, 8 chunks, lds 23936
    Case('w_r4n1_x0d0', dict(path='generic', msub=4, nsub=1, xstage=0, dystage=0, splits=8, balanced=0),
         cin=3, k=(5, 5, 5), pad=(2, 2, 2), odims=(5, 12, 20), op='wgrad', xview='s2', tr='shift', accumulate=True),   # tile 4x8x16 mw 0 cc 2, 8 chunks, lds 49928
    Case('w_r4n1_x1d0', dict(path='generic', msub=4, nsub=1, xstage=1, dystage=0, splits=8, balanced=0),
         cin=66, k=(2, 2, 2), pad=(0, 0, 2), odims=(5, 3, 20), op='wgrad', yview='off1', tr='shift', accumulate=True),   # tile 4x2x16 mw 0 cc 30, 8 chunks, lds 46464
    Case('w_r4n1_x1d1', dict(path='generic', msub=4, nsub=1, xstage=1, dystage=1, splits=8, balanced=0),
         cin=66, k=(2, 2, 2), pad=(0, 0, 2), odims=(5, 3, 20), op='wgrad', tr='shift', accumulate=True),   # tile 4x2x16 mw 0 cc 30, 8 chunks, lds 46464
    Case('w_r4n1_x1d2', dict(path='generic', msub=4, nsub=1, xstage=1, dystage=2, splits=8, balanced=0),
         cin=66, k=(2, 2, 2), pad=(0, 0, 2), odims=(5, 3, 20), op='wgrad', yview='co', tr='shift', accumulate=True),   # tile 4x2x16 mw 0 cc 30, 8 chunks, lds 46464
    Case('w_r4n2_x0d0', dict(path='generic', msub=4, nsub=2, xstage=0, dystage=0, splits=8, balanced=0),
         cin=3, cout=24, k=(5, 5, 5), pad=(2, 2, 3), odims=(5, 5, 20), op='wgrad', xview='off1', tr='pre'),   # tile 4x4x16 mw 0 cc 2, 8 chunks, lds 45064
    Case('w_r4n2_x1d0', dict(path='generic', msub=4, nsub=2, xstage=1, dystage=0, splits=8, balanced=0),
         cin=3, cout=24, k=(5, 5, 5), pad=(2, 2, 3), odims=(5, 5, 20), op='wgrad', xview='slice', yview='off1', tr='pre'),   # tile 4x4x16 mw 0 cc 2, 8 chunks, lds 47232
    Case('w_r4n2_x1d1', dict(path='generic', msub=4, nsub=2, xstage=1, dystage=1, splits=8, balanced=0),
         cin=3, cout=24, k=(5, 5, 5), pad=(2, 2, 3), odims=(5, 5, 20), op='wgrad', xview='slice', tr='pre'),   # tile 4x4x16 mw 0 cc 2, 8 chunks, lds 47232
    Case('w_r4n2_x1d2', dict(path='generic', msub=4, nsub=2, xstage=1, dystage=2, splits=8, balanced=0),
         cin=3, cout=24, k=(5, 5, 5), pad=(2, 2, 3), odims=(3, 5, 20), op='wgrad', xview='slice', yview='co', tr='pre'),   # tile 2x4x16 mw 0 cc 2, 8 chunks, lds 27776
    Case('w_r8n1_x0d0', dict(path='generic', msub=8, nsub=1, xstage=0, dystage=0, splits=8, balanced=0),
         cin=66, k=(5, 5, 5), pad=(2, 2, 0), odims=(5, 12, 20), op='wgrad', xview='off1', tr='post'),   # tile 4x8x16 mw 0 cc 4, 8 chunks, lds 65296
    Case('w_r8n1_x1d0', dict(path='generic', msub=8, nsub=1, xstage=1, dystage=0, splits=8, balanced=0),
         cin=66, k=(3, 3, 3), pad=(1, 1, 0), odims=(3, 5, 20), op='wgrad', yview='off1', tr='post'),   # tile 2x4x16 mw 0 cc 18, 8 chunks, lds 45696
    Case('w_r8n1_x1d1', dict(path='generic', msub=8, nsub=1, xstage=1, dystage=1, splits=8, balanced=0),
         cin=66, k=(4, 4, 4), pad=(1, 1, 0), odims=(5, 8, 20), op='wgrad', tr='post'),   # tile 3x6x16 mw 0 cc 8, 8 chunks, lds 55552
    Case('w_r8n1_x1d2', dict(path='generic', msub=8, nsub=1, xstage=1, dystage=2, splits=8, balanced=0),
         cin=66, k=(3, 3, 3), pad=(1, 1, 0), odims=(3, 5, 20), op='wgrad', yview='co', tr='post'),   # tile 2x4x16 mw 0 cc 18, 8 chunks, lds 45696
    # ---- edges
    Case('e_w1_cin1', dict(path='generic', msub=1, nsub=1, xstage=0, forced=0, splits=1, vec_store=0),
         B=2, k=(3, 3, 3), pad=(1, 1, 1), odims=(3, 5, 1), tr='shift'),   # tile 4x16x1 mw 1 cc 4, 1 chunks, lds 13824
    Case('e_w2_cin3', dict(path='generic', msub=1, nsub=1, xstage=0, forced=0, splits=1, vec_store=0),
         B=2, cin=3, cout=24, k=(3, 3, 3), pad=(1, 1, 1), odims=(3, 5, 2), yview='slice', tr='both'),   # tile 4x8x2 mw 2 cc 4, 1 chunks, lds 12288
    Case('e_w3_cin3', dict(path='generic', msub=1, nsub=1, xstage=0, forced=0, splits=1, vec_store=0),
         cin=3, cout=40, k=(3, 3, 3), pad=(1, 1, 2), odims=(5, 5, 3), tr='pre', accumulate=True),   # tile 2x8x4 mw 2 cc 4, 1 chunks, lds 12288
    Case('e_cin3_x1', dict(path='generic', msub=1, nsub=1, xstage=1, forced=0, splits=1, vec_store=1),
         B=2, cin=3, k=(3, 3, 3), pad=(1, 1, 1), odims=(3, 5, 8), tr='post'),   # tile 4x2x8 mw 8 cc 4, 1 chunks, lds 14848
    Case('e_cin2_x2', dict(path='generic', msub=1, nsub=1, xstage=2, forced=0, splits=1, vec_store=1),
         B=2, cin=2, k=(3, 3, 3), pad=(1, 1, 1), odims=(3, 5, 8), xview='s2co', tr='shift'),   # tile 4x2x8 mw 8 cc 4, 1 chunks, lds 13312
    Case('e_1x1x1_cin1', dict(path='generic', msub=1, nsub=1, xstage=0, forced=0, splits=1, vec_store=0),
         ),   # tile 1x16x4 mw 1 cc 4, 1 chunks, lds 3072
    Case('e_s2_oddw', dict(path='generic', msub=1, nsub=1, xstage=0, forced=0, splits=1, vec_store=0),
         B=2, cin=16, cout=24, k=(1, 3, 3), pad=(0, 1, 1), odims=(1, 6, 5), xview='s2', tr='shift'),   # tile 1x8x8 mw 4 cc 16, 1 chunks, lds 17920
    Case('e_s2co_oddk', dict(path='generic', msub=1, nsub=1, xstage=2, forced=0, splits=1, vec_store=0),
         B=2, cin=16, cout=24, k=(1, 3, 3), pad=(0, 1, 1), odims=(1, 6, 6), xview='s2co', tr='both'),   # tile 1x8x8 mw 4 cc 16, 1 chunks, lds 19968
    Case('e_s2d_in', dict(path='generic', msub=1, nsub=1, xstage=2, forced=0, splits=1, vec_store=0),
         B=2, cin=16, cout=24, k=(2, 2, 2), pad=(1, 1, 1), odims=(3, 5, 6), xview='s2d', yview='slice', tr='pre'),   # tile 1x8x8 mw 4 cc 16, 1 chunks, lds 24064
    Case('e_misaligned_k3', dict(path='generic', msub=2, nsub=1, xstage=0, forced=0, splits=1, vec_store=1),
         B=2, cin=16, cout=128, k=(3, 3, 3), pad=(1, 1, 1), odims=(8, 16, 12), xview='off1', tr='shift'),   # tile 4x4x8 mw 8 cc 16, 1 chunks, lds 52736
    Case('e_c130_n16', dict(path='generic', msub=8, nsub=1, xstage=1, forced=0, splits=17, vec_store=1),
         B=2, cin=130, k=(3, 3, 3), pad=(1, 1, 1), odims=(8, 16, 12), tr='both'),   # tile 4x8x16 mw 8 cc 4, 33 chunks, lds 31744
    Case('e_c130_2d', dict(path='generic', msub=2, nsub=4, xstage=1, forced=0, splits=9, vec_store=1),
         B=2, cin=130, cout=128, k=(1, 3, 3), pad=(0, 1, 1), odims=(1, 16, 20), tr='post'),   # tile 1x4x32 mw 16 cc 8, 17 chunks, lds 28160
    Case('e_c130_mw4', dict(path='generic', msub=4, nsub=2, xstage=1, forced=0, splits=17, vec_store=1),
         B=2, cin=130, cout=128, k=(3, 3, 3), pad=(1, 1, 1), odims=(8, 8, 4), tr='scale'),   # tile 8x8x4 mw 4 cc 4, 33 chunks, lds 34816
    Case('e_forced', dict(path='generic', msub=4, nsub=1, xstage=0, forced=1, splits=1, vec_store=0),
         B=2, cin=3, k=(4, 4, 4), pad=(1, 1, 1), odims=(8, 3, 1), xdims=(8, 3, 2), xview='s2', tr='shift'),   # tile 8x16x2 mw 1 cc 4, 1 chunks, lds 35328
    Case('e_forced_co', dict(path='generic', msub=4, nsub=1, xstage=0, forced=1, splits=1, vec_store=0),
         cin=2, k=(4, 4, 4), pad=(1, 1, 2), odims=(5, 2, 1), xdims=(5, 2, 2), xview='s2co', tr='both', accumulate=True),   # tile 8x16x2 mw 1 cc 4, 1 chunks, lds 35328
    Case('s_given1_b', dict(path='generic', msub=1, nsub=1, xstage=1, forced=0, splits=1, vec_store=1),
         B=2, cin=66, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 3, 12), tr='shift', splits=1),   # tile 1x4x16 mw 8 cc 16, 5 chunks, lds 56832
    Case('s_5chunks_4asked_b', dict(path='generic', msub=1, nsub=1, xstage=1, forced=0, splits=3, vec_store=1),
         B=2, cin=66, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 3, 12), tr='shift', splits=4),   # tile 1x4x16 mw 8 cc 16, 5 chunks, lds 56832
    Case('s_4chunks_3asked_b', dict(path='generic', msub=1, nsub=1, xstage=1, forced=0, splits=2, vec_store=1),
         B=2, cin=52, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 3, 12), tr='shift', splits=3),   # tile 1x4x16 mw 8 cc 16, 4 chunks, lds 56832
    Case('s_more_than_chunks_b', dict(path='generic', msub=1, nsub=1, xstage=1, forced=0, splits=5, vec_store=1),
         B=2, cin=66, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 3, 12), tr='shift', splits=64),   # tile 1x4x16 mw 8 cc 16, 5 chunks, lds 56832
    Case('s_auto_b', dict(path='generic', msub=1, nsub=2, xstage=1, forced=0, splits=5, vec_store=1),
         B=2, cin=66, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 3, 12), tr='shift'),   # tile 1x4x16 mw 8 cc 8, 9 chunks, lds 43520
    Case('s_auto_x0_b', dict(path='generic', msub=1, nsub=2, xstage=0, forced=0, splits=5, vec_store=1),
         B=2, cin=66, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 3, 12), xview='off1', yview='slice', tr='shift'),   # tile 2x4x8 mw 8 cc 8, 9 chunks, lds 37376
    Case('s_auto_x2_b', dict(path='generic', msub=4, nsub=1, xstage=2, forced=0, splits=9, vec_store=1),
         B=2, cin=66, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 3, 12), xview='s2co', yview='co', tr='shift'),   # tile 4x4x16 mw 8 cc 4, 17 chunks, lds 19968
    Case('s_given1_a', dict(path='generic', msub=1, nsub=1, xstage=1, forced=0, splits=1, vec_store=1),
         B=2, cin=66, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 3, 12), tr='shift', bias=False, accumulate=True, splits=1),   # tile 1x4x16 mw 8 cc 16, 5 chunks, lds 56832
    Case('s_5chunks_4asked_a', dict(path='generic', msub=1, nsub=1, xstage=1, forced=0, splits=3, vec_store=1),
         B=2, cin=66, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 3, 12), tr='shift', bias=False, accumulate=True, splits=4),   # tile 1x4x16 mw 8 cc 16, 5 chunks, lds 56832
    Case('s_4chunks_3asked_a', dict(path='generic', msub=1, nsub=1, xstage=1, forced=0, splits=2, vec_store=1),
         B=2, cin=52, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 3, 12), tr='shift', bias=False, accumulate=True, splits=3),   # tile 1x4x16 mw 8 cc 16, 4 chunks, lds 56832
    Case('s_more_than_chunks_a', dict(path='generic', msub=1, nsub=1, xstage=1, forced=0, splits=5, vec_store=1),
         B=2, cin=66, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 3, 12), tr='shift', bias=False, accumulate=True, splits=64),   # tile 1x4x16 mw 8 cc 16, 5 chunks, lds 56832
    Case('s_auto_a', dict(path='generic', msub=1, nsub=2, xstage=1, forced=0, splits=5, vec_store=1),
         B=2, cin=66, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 3, 12), tr='shift', bias=False, accumulate=True),   # tile 1x4x16 mw 8 cc 8, 9 chunks, lds 43520
    Case('s_auto_x0_a', dict(path='generic', msub=1, nsub=2, xstage=0, forced=0, splits=5, vec_store=1),
         B=2, cin=66, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 3, 12), xview='off1', yview='slice', tr='shift', bias=False, accumulate=True),   # tile 2x4x8 mw 8 cc 8, 9 chunks, lds 37376
    Case('s_auto_x2_a', dict(path='generic', msub=4, nsub=1, xstage=2, forced=0, splits=9, vec_store=1),
         B=2, cin=66, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 3, 12), xview='s2co', yview='co', tr='shift', bias=False, accumulate=True),   # tile 4x4x16 mw 8 cc 4, 17 chunks, lds 19968
    Case('s_given1_ba', dict(path='generic', msub=1, nsub=1, xstage=1, forced=0, splits=1, vec_store=1),
         B=2, cin=66, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 3, 12), tr='shift', accumulate=True, splits=1),   # tile 1x4x16 mw 8 cc 16, 5 chunks, lds 56832
    Case('s_5chunks_4asked_ba', dict(path='generic', msub=1, nsub=1, xstage=1, forced=0, splits=3, vec_store=1),
         B=2, cin=66, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 3, 12), tr='shift', accumulate=True, splits=4),   # tile 1x4x16 mw 8 cc 16, 5 chunks, lds 56832
    Case('s_4chunks_3asked_ba', dict(path='generic', msub=1, nsub=1, xstage=1, forced=0, splits=2, vec_store=1),
         B=2, cin=52, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 3, 12), tr='shift', accumulate=True, splits=3),   # tile 1x4x16 mw 8 cc 16, 4 chunks, lds 56832
    Case('s_more_than_chunks_ba', dict(path='generic', msub=1, nsub=1, xstage=1, forced=0, splits=5, vec_store=1),
         B=2, cin=66, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 3, 12), tr='shift', accumulate=True, splits=64),   # tile 1x4x16 mw 8 cc 16, 5 chunks, lds 56832
    Case('s_auto_ba', dict(path='generic', msub=1, nsub=2, xstage=1, forced=0, splits=5, vec_store=1),
         B=2, cin=66, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 3, 12), tr='shift', accumulate=True),   # tile 1x4x16 mw 8 cc 8, 9 chunks, lds 43520
    Case('s_auto_x0_ba', dict(path='generic', msub=1, nsub=2, xstage=0, forced=0, splits=5, vec_store=1),
         B=2, cin=66, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 3, 12), xview='off1', yview='slice', tr='shift', accumulate=True),   # tile 2x4x8 mw 8 cc 8, 9 chunks, lds 37376
    Case('s_auto_x2_ba', dict(path='generic', msub=4, nsub=1, xstage=2, forced=0, splits=9, vec_store=1),
         B=2, cin=66, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 3, 12), xview='s2co', yview='co', tr='shift', accumulate=True),   # tile 4x4x16 mw 8 cc 4, 17 chunks, lds 19968
    Case('p_c256_s64', dict(path='pointwise', splits=2, vec_store=1),
         B=2, cin=256, cout=40, odims=(1, 8, 8), tr='shift'),   # tile 1x1x64 mw 16 cc 64, 8 chunks, lds 33792
    Case('p_c260_s68', dict(path='pointwise', splits=2, vec_store=1),
         B=2, cin=260, cout=40, odims=(1, 4, 17), tr='both', accumulate=True),   # tile 1x1x64 mw 16 cc 64, 9 chunks, lds 34048
    Case('p_c260_s4_notr', dict(path='pointwise', splits=2, vec_store=1),
         cin=260, cout=40, odims=(1, 2, 2), bias=False),   # tile 1x1x64 mw 16 cc 64, 9 chunks, lds 32768
    Case('p_c2048_s4', dict(path='pointwise', splits=16, vec_store=1),
         cin=2048, cout=64, odims=(1, 2, 2), tr='pre'),   # tile 1x1x64 mw 16 cc 64, 64 chunks, lds 33792
    Case('p_c2052_notr', dict(path='pointwise', splits=13, vec_store=1),
         cin=2052, cout=64, odims=(1, 2, 2)),   # tile 1x1x64 mw 16 cc 64, 65 chunks, lds 32768
    Case('p_c2052_tr_generic', dict(path='generic', msub=1, nsub=1, xstage=0, forced=0, splits=17, vec_store=0),
         cin=2052, cout=64, odims=(1, 2, 2), tr='shift'),   # tile 1x8x8 mw 2 cc 64, 33 chunks, lds 26112
    Case('p_blocks255', dict(path='pointwise', splits=2, vec_store=1),
         cin=256, cout=544, odims=(1, 30, 32), tr='post'),   # tile 1x1x64 mw 16 cc 64, 8 chunks, lds 33792
    Case('p_blocks256', dict(path='pointwise', splits=1, vec_store=1),
         cin=256, cout=512, odims=(1, 32, 32), tr='post'),   # tile 1x1x64 mw 16 cc 64, 8 chunks, lds 34816
    Case('p_given1', dict(path='pointwise', splits=1, vec_store=1),
         B=2, cin=260, cout=40, odims=(1, 8, 8), tr='shift', splits=1),   # tile 1x1x64 mw 16 cc 64, 9 chunks, lds 35328
    Case('p_cl', dict(path='pointwise', splits=1, vec_store=0),
         B=2, cin=96, cout=20, odims=(1, 8, 8), yview='cl', tr='shift'),   # tile 1x1x64 mw 16 cc 64, 3 chunks, lds 33792
    Case('p_cl_split', dict(path='pointwise', splits=2, vec_store=1),
         B=2, cin=260, cout=12, odims=(1, 8, 8), yview='cl', tr='scale', accumulate=True),   # tile 1x1x64 mw 16 cc 64, 9 chunks, lds 34048
    Case('p_slice', dict(path='pointwise', splits=1, vec_store=1),
         B=2, cin=64, cout=40, odims=(1, 8, 8), xview='slice', yview='slice'),   # tile 1x1x64 mw 16 cc 64, 2 chunks, lds 32768
    Case('d_cols_1024', dict(path='dense_cols', splits=1, vec_store=0),
         cin=67, cout=1024, tr='pre'),   # tile 0x0x0 mw 0 cc 0, 1 chunks, lds 6412
    Case('d_cols_1030_b3', dict(path='dense_cols', splits=1, vec_store=0),
         B=3, cin=67, cout=1030, tr='shift', accumulate=True),   # tile 0x0x0 mw 0 cc 0, 1 chunks, lds 6948
    Case('d_cols_b8_c2048', dict(path='dense_cols', splits=1, vec_store=0),
         B=8, cin=2048, cout=1024, bias=False),   # tile 0x0x0 mw 0 cc 0, 1 chunks, lds 71680
    Case('d_cols_c2049_leaves', dict(path='generic', msub=1, nsub=4, xstage=0, forced=0, splits=11, vec_store=0),
         B=2, cin=2049, cout=1024),   # tile 1x16x4 mw 1 cc 64, 33 chunks, lds 42496
    Case('d_b9_generic', dict(path='generic', msub=1, nsub=4, xstage=0, forced=0, splits=1, vec_store=0),
         B=9, cin=67, cout=1024, tr='shift'),   # tile 1x16x4 mw 1 cc 64, 2 chunks, lds 42496
    Case('d_rows_1024', dict(path='dense_rows', splits=1, vec_store=0),
         B=2, cin=1024, cout=40),   # tile 0x0x0 mw 0 cc 0, 4 chunks, lds 128
    Case('d_rows_4096', dict(path='dense_rows', splits=2, vec_store=0),
         B=2, cin=4096, cout=40, accumulate=True),   # tile 0x0x0 mw 0 cc 0, 16 chunks, lds 128
    Case('d_rows_4100', dict(path='dense_rows', splits=2, vec_store=0),
         B=3, cin=4100, cout=67),   # tile 0x0x0 mw 0 cc 0, 17 chunks, lds 128
    Case('d_rows_4100_nc', dict(path='dense_rows', splits=1, vec_store=0),
         B=3, cin=4100, cout=67, yview='nc'),   # tile 0x0x0 mw 0 cc 0, 17 chunks, lds 128
    Case('d_rows_4096_nc_acc', dict(path='dense_rows', splits=1, vec_store=0),
         B=2, cin=4096, cout=40, yview='nc', bias=False, accumulate=True),   # tile 0x0x0 mw 0 cc 0, 16 chunks, lds 128
    Case('d_rows_scale_leaves', dict(path='generic', msub=1, nsub=1, xstage=0, forced=0, splits=16, vec_store=0),
         B=2, cin=1024, cout=40, tr='scale'),   # tile 1x16x4 mw 1 cc 64, 16 chunks, lds 26112
    Case('d_wgrad_1024', dict(path='dense_wgrad', splits=1, vec_store=0),
         B=4, cin=67, cout=1024, op='wgrad'),   # tile 0x0x0 mw 0 cc 0, 1 chunks, lds 0
    Case('d_wgrad_1030_tr', dict(path='dense_wgrad', splits=1, vec_store=0),
         B=3, cin=67, cout=1030, op='wgrad', tr='pre', accumulate=True),   # tile 0x0x0 mw 0 cc 0, 1 chunks, lds 0
    Case('d_wgrad_1024_tr', dict(path='dense_wgrad', splits=1, vec_store=0),
         B=8, cin=5, cout=1024, op='wgrad', tr='both'),   # tile 0x0x0 mw 0 cc 0, 1 chunks, lds 0
    Case('d_wgrad_1030', dict(path='dense_wgrad', splits=1, vec_store=0),
         cin=5, cout=1030, op='wgrad', accumulate=True),   # tile 0x0x0 mw 0 cc 0, 1 chunks, lds 0
    Case('w_det', dict(path='generic', msub=4, nsub=2, xstage=1, dystage=1, splits=1, balanced=0),
         B=2, cin=16, cout=24, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 5, 12), op='wgrad', tr='shift', deterministic=True),   # tile 4x5x12 mw 0 cc 9, 4 chunks, lds 63296
    Case('w_convT_balanced', dict(path='generic', msub=1, nsub=4, xstage=1, dystage=2, splits=4, balanced=1),
         B=2, cin=6, cout=64, k=(3, 3, 3), pad=(1, 1, 1), odims=(3, 4, 8), op='wgrad', geom='convT', yview='s2d', tr='both', boxes='geom'),   # tile 2x4x8 mw 0 cc 6, 4 chunks, lds 23936
    Case('w_convT_balanced_acc', dict(path='generic', msub=2, nsub=4, xstage=1, dystage=2, splits=1, balanced=1),
         cin=16, cout=64, k=(3, 3, 3), pad=(1, 1, 1), odims=(2, 4, 8), op='wgrad', geom='convT', yview='s2d', tr='pre', accumulate=True, boxes='geom'),   # tile 2x4x8 mw 0 cc 16, 1 chunks, lds 32256
    Case('w_boxes_ignored', dict(path='generic', msub=4, nsub=2, xstage=1, dystage=1, splits=4, balanced=0),
         B=2, cin=16, cout=40, k=(3, 3, 3), pad=(1, 1, 1), odims=(5, 5, 12), op='wgrad', tr='shift', boxes='odd'),   # tile 4x5x12 mw 0 cc 9, 4 chunks, lds 63296
    Case('w_t512', dict(path='generic', msub=8, nsub=1, xstage=1, dystage=1, splits=2, balanced=0),
         B=2, cin=2, k=(8, 8, 8), pad=(3, 3, 3), odims=(2, 3, 4), op='wgrad', tr='shift'),   # tile 2x3x4 mw 0 cc 1, 2 chunks, lds 7744
    Case('w_w1', dict(path='generic', msub=2, nsub=1, xstage=0, dystage=0, splits=2, balanced=0),
         B=2, cin=3, k=(3, 3, 3), pad=(1, 1, 1), odims=(3, 5, 1), op='wgrad', tr='shift'),   # tile 3x5x4 mw 0 cc 3, 2 chunks, lds 8164
    Case('w_w3_x_s2', dict(path='generic', msub=2, nsub=2, xstage=0, dystage=0, splits=2, balanced=0),
         B=2, cin=16, cout=24, k=(1, 3, 3), pad=(0, 1, 1), odims=(1, 6, 3), op='wgrad', xview='s2', tr='post', accumulate=True),   # tile 1x6x4 mw 0 cc 14, 2 chunks, lds 7864
    Case('w_cin130', dict(path='generic', msub=4, nsub=2, xstage=1, dystage=1, splits=2, balanced=0),
         B=2, cin=130, cout=120, k=(3, 3, 3), pad=(1, 1, 1), odims=(3, 5, 12), op='wgrad', tr='both'),   # tile 3x5x12 mw 0 cc 9, 2 chunks, lds 51008
    Case('f_convT_k3', dict(path='generic', msub=1, nsub=1, xstage=1, forced=0, splits=1, vec_store=0),
         B=2, cin=12, cout=5, k=(3, 3, 3), pad=(1, 1, 1), odims=(3, 4, 8), geom='convT', yview='s2d', tr='pre', boxes='geom'),   # tile 2x4x8 mw 8 cc 8, 2 chunks, lds 12800
    # ---- data gradients: the same entry with the data-gradient weights, against autograd
    Case('g_dgrad_k3', dict(path='generic', msub=1, nsub=2, xstage=1, forced=0, splits=3, vec_store=1),
         B=2, cin=40, cout=24, k=(3, 3, 3), pad=(1, 1, 1), odims=(3, 5, 12), geom='dgrad', yview='slice', bias=False, accumulate=True),   # tile 2x2x16 mw 8 cc 8, 5 chunks, lds 42496
    Case('g_dgrad_2d_x0', dict(path='generic', msub=1, nsub=4, xstage=0, forced=0, splits=9, vec_store=1),
         B=2, cin=130, cout=64, k=(1, 3, 3), pad=(0, 1, 1), odims=(1, 6, 8), geom='dgrad', xview='off1', bias=False),   # tile 1x8x8 mw 8 cc 8, 17 chunks, lds 24064
    Case('g_convT_dgrad', dict(path='generic', msub=1, nsub=1, xstage=2, forced=0, splits=1, vec_store=1),
         B=2, cin=5, cout=12, k=(3, 3, 3), pad=(1, 1, 1), odims=(3, 4, 8), geom='convT_dgrad', xview='s2d', bias=False, accumulate=True, boxes='geom'),   # tile 2x4x8 mw 8 cc 16, 3 chunks, lds 22016
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------------------ views
def _contig(st, off, B, C, D, H, W, sB=None):
  return V.View(st, off, B, C, D, H, W, C * D * H * W if sB is None else sB, D * H * W, H * W, W, 1)


def _sb2(C, S):
  sB = C * S
  while sB % 4 != 2: sB += 1
  return sB


def view_numel(kind, B, C, dims):
  D, H, W = dims
  S = D * H * W
  return {"plain": B * C * S, "slice": B * (C + 5) * S, "off1": B * C * S + 1, "sb2": B * _sb2(C, S),
          "s2": B * C * D * H * (2 * W - W % 2), "s2co": B * C * S, "s2d": B * C * S, "co": B * C * S,
          "cl": B * S * (C + 3), "nc": B * 2 * C * S}[kind]


def make_view(kind, st, B, C, dims):
  """The logical [B, C, D, H, W] view of kind `kind` over the flat storage st (view_numel elements)."""
  D, H, W = dims
  S = D * H * W
  if kind == "plain": return _contig(st, 0, B, C, D, H, W)
  if kind == "slice": return _contig(st, 0, B, C + 5, D, H, W).channels(2, 2 + C)       # channels 2 .. 2 + C of a wider buffer
  if kind == "off1": return _contig(st, 1, B, C, D, H, W)                                # base off by 4 bytes
  if kind == "sb2": return _contig(st, 0, B, C, D, H, W, sB=_sb2(C, S))                  # batch stride = 2 mod 4
  if kind == "s2":                                                                       # every second column, no table
    return V.strided_view(_contig(st, 0, B, C, D, H, 2 * W - W % 2), (1, 1, 2))
  if kind == "s2co":                                                                     # ... with a channel table
    assert C % 2 == 0
    return V.space_to_depth_view(_contig(st, 0, B, C // 2, D, H, 2 * W), (1, 1, 2), parity_major=True)
  if kind == "co": return make_view("s2co", st, B, C, dims)
  if kind == "s2d":                                                                      # parity-major space-to-depth
    assert C % 8 == 0
    return V.space_to_depth_view(_contig(st, 0, B, C // 8, 2 * D, 2 * H, 2 * W), (2, 2, 2), parity_major=True)
  if kind == "cl":                                                                       # channel-last, C + 3 channels wide
    Ct = C + 3
    return V.View(st, 0, B, C, D, H, W, S * Ct, 1, H * W * Ct, W * Ct, Ct)
  if kind == "nc":                                                                       # every second channel slot
    return V.View(st, 0, B, C, D, H, W, 2 * C * S, 2 * S, H * W, W, 1)
  raise ValueError(kind)


def inside_mask(kind, B, C, dims):
  """bool [numel]: the elements of the storage that the view addresses."""
  st = t.zeros(view_numel(kind, B, C, dims))
  write_logical(make_view(kind, st, B, C, dims), t.ones(B, C, *dims))
  return st != 0


# ------------------------------------------------------------------------------------------------ inputs
class Built:
  """The seeded CPU tensors of a case (float32) and its geometry."""


def build(c: Case) -> Built:
  b = Built()
  b.case = c
  g = t.Generator().manual_seed(zlib.crc32(c.name.encode()))
  rn = lambda *s: t.randn(*s, generator=g)
  T = c.k[0] * c.k[1] * c.k[2]
  if c.geom == "convT":
    wshape = (c.cin, c.cout) + c.k
    b.geo = G.convt_fwd(wshape, c.pad[0])
    b.ycin, b.ycout = c.cin, 8 * c.cout
  elif c.geom == "dgrad":
    wshape = (c.cin, c.cout) + c.k
    b.geo = G.conv_dgrad(wshape, c.pad)
    b.ycin, b.ycout = c.cin, c.cout
  elif c.geom == "convT_dgrad":          # x = the parity-major view of dy [B, cin, 2D, 2H, 2W]
    wshape = (c.cout, c.cin) + c.k
    b.geo = G.convt_dgrad(wshape, c.pad[0])
    b.ycin, b.ycout = 8 * c.cin, c.cout
  else:
    wshape = (c.cout, c.cin) + c.k
    b.geo = G.conv_fwd(wshape, c.pad)
    b.ycin, b.ycout = c.cin, c.cout
  b.window, b.pad_lo, b.npad = b.geo.window, b.geo.pad_lo, b.geo.npad
  b.w = rn(*wshape) / float(np.sqrt(c.cin * T))
  assert c.op == "fwd" or c.geom in ("conv", "convT")
  b.index = t.as_tensor(b.geo.index).long()
  b.wp = t.where(b.index >= 0, b.w.reshape(-1)[b.index.clamp(min=0)], t.zeros(()))
  b.bias = rn(c.cout) if (c.bias and c.op == "fwd") else None
  b.bp = None
  if b.bias is not None:
    bi = t.as_tensor(G.bias_index(c.cout, 8 if c.geom == "convT" else 1, b.npad, parity_major=c.geom == "convT")).long()
    b.bp = t.where(bi >= 0, b.bias[bi.clamp(min=0)], t.zeros(()))
  b.scale = b.shift = None
  if c.tr:
    b.scale = t.rand(c.cin, generator=g) + 0.5
    # O(1) and mostly positive: a post-ReLU must not silence a whole channel of a small case
    b.shift = t.zeros(c.cin) if c.tr == "scale" else t.randn(c.cin, generator=g) * 0.7 + 0.5
  b.pre, b.post = c.tr in ("pre", "both"), c.tr in ("post", "both")
  b.xs = rn(view_numel(c.xview, c.B, b.ycin, c.xd))
  ny = view_numel(c.yview, c.B, b.ycout, c.odims)
  if c.op == "fwd":
    b.y0 = rn(ny) if c.accumulate else t.full((ny,), SENTINEL)
  else:
    b.dys = rn(ny)
    b.dw0 = rn(b.index.numel()) if c.accumulate else t.full((b.index.numel(),), SENTINEL)
  b.boxes = None
  if c.boxes == "geom":
    b.boxes = (b.geo.n_boxes, b.geo.c_boxes)
  elif c.boxes == "odd":          # three groups over channels they do not divide: the information must be ignored
    b.boxes = (((0, 1, 0, 1, 0, 1),) * 3, ((0, 1, 0, 1, 0, 1),) * 3)
  return b


def xview(b, st): return make_view(b.case.xview, st, b.case.B, b.ycin, b.case.xd)
def yview(b, st): return make_view(b.case.yview, st, b.case.B, b.ycout, b.case.odims)


def transform_of(b, dev=None, cls=None):
  """The Transform of the case on device dev (None when the case has none)."""
  if b.scale is None: return None
  from corenet_amd.backend import Transform
  return (cls or Transform)(b.scale.to(dev) if dev else b.scale, b.shift.to(dev) if dev else b.shift, b.pre, b.post)


# ------------------------------------------------------------------------------------------------ float64 references
def _transformed(b, x):
  if b.scale is None: return x
  sh = [1, -1, 1, 1, 1]
  if b.pre: x = x.relu()
  x = x * b.scale.to(x.dtype).view(sh) + b.shift.to(x.dtype).view(sh)
  if b.post: x = x.relu()
  return x


def _pads(b, x, pad_lo):
  pads = []
  for dim in (2, 1, 0):
    lo = pad_lo[dim]
    pads += [lo, b.case.odims[dim] + b.window[dim] - 1 - lo - x.shape[2 + dim]]
  return pads


def logical_x(b, dtype=t.float64):
  return logical(xview(b, b.xs.to(dtype)))


def ref_fwd_logical(b, dtype=t.float64):
  """The conv part of y (no bias, no accumulation) as torch's own operator computes it, logical [B, ycout, D, H, W]."""
  c = b.case
  xt = _transformed(b, logical_x(b, dtype))
  if c.geom == "convT":
    full = F.conv_transpose3d(xt, b.w.to(dtype), None, stride=2, padding=c.pad[0], output_padding=1)   # [B, cout, 2D, 2H, 2W]
    B, N = full.shape[:2]
    D, H, W = c.odims
    return full.view(B, N, D, 2, H, 2, W, 2).permute(0, 3, 5, 7, 1, 2, 4, 6).reshape(B, 8 * N, D, H, W)   # parity major
  if c.geom == "dgrad":                  # autograd of the forward convolution, the transformed x as its output gradient
    with t.enable_grad():
      xin = t.zeros(c.B, c.cout, *c.odims, dtype=dtype, requires_grad=True)
      (g,) = t.autograd.grad(F.conv3d(xin, b.w.to(dtype), padding=c.pad), xin, xt)
    return g
  if c.geom == "convT_dgrad":            # ... of the transposed convolution; the storage of x is dy itself
    D, H, W = c.xd
    assert b.scale is None                     # (this geometry is given no input transform)
    dy = b.xs.to(dtype).view(c.B, c.cin, 2 * D, 2 * H, 2 * W)
    with t.enable_grad():
      xin = t.zeros(c.B, c.cout, *c.odims, dtype=dtype, requires_grad=True)
      (g,) = t.autograd.grad(F.conv_transpose3d(xin, b.w.to(dtype), None, stride=2, padding=c.pad[0], output_padding=1), xin, dy)
    return g
  return F.conv3d(F.pad(xt, _pads(b, xt, b.pad_lo)), b.w.to(dtype))


def corr_logical(b, dtype=t.float64, wp=None, pad_lo=None, pad_first=False, chan_keep=None):
  """The same through the PACKED weights -- the form the library is handed -- with the knobs the sensitivity test turns:
  other packed weights, other pads, the zero pad transformed, input channels dropped."""
  pad_lo = b.pad_lo if pad_lo is None else pad_lo
  x = logical_x(b, dtype)
  if pad_first:
    xp = _transformed(b, F.pad(x, _pads(b, x, pad_lo)))
  else:
    xt = _transformed(b, x)
    xp = F.pad(xt, _pads(b, xt, pad_lo))
  if chan_keep is not None:
    xp = xp * chan_keep.to(dtype).view(1, -1, 1, 1, 1)
  wk = (b.wp if wp is None else wp).to(dtype).view(b.ycin, *b.window, b.npad).permute(4, 0, 1, 2, 3)
  return F.conv3d(xp, wk)[:, :b.ycout]


def bias_logical(b, dtype=t.float64):
  if b.bp is None: return 0.0
  return b.bp[:b.ycout].to(dtype).view(1, -1, 1, 1, 1)


def expected_y(b, conv_part, bias_times=1, accumulate=None):
  """float64 storage the call must leave: y0 outside the view, (y0 +) bias + conv inside."""
  acc = b.case.accumulate if accumulate is None else accumulate
  st = b.y0.double().clone()
  write_logical(yview(b, st), conv_part + bias_times * bias_logical(b), acc)
  return st


@t.enable_grad()
def ref_wgrad_packed(b, dtype=t.float64, pad_lo=None, pad_first=False, dy_keep=None):
  """Autograd's weight gradient in the packed layout [cin][T][npad] (zeros where the packed weights hold no real tap).
  dy_keep: 0/1 over [B, 1, D, H, W], the output positions that take part (sensitivity test)."""
  c = b.case
  dy = logical(yview(b, b.dys.to(dtype)))
  if dy_keep is not None: dy = dy * dy_keep.to(dtype)
  w = b.w.to(dtype).clone().requires_grad_(True)
  x = logical_x(b, dtype)
  if c.geom == "convT":
    out = F.conv_transpose3d(_transformed(b, x), w, None, stride=2, padding=c.pad[0], output_padding=1)
    B, N = out.shape[:2]
    D, H, W = c.odims
    out = out.view(B, N, D, 2, H, 2, W, 2).permute(0, 3, 5, 7, 1, 2, 4, 6).reshape(B, 8 * N, D, H, W)
  else:
    pl = b.pad_lo if pad_lo is None else pad_lo
    if pad_first:
      xp = _transformed(b, F.pad(x, _pads(b, x, pl)))
    else:
      xt = _transformed(b, x)
      xp = F.pad(xt, _pads(b, xt, pl))
    out = F.conv3d(xp, w)
  (gw,) = t.autograd.grad(out, w, dy)
  return t.where(b.index >= 0, gw.reshape(-1)[b.index.clamp(min=0)], t.zeros((), dtype=dtype))


def real_entries(b):
  """Entries of the packed gradient that hold a real tap of a real column (the tap boxes of the geometries here cover them all)."""
  return b.index >= 0


def err_inside(got, want, mask, scale):
  """max |got - want| over mask, in units of `scale` (= max |reference|)."""
  d = (got.double() - want.double()).abs()
  return float(d[mask].max()) / (float(scale) + 1e-300)


def outside_equal(got, y0, mask):
  """Everything the view does not address is bit-identical to what the buffer held."""
  return bool(t.equal(got[~mask].view(t.int32), y0[~mask].view(t.int32)))


# ------------------------------------------------------------------------------------------------ running and checking
def query_plan(be, b, xs, ys, wp, dw=None):
  """The plan of the case's call on these storages (be: HipBackend; any device, CPU included)."""
  c = b.case
  tr = transform_of(b, xs.device)
  if c.op == "fwd":
    return be.conv_fwd_plan(xview(b, xs), tr, wp, b.npad, None if b.bp is None else wp, 0, yview(b, ys), b.window, b.pad_lo,
                            c.splits, c.accumulate, boxes=b.boxes)
  return be.conv_wgrad_plan(xview(b, xs), tr, yview(b, ys), dw, b.npad, b.window, b.pad_lo, not c.accumulate, boxes=b.boxes)


def run_fwd(be, b, dev, tr_cls=None):
  """The case's crn_conv_fwd call on device dev -> the output storage."""
  c = b.case
  y = b.y0.to(dev).clone()
  xs = b.xs.to(dev)
  be.conv_fwd(xview(b, xs), transform_of(b, dev, tr_cls), b.wp.to(dev), b.npad, None if b.bp is None else b.bp.to(dev), 0,
              yview(b, y), b.window, b.pad_lo, c.splits, c.accumulate, boxes=b.boxes)
  return y


def run_wgrad(be, b, dev, tr_cls=None):
  c = b.case
  dw = b.dw0.to(dev).clone()
  be.conv_wgrad(xview(b, b.xs.to(dev)), transform_of(b, dev, tr_cls), yview(b, b.dys.to(dev)), dw, b.npad, b.window, b.pad_lo,
                not c.accumulate, boxes=b.boxes)
  return dw


class FwdRef:
  """float64 reference of a forward case, computed once: what the storage must hold, and the range of the bar."""

  def __init__(self, b):
    conv = ref_fwd_logical(b)
    self.mask = inside_mask(b.case.yview, b.case.B, b.ycout, b.case.odims)
    self.want = expected_y(b, conv)
    self.range = float((conv + bias_logical(b)).abs().max())      # of what the call computes (not of an accumulation base)

  def check(self, b, got):
    """-> (max error inside the view / range, everything outside the view bit-identical)."""
    got = got.detach().cpu()
    return err_inside(got, self.want, self.mask, self.range), outside_equal(got, b.y0, self.mask)


class WgradRef:
  def __init__(self, b):
    self.grad = ref_wgrad_packed(b)
    self.real = real_entries(b)
    self.range = float(self.grad.abs().max())                     # = max |dw - dw0| of an accumulating call
    self.want = self.grad + (b.dw0.double() if b.case.accumulate else 0.0)

  def check(self, b, got):
    """-> (max error over the real entries / range, the other entries right: columns >= Cout hold no tap, so a zero_first
    call leaves 0 there and an accumulating one the bits it found; under tap boxes they may be left untouched: not looked at)."""
    got = got.detach().cpu()
    pad_ok = True
    if b.case.boxes != "geom":
      pad = ~self.real
      pad_ok = bool(t.equal(got[pad], b.dw0[pad])) if b.case.accumulate else bool((got[pad] == 0).all())
    return err_inside(got, self.want, self.real, self.range), pad_ok
