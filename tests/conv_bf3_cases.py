"""The case table of the split-bf16 convolution engine (csrc/conv_bf3.hip) and what its tests share.  TEST INFRASTRUCTURE ONLY.

One row = one crn_conv_fwd_bf3 / crn_conv_fwd_bf3_slabs (also with a fused BatchRenorm epilogue) or crn_conv_wgrad_bf3_boxes
call on views of seeded tensors, and the kernel variant the row is there for (`expect`: fields of the plan query
crn_conv_fwd_bf3_plan / crn_conv_wgrad_bf3_plan).  The Case dataclass, the view kinds, the seeded inputs, the float64
references and the sentinel discipline are those of tests/conv_fp32_cases.py.  tests/test_conv_bf3_plan_cpu.py asks the
query on the CPU and proves what the table reaches; tests/test_conv_bf3_gpu.py runs every row on the GPU.

Shapes were found with the query, smallest first: y of (5, 9, 16) = four 4 x 8 x 16 tiles, partial in D and H; (5, 9, 32) =
two tiles in W; (9, 10, 8) = four 8 x 8 x 8 tiles, partial in D and H.  No tensor of the table has more than about 2M elements.

Bars.  Against float64: BAR = 2e-5 of max|reference|; the operand split alone (the split model below, summed in float64) takes
3.0e-6 .. 7.0e-6 of it on the rows here.  Against the split model: SPLIT_BAR = 4 x 1.03e-6, four times the largest difference
between float32 and float64 summation of the split model over all rows (row e_scalar_store_mw8).  Measured on an MI355X, largest error per
kernel family, of max|reference| (against float64 / against the split model):
  forward plain, unit-stride x, 5x5 planes   4.9e-6 / 8.0e-7      weight gradient, 8 pairs per wave, 16-wide tiles   7.0e-6 / 8.6e-7
  forward plain, unit-stride x, 4x4 planes   5.6e-6 / 6.2e-7      weight gradient, 8 pairs per wave, 8-wide tiles    7.1e-6 / 3.4e-7
  forward plain, stride-2 x, 4x4 planes      5.0e-6 / 5.4e-7      weight gradient, 4 pairs, plain dy, 16-wide        5.5e-6 / 6.9e-7
  forward half kernels                       5.0e-6 / 5.6e-7      weight gradient, 4 pairs, stride-2 dy, 16-wide     6.7e-6 / 4.5e-7
  forward wave-specialised                   5.4e-6 / 6.4e-7      weight gradient, 4 pairs, stride-2 dy, 8-wide      6.4e-6 / 4.2e-7
Fused epilogues: statistics sums within 1.3e-8 of float64 sums over the launch's own y (bar 3e-6), backward sums within 1.4e-7
(bar 2e-5).  The staged-weights and the slab form gave the same bits on every forward row, the wave-specialised kernel included.
"""
from __future__ import annotations

import dataclasses

import torch as t
import torch.nn.functional as F

import conv_fp32_cases as K32
from conv_fp32_cases import SENTINEL, make_view, view_numel, inside_mask, xview, yview, transform_of       # noqa: F401 (shared)
from kernel_contract_emu import EmuBackend, logical, write_logical
from corenet_amd.model import conv_geometry as G

SPLIT_MAX_F32 = 1.03e-6     # the largest difference, over all rows, between the split model summed in float32 (torch's order) and
                            # in float64, of max|reference| (tests/test_conv_bf3_plan_cpu.py measures it: row e_scalar_store_mw8)
SPLIT_BAR = 4 * SPLIT_MAX_F32     # the kernel against the split model: only the order of the float32 sums differs (32-deep MFMA
                                  # blocks, split-K partial sums, atomics in the weight gradient), allowed 4x torch's own
BAR = 2e-5             # of max|float64 reference|: the project's bar for this engine (tests/test_kernels_gpu.py), forward, data
                       # gradient and weight gradient alike
_EMU = EmuBackend()


@dataclasses.dataclass(frozen=True)
class Case(K32.Case):
  slabs: bool = False                # forward: the weights as the slab image of crn_bf3_operands
  bias_b: bool = False               # forward: one bias row per sample (bias_sB = Npad)
  fuse: str = ""                     # "" | stats (crn_conv_fwd_bf3_slabs_stats) | bnbwd (crn_conv_fwd_bf3_slabs_bnbwd)
  decline: str = ""                  # fuse rows: what makes the launch decline (nparts == 0) where the shape alone does not:
                                     # ws_short | ndsum | x_misaligned | sB_x


def _c(name, expect, **kw):
  return Case(name, expect, **kw)


P5, P4 = (2, 2, 2), (1, 1, 1)
# ------------------------------------------------------------------------------------------------ the table
# expect = what the plan query says for the row; a retune that moves a row to another kernel fails
# tests/test_conv_bf3_plan_cpu.py, and the row then gets another shape (found with the query), never another expectation.
#
# What no shape reaches (tests/test_conv_bf3_plan_cpu.py::test_what_no_call_reaches holds the arithmetic):
#  * the LDS shrink loop of NSUB and both `lds > limit` rejections: a patch has at most 1024 staging units = 64 KiB, the weight
#    slabs of the widest block 56 KiB (weight gradient: 64 KiB of dy), the channel tables 6 KiB -- under the 159.5 KiB limit;
#  * `nch <= 64` of the wave-specialised kernel can never be false: x->C <= kTabC = 512 gives at most 64 chunks;
#  * a failing bf3_ws_timetable_ok<5>: it holds for every 1 <= nch <= 64 (the query is asked for each);
#  * `2 * UP <= 256` and the LDS bound of the wave-specialised kernel: it needs 16-wide tiles and kd = 5, so a patch is 8 planes
#    of UP units and the 1024-unit limit gives UP <= 128 (a 5^3 window with an odd pw, 132 units per plane, is rejected outright:
#    it is a row of rejections()).
#    So the fall-back from the wave-specialised to the plain kernel is NOT reachable, and no row exercises it: every call that
#    meets `NSUB == 2 && NG == 7 && slabs && unit-stride x && 16-wide tiles && kd == 5` runs the wave-specialised kernel.  (Row
#    f_n2_g7_s_oddpw reaches the plain NSUB 2 / seven-group / slab kernel on 8-wide tiles, where those conditions do not hold.)
#  * `D*H*W % 4 != 0` among the decline conditions of the fused epilogues: an accepted y has W % 8 == 0.
CASES = [
    # ---- one row per instantiated forward kernel: plain (NSUB 1/2/4) x (unit-stride x under 5x5 planes | under 4x4 planes |
    # stride-2 x under 4x4 planes) x (weights staged | slabs), the four half kernels, the wave-specialised kernel
    _c('f_n1_g7_w', dict(kind='plain', nsub=1, xmode=1, ng=7, slabs=0, half_last=0, splits=2, vec_store=1, mode=3),
       B=2, cin=13, cout=12, k=(5, 5, 5), pad=P5, odims=(5, 9, 16), tr='pre'),
    _c('f_n1_g7_s', dict(kind='plain', nsub=1, xmode=1, ng=7, slabs=1, half_last=1, lead=1, splits=2, vec_store=1, mode=3),
       cin=12, cout=16, k=(2, 5, 5), pad=(1, 2, 1), odims=(5, 9, 32), tr='post', slabs=True),      # (odd pw: 22 patch columns, no half kernel)
    _c('f_n2_g7_w', dict(kind='plain', nsub=2, xmode=1, ng=7, slabs=0, half_last=1, splits=3, vec_store=1, mode=3),
       cin=20, cout=24, k=(5, 5, 5), pad=P5, odims=(5, 9, 32), xview='slice', yview='slice', tr='both', accumulate=True),
    _c('f_n2_g7_s_oddpw', dict(kind='plain', nsub=2, xmode=1, ng=7, slabs=1, lead=1, td=8, splits=3, vec_store=1, mode=3),
       B=2, cin=20, cout=24, k=(5, 5, 5), pad=(2, 2, 3), odims=(9, 10, 8), tr='shift', slabs=True),
    _c('f_n4_g7_w', dict(kind='plain', nsub=4, xmode=1, ng=7, slabs=0, splits=9, vec_store=1, mode=3),
       cin=72, cout=40, k=(5, 5, 5), pad=P5, odims=(5, 9, 16), xview='sb2', tr='scale', bias=False),
    _c('f_n4_g7_s', dict(kind='plain', nsub=4, xmode=1, ng=7, slabs=1, half_last=1, splits=3, vec_store=1, mode=3),
       B=3, cin=20, cout=40, k=(5, 5, 5), pad=P5, odims=(9, 10, 8), tr='pre', slabs=True),
    _c('f_n1_g4_w', dict(kind='plain', nsub=1, xmode=1, ng=4, slabs=0, half_last=0, lead=1, splits=2, vec_store=1, mode=3),
       B=2, cin=13, cout=12, k=(4, 4, 4), pad=P4, odims=(5, 9, 16), tr='post'),
    _c('f_n1_g4_s', dict(kind='plain', nsub=1, xmode=1, ng=4, slabs=1, half_last=1, lead=0, splits=2, vec_store=1, mode=3),
       cin=12, cout=16, k=(4, 4, 4), pad=(1, 1, 2), odims=(9, 10, 8), tr='shift', slabs=True),
    _c('f_n2_g4_w', dict(kind='plain', nsub=2, xmode=1, ng=4, slabs=0, splits=9, vec_store=1, mode=3),
       cin=72, cout=24, k=(4, 4, 4), pad=(1, 1, 2), odims=(5, 9, 32), yview='off1', tr='pre', accumulate=True, bias=False),
    _c('f_n2_g4_s', dict(kind='plain', nsub=2, xmode=1, ng=4, slabs=1, splits=9, vec_store=1, mode=3),
       B=2, cin=72, cout=40, k=(4, 4, 4), pad=P4, odims=(9, 10, 8), tr='both', slabs=True),
    _c('f_n4_g4_w', dict(kind='plain', nsub=4, xmode=1, ng=4, slabs=0, half_last=1, splits=3, vec_store=1, mode=3),
       cin=20, cout=40, k=(4, 4, 4), pad=(2, 2, 2), odims=(5, 9, 16), xdims=(6, 10, 16), tr='scale'),
    _c('f_n4_g4_s', dict(kind='plain', nsub=4, xmode=1, ng=4, slabs=1, splits=9, vec_store=1, mode=3),
       cin=72, cout=64, k=(4, 4, 4), pad=P4, odims=(5, 9, 16), xview='slice', tr='shift', slabs=True),
    _c('f_n1_x2_w', dict(kind='plain', nsub=1, xmode=2, ng=4, slabs=0, half_last=1, splits=2, vec_store=1, mode=3),
       B=2, cin=12, cout=12, k=(4, 4, 4), pad=P4, odims=(5, 9, 16), xview='s2co', tr='pre'),
    _c('f_n1_x2_s', dict(kind='plain', nsub=1, xmode=2, ng=4, slabs=1, half_last=0, splits=3, vec_store=1, mode=3),
       cin=3, cout=12, k=(7, 7, 7), pad=(3, 3, 3), odims=(5, 9, 16), geom='convT_dgrad', xview='s2d', bias=False, boxes='geom', slabs=True),
    _c('f_n2_x2_w', dict(kind='plain', nsub=2, xmode=2, ng=4, slabs=0, splits=3, vec_store=1, mode=3),
       cin=22, cout=24, k=(4, 4, 4), pad=(1, 1, 2), odims=(9, 10, 8), xview='s2co', yview='sb2', tr='post', accumulate=True),
    _c('f_n2_x2_s', dict(kind='plain', nsub=2, xmode=2, ng=4, slabs=1, rowskip=1, splits=2, vec_store=1, mode=3),
       B=2, cin=2, cout=24, k=(7, 7, 7), pad=(3, 3, 3), odims=(5, 9, 16), geom='convT_dgrad', xview='s2d', bias=False, boxes='geom', slabs=True),
    _c('f_n4_x2_w', dict(kind='plain', nsub=4, xmode=2, ng=4, slabs=0, splits=3, vec_store=1, mode=3),
       cin=20, cout=40, k=(4, 4, 4), pad=P4, odims=(5, 9, 16), xview='s2co', tr='both'),
    _c('f_n4_x2_s', dict(kind='plain', nsub=4, xmode=2, ng=4, slabs=1, rowskip=1, splits=2, vec_store=1, mode=3),
       cin=2, cout=40, k=(7, 7, 7), pad=(3, 3, 3), odims=(5, 9, 32), geom='convT_dgrad', xview='s2d', bias=False, accumulate=True, boxes='geom', slabs=True),
    _c('f_half_g7_w', dict(kind='half', nsub=1, xmode=1, ng=7, slabs=0, half_last=1, splits=2, vec_store=1, mode=3),
       B=2, cin=12, cout=12, k=(5, 5, 5), pad=P5, odims=(5, 9, 16), tr='pre'),
    _c('f_half_g7_s', dict(kind='half', nsub=1, xmode=1, ng=7, slabs=1, half_last=1, splits=1, vec_store=1, mode=0),
       B=2, cin=3, cout=16, k=(5, 5, 5), pad=(0, 0, 0), odims=(5, 9, 32), xdims=(9, 13, 36), tr='both', slabs=True),
    _c('f_half_g4_w', dict(kind='half', nsub=1, xmode=1, ng=4, slabs=0, half_last=1, lead=0, splits=4, vec_store=1, mode=3),
       cin=25, cout=12, k=(4, 4, 4), pad=(1, 1, 2), odims=(5, 9, 16), yview='off1', tr='post'),
    _c('f_half_g4_s_oddpw', dict(kind='half', nsub=1, xmode=1, ng=4, slabs=1, half_last=1, lead=1, splits=2, vec_store=1, mode=3),
       B=2, cin=9, cout=16, k=(4, 4, 4), pad=P4, odims=(5, 9, 16), yview='slice', tr='shift', accumulate=True, slabs=True),
    _c('f_ws_1', dict(kind='ws', nsub=2, xmode=1, ng=7, slabs=1, splits=1, per_split=1, vec_store=1, mode=0),
       B=2, cin=7, cout=24, k=(5, 5, 5), pad=P5, odims=(5, 9, 16), tr='pre', slabs=True),
    _c('f_ws_2', dict(kind='ws', nsub=2, xmode=1, ng=7, slabs=1, splits=9, per_split=2, vec_store=1, mode=3),
       cin=133, cout=24, k=(5, 5, 5), pad=P5, odims=(5, 9, 16), yview='slice', tr='both', accumulate=True, slabs=True),
    _c('f_ws_3', dict(kind='ws', nsub=2, xmode=1, ng=7, slabs=1, splits=11, per_split=3, vec_store=1, mode=3),
       cin=264, cout=20, k=(5, 5, 5), pad=P5, odims=(5, 9, 16), tr='shift', slabs=True),
    # ---- the NSUB selection: Npad <= 16 / <= 32 above; Npad > 32: 64 columns for up to 64 tiles of 16-wide sub-tiles (above) or for
    # few input channels without n-boxes; 32 columns otherwise
    _c('n_tiles72_c20', dict(kind='plain', nsub=4, xmode=1, ng=4, splits=3, chunks=3),
       B=3, cin=20, cout=40, k=(4, 4, 4), pad=P4, odims=(13, 9, 48), tr='pre'),
    _c('n_tiles72_c40', dict(kind='plain', nsub=2, xmode=1, ng=4, splits=2, vec_store=1, mode=3),
       B=3, cin=40, cout=40, k=(4, 4, 4), pad=P4, odims=(13, 9, 48), tr='pre', slabs=True),
    _c('n_tiles72_nbox', dict(kind='plain', nsub=2, xmode=1, ng=4, rowskip=1, n_groups=8, splits=2),
       B=3, cin=20, cout=5, k=(7, 7, 7), pad=(3, 3, 3), odims=(13, 9, 48), geom='convT', yview='s2d', tr='pre', boxes='geom', slabs=True),
    _c('n_mw8_c40', dict(kind='plain', nsub=2, xmode=1, ng=7, td=8, tw=8, splits=5, vec_store=1, mode=3),
       cin=40, cout=40, k=(5, 5, 5), pad=P5, odims=(9, 10, 8), tr='post'),
    # ---- edges
    _c('e_cin1', dict(kind='half', nsub=1, xmode=1, ng=7, half_last=1, splits=1, mode=0),
       B=2, cin=1, cout=16, k=(5, 5, 5), pad=P5, odims=(5, 9, 16), tr='shift'),
    _c('e_cin2_x2', dict(kind='plain', nsub=1, xmode=2, ng=4, half_last=1, splits=1, mode=0),
       B=2, cin=2, cout=16, k=(4, 4, 4), pad=P4, odims=(5, 9, 16), xview='s2co', tr='shift'),
    _c('e_cin6_x2', dict(kind='plain', nsub=2, xmode=2, ng=4, half_last=0, splits=1, mode=1),
       B=2, cin=6, cout=24, k=(4, 4, 4), pad=P4, odims=(9, 10, 8), xview='s2co', tr='both', accumulate=True),
    _c('e_cin7_mw8', dict(kind='plain', nsub=1, xmode=1, ng=7, half_last=0, td=8, splits=1, mode=0),
       B=2, cin=7, cout=16, k=(5, 5, 5), pad=P5, odims=(9, 10, 8), tr='pre'),
    _c('e_sb_gap', dict(kind='plain', nsub=2, xmode=1, ng=7, splits=3, vec_store=1, mode=3),
       B=3, cin=20, cout=24, k=(5, 5, 5), pad=P5, odims=(9, 10, 8), xview='sb2', yview='sb2', tr='pre'),
    _c('e_pad0_xbig', dict(kind='plain', nsub=2, xmode=1, ng=4, lead=0, splits=2),
       cin=13, cout=24, k=(4, 4, 4), pad=(0, 0, 0), odims=(5, 9, 16), xdims=(8, 12, 20), tr='post'),
    _c('e_pad_big', dict(kind='plain', nsub=2, xmode=1, ng=7, lead=0, splits=2),
       cin=13, cout=24, k=(5, 5, 5), pad=(4, 3, 4), odims=(9, 10, 8), xdims=(6, 8, 6), tr='both'),
    _c('e_pad0_xbig_x2', dict(kind='plain', nsub=2, xmode=2, ng=4, lead=0, splits=2),
       cin=14, cout=24, k=(4, 4, 4), pad=(0, 0, 0), odims=(5, 9, 16), xdims=(8, 12, 20), xview='s2co', tr='post'),
    _c('e_pad_big_x2', dict(kind='plain', nsub=2, xmode=2, ng=4, td=8, lead=0, splits=2),
       cin=14, cout=24, k=(4, 4, 4), pad=(3, 2, 4), odims=(9, 10, 8), xdims=(6, 8, 6), xview='s2co', tr='both'),
    _c('e_pad_odd_xsmall_x2', dict(kind='plain', nsub=1, xmode=2, ng=4, lead=1, splits=2),
       B=2, cin=10, cout=16, k=(4, 4, 4), pad=(4, 1, 5), odims=(5, 9, 16), xdims=(4, 8, 10), xview='s2co', tr='pre'),
    _c('e_bias_per_sample_mw8', dict(kind='plain', nsub=2, xmode=1, ng=4, td=8, splits=2, mode=3),
       B=3, cin=13, cout=24, k=(4, 4, 4), pad=P4, odims=(9, 10, 8), tr='pre', bias_b=True),
    _c('e_bias_per_sample_mw8_acc', dict(kind='plain', nsub=2, xmode=1, ng=7, td=8, splits=1, mode=1),
       B=3, cin=8, cout=24, k=(5, 5, 5), pad=P5, odims=(9, 10, 8), accumulate=True, bias_b=True, slabs=True),
    _c('e_scalar_store_acc_w16', dict(kind='plain', nsub=2, xmode=1, ng=4, splits=1, vec_store=0, mode=1),
       B=2, cin=8, cout=24, k=(4, 4, 4), pad=P4, odims=(5, 9, 16), yview='sb2', tr='pre', accumulate=True),
    _c('e_scalar_store_mw8', dict(kind='plain', nsub=4, xmode=1, ng=7, td=8, splits=1, vec_store=0, mode=0),
       B=2, cin=8, cout=40, k=(5, 5, 5), pad=P5, odims=(9, 10, 8), yview='co', tr='pre'),
    _c('e_bias_per_sample', dict(kind='plain', nsub=2, xmode=1, ng=7, splits=2, mode=3),
       B=3, cin=13, cout=24, k=(5, 5, 5), pad=P5, odims=(5, 9, 16), tr='pre', bias_b=True),
    _c('e_bias_per_sample_acc', dict(kind='ws', nsub=2, xmode=1, ng=7, splits=1, mode=1),
       B=3, cin=8, cout=24, k=(5, 5, 5), pad=P5, odims=(5, 9, 16), accumulate=True, bias_b=True, slabs=True),
    _c('e_scalar_store', dict(kind='plain', nsub=4, xmode=1, ng=7, splits=1, vec_store=0, mode=0),
       B=2, cin=8, cout=40, k=(5, 5, 5), pad=P5, odims=(5, 9, 16), yview='co', tr='pre'),
    _c('e_scalar_store_acc', dict(kind='plain', nsub=4, xmode=1, ng=4, splits=1, vec_store=0, mode=1),
       B=2, cin=8, cout=40, k=(4, 4, 4), pad=P4, odims=(9, 10, 8), yview='off1', tr='pre', accumulate=True),
    _c('e_vec_store_acc', dict(kind='plain', nsub=4, xmode=1, ng=4, splits=1, vec_store=1, mode=1),
       B=2, cin=8, cout=40, k=(4, 4, 4), pad=P4, odims=(9, 10, 8), yview='slice', tr='pre', accumulate=True),
    _c('e_boxes_odd', dict(kind='plain', nsub=4, xmode=1, ng=4, rowskip=0, n_groups=0, c_groups=0, splits=3),
       cin=20, cout=40, k=(4, 4, 4), pad=P4, odims=(5, 9, 16), tr='pre', boxes='odd'),
    _c('e_convT_boxes', dict(kind='plain', nsub=4, xmode=1, ng=4, rowskip=1, n_groups=8, c_groups=0, splits=2),
       B=2, cin=12, cout=5, k=(7, 7, 7), pad=(3, 3, 3), odims=(5, 9, 16), geom='convT', yview='s2d', tr='pre', boxes='geom'),
    _c('e_convT_noboxes', dict(kind='plain', nsub=4, xmode=1, ng=4, rowskip=0, n_groups=0, splits=2),
       B=2, cin=12, cout=5, k=(7, 7, 7), pad=(3, 3, 3), odims=(5, 9, 16), geom='convT', yview='s2d', tr='pre'),
    _c('e_convT_dgrad_cbox', dict(kind='plain', nsub=2, xmode=2, ng=4, rowskip=1, n_groups=0, c_groups=8, splits=2, mode=3),
       B=2, cin=2, cout=20, k=(7, 7, 7), pad=(3, 3, 3), odims=(9, 10, 8), geom='convT_dgrad', xview='s2d', bias=False, boxes='geom'),
    _c('g_dgrad_k5', dict(kind='ws', nsub=2, xmode=1, ng=7, splits=3, mode=3),
       B=2, cin=20, cout=24, k=(5, 5, 5), pad=P5, odims=(5, 9, 16), geom='dgrad', bias=False, accumulate=True, slabs=True),
    # ---- windows the model does not use but the entry accepts
    _c('w_344', dict(kind='plain', nsub=2, xmode=1, ng=4, splits=2), cin=13, cout=24, k=(3, 4, 4), pad=(1, 1, 2), odims=(5, 9, 16), tr='pre'),
    _c('w_255', dict(kind='plain', nsub=2, xmode=1, ng=7, splits=2), cin=13, cout=24, k=(2, 5, 5), pad=(1, 2, 2), odims=(5, 9, 16), tr='pre', slabs=True),
    _c('w_744', dict(kind='plain', nsub=2, xmode=1, ng=4, td=8, splits=2), cin=13, cout=24, k=(7, 4, 4), pad=(3, 1, 2), odims=(9, 10, 8), tr='pre'),
    _c('w_127', dict(kind='plain', nsub=2, xmode=1, ng=4, splits=2), cin=13, cout=24, k=(1, 2, 7), pad=(0, 1, 3), odims=(5, 9, 16), tr='pre', slabs=True),
    _c('w_535', dict(kind='plain', nsub=2, xmode=1, ng=4, splits=2), cin=13, cout=24, k=(5, 3, 5), pad=(2, 1, 2), odims=(5, 9, 16), tr='pre'),
    _c('w_235_half', dict(kind='half', nsub=1, xmode=1, ng=4, splits=2), cin=12, cout=16, k=(2, 3, 5), pad=(1, 1, 2), odims=(5, 9, 16), tr='pre'),
    _c('w_547_ws', dict(kind='ws', nsub=2, xmode=1, ng=7, splits=2), cin=13, cout=24, k=(5, 4, 7), pad=(2, 1, 2), odims=(5, 9, 16), tr='pre', slabs=True),
    _c('w_539_ws', dict(kind='ws', nsub=2, xmode=1, ng=7, splits=1), B=2, cin=8, cout=24, k=(5, 3, 9), pad=(2, 1, 4), odims=(5, 9, 16), tr='pre', slabs=True),
    _c('w_755_mw8', dict(kind='plain', nsub=2, xmode=1, ng=7, td=8, splits=2), cin=13, cout=24, k=(7, 5, 5), pad=(3, 2, 2), odims=(9, 10, 8), tr='pre'),
    # ---- fused BatchRenorm epilogues at partial tiles, two N blocks (Npad 128 in 64-column blocks), and what makes them decline
    _c('s_stats_16', dict(kind='plain', nsub=4, splits=1, vec_store=1, nparts=8), B=2, cin=6, cout=80, k=(5, 5, 5), pad=P5,
       odims=(5, 9, 16), tr='pre', slabs=True, fuse='stats'),
    _c('s_stats_32', dict(kind='plain', nsub=4, splits=1, vec_store=1, nparts=16), B=2, cin=8, cout=72, k=(4, 4, 4), pad=P4,
       odims=(6, 10, 32), tr='pre', slabs=True, fuse='stats'),
    _c('s_stats_ws', dict(kind='ws', nsub=2, splits=1, vec_store=1, nparts=8), B=2, cin=8, cout=24, k=(5, 5, 5), pad=P5,
       odims=(5, 9, 16), tr='pre', slabs=True, fuse='stats'),
    _c('s_bnbwd_16', dict(kind='plain', nsub=4, splits=1, vec_store=1, nparts=8), B=2, cin=6, cout=80, k=(5, 5, 5), pad=P5,
       odims=(5, 9, 16), bias=False, slabs=True, fuse='bnbwd'),
    _c('s_bnbwd_32', dict(kind='plain', nsub=4, splits=1, vec_store=1, nparts=16), B=2, cin=8, cout=72, k=(4, 4, 4), pad=P4,
       odims=(6, 10, 32), bias=False, slabs=True, fuse='bnbwd'),
    _c('s_bnbwd_ws', dict(kind='ws', nsub=2, splits=1, vec_store=1, nparts=8), B=2, cin=8, cout=24, k=(5, 5, 5), pad=P5,
       odims=(5, 9, 16), bias=False, slabs=True, fuse='bnbwd'),
    _c('s_stats_half', dict(kind='half', nsub=1, half_last=1, splits=1, vec_store=1, nparts=8), B=2, cin=3, cout=10, k=(5, 5, 5), pad=P5,
       odims=(5, 9, 16), tr='pre', slabs=True, fuse='stats'),                                       # (the epilogue is shared: the half kernel too)
    _c('s_bnbwd_half', dict(kind='half', nsub=1, half_last=1, splits=1, vec_store=1, nparts=8), B=2, cin=3, cout=10, k=(5, 5, 5), pad=P5,
       odims=(5, 9, 16), bias=False, slabs=True, fuse='bnbwd'),
    _c('s_decl_splits', dict(splits=2, nparts=0), B=2, cin=13, cout=80, k=(5, 5, 5), pad=P5, odims=(5, 9, 16), slabs=True, fuse='stats'),
    _c('s_decl_scalar_store', dict(splits=1, vec_store=0, nparts=0), B=2, cin=6, cout=80, k=(5, 5, 5), pad=P5, odims=(5, 9, 16),
       yview='off1', slabs=True, fuse='stats'),
    _c('s_decl_ws_short', dict(splits=1, vec_store=1, nparts=0), B=2, cin=6, cout=80, k=(5, 5, 5), pad=P5, odims=(5, 9, 16),
       slabs=True, fuse='stats', decline='ws_short'),
    _c('s_decl_ndsum', dict(splits=1, vec_store=1, nparts=0), B=2, cin=6, cout=80, k=(5, 5, 5), pad=P5, odims=(5, 9, 16),
       slabs=True, fuse='bnbwd', bias=False, decline='ndsum'),
    _c('s_decl_x_misaligned', dict(splits=1, vec_store=1, nparts=0), B=2, cin=6, cout=80, k=(5, 5, 5), pad=P5, odims=(5, 9, 16),
       slabs=True, fuse='bnbwd', bias=False, decline='x_misaligned'),
    _c('s_decl_sB_x', dict(splits=1, vec_store=1, nparts=0), B=2, cin=6, cout=80, k=(5, 5, 5), pad=P5, odims=(5, 9, 16),
       slabs=True, fuse='bnbwd', bias=False, decline='sB_x'),
    # ---- one row per instantiated weight-gradient kernel: NSUB x (dy staging, tap pairs per wave, tile width)
    _c('g_n1_d1_p8_w16', dict(nsub=1, dmode=1, tpw=8, twt=16, pipe=1, inherit=1, boxskip=0, splits=8),
       B=2, cin=13, cout=12, k=(5, 5, 5), pad=P5, odims=(5, 9, 16), op='wgrad', tr='pre'),
    _c('g_n2_d1_p8_w16', dict(nsub=2, dmode=1, tpw=8, twt=16, pipe=1, inherit=1, splits=8),
       B=2, cin=72, cout=56, k=(5, 5, 5), pad=P5, odims=(5, 9, 16), op='wgrad', xview='slice', yview='slice', tr='both', accumulate=True),
    _c('g_n1_d2_p4_w16', dict(nsub=1, dmode=2, tpw=4, twt=16, pipe=1, boxskip=1, splits=8),
       B=2, cin=12, cout=2, k=(7, 7, 7), pad=(3, 3, 3), odims=(5, 9, 16), op='wgrad', geom='convT', yview='s2d', tr='pre', boxes='geom'),
    _c('g_n2_d2_p4_w16', dict(nsub=2, dmode=2, tpw=4, twt=16, pipe=0, boxskip=0, splits=8),
       B=2, cin=13, cout=24, k=(4, 4, 4), pad=P4, odims=(5, 9, 16), op='wgrad', yview='co', tr='post'),
    _c('g_n1_d1_p4_w16', dict(nsub=1, dmode=1, tpw=4, twt=16, pipe=1, splits=4),
       cin=20, cout=40, k=(4, 4, 4), pad=(1, 1, 2), odims=(5, 9, 16), op='wgrad', tr='shift', accumulate=True),
    _c('g_n2_d1_p4_w16', dict(nsub=2, dmode=1, tpw=4, twt=16, pipe=0, splits=16, chunks=16),
       B=2, cin=7, cout=20, k=(4, 4, 4), pad=P4, odims=(5, 9, 32), op='wgrad', xview='sb2', tr='pre'),
    _c('g_n1_d1_p8_w8', dict(nsub=1, dmode=1, tpw=8, twt=8, pipe=1, splits=8),
       B=2, cin=13, cout=12, k=(5, 5, 5), pad=P5, odims=(9, 10, 8), op='wgrad', tr='both'),
    _c('g_n2_d1_p8_w8', dict(nsub=2, dmode=1, tpw=8, twt=8, pipe=0, splits=12),
       cin=20, cout=24, k=(5, 5, 5), pad=(2, 2, 1), odims=(9, 10, 24), op='wgrad', tr='pre', accumulate=True),
    _c('g_n1_d2_p4_w8', dict(nsub=1, dmode=2, tpw=4, twt=8, pipe=1, boxskip=1, splits=8),
       B=2, cin=13, cout=2, k=(7, 7, 7), pad=(3, 3, 3), odims=(9, 10, 8), op='wgrad', geom='convT', yview='s2d', tr='post', boxes='geom'),
    _c('g_n2_d2_p4_w8', dict(nsub=2, dmode=2, tpw=4, twt=8, pipe=0, boxskip=1, n_groups=8, splits=8),
       B=2, cin=12, cout=3, k=(7, 7, 7), pad=(3, 3, 3), odims=(9, 10, 8), op='wgrad', geom='convT', yview='s2d', tr='pre', accumulate=True, boxes='geom'),
    # ---- weight-gradient edges
    _c('g_boxes_odd', dict(nsub=2, dmode=2, tpw=4, boxskip=0, n_groups=0), B=2, cin=13, cout=20, k=(4, 4, 4), pad=P4, odims=(5, 9, 16),
       op='wgrad', yview='co', tr='pre', boxes='odd'),
    _c('g_convT_noboxes', dict(nsub=1, dmode=2, tpw=4, boxskip=0), B=2, cin=12, cout=2, k=(7, 7, 7), pad=(3, 3, 3), odims=(5, 9, 16),
       op='wgrad', geom='convT', yview='s2d', tr='pre'),
    _c('g_633_noinherit', dict(nsub=2, dmode=1, tpw=4, twt=16, inherit=0), B=2, cin=13, cout=24, k=(6, 3, 3), pad=(2, 1, 1),
       odims=(9, 9, 16), op='wgrad', tr='pre'),
    _c('g_633_w8_inherit', dict(nsub=2, dmode=2, tpw=4, twt=8, inherit=1), B=2, cin=13, cout=24, k=(6, 3, 3), pad=(2, 1, 1),
       odims=(9, 10, 8), op='wgrad', yview='co', tr='pre'),
    _c('g_178', dict(nsub=2, dmode=1, tpw=4, twt=16), B=2, cin=13, cout=24, k=(1, 7, 8), pad=(0, 3, 3), odims=(5, 9, 16), op='wgrad', tr='pre'),
    _c('g_255', dict(nsub=2, dmode=1, tpw=4, twt=16), B=2, cin=13, cout=24, k=(2, 5, 5), pad=(1, 2, 2), odims=(5, 9, 16), op='wgrad', tr='pre'),
    _c('g_288', dict(nsub=1, dmode=1, tpw=8, twt=16), B=2, cin=13, cout=12, k=(2, 8, 8), pad=(0, 3, 4), odims=(5, 9, 16), op='wgrad', tr='pre'),
    _c('g_splits1', dict(nsub=2, dmode=1, tpw=4, splits=1, per_split=4), cin=264, cout=128, k=(4, 4, 4), pad=P4, odims=(5, 9, 16), op='wgrad'),
    _c('g_splits_between', dict(nsub=2, dmode=1, tpw=8, splits=4, per_split=2, chunks=8), B=2, cin=136, cout=64, k=(5, 5, 5), pad=P5,
       odims=(5, 9, 16), op='wgrad', tr='pre'),
    _c('g_det', dict(nsub=2, dmode=1, tpw=8, splits=1, per_split=8), B=2, cin=13, cout=24, k=(5, 5, 5), pad=P5, odims=(5, 9, 16),
       op='wgrad', tr='pre', deterministic=True),
    _c('g_cin1', dict(nsub=1, dmode=1, tpw=8, twt=16), B=2, cin=1, cout=16, k=(5, 5, 5), pad=P5, odims=(5, 9, 16), op='wgrad'),
    _c('g_pad0_xbig', dict(nsub=2, dmode=1, tpw=4, twt=16), B=2, cin=12, cout=24, k=(4, 4, 4), pad=(0, 0, 0), odims=(5, 9, 16),
       xdims=(8, 12, 20), op='wgrad', tr='pre', accumulate=True),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------------------ inputs
def build(c: Case):
  """The seeded CPU tensors of a case (conv_fp32_cases.build) plus what only this engine takes: the slab image of the packed
  weights, one bias row per sample, and for a fuse row the norm's saved statistics / input."""
  b = K32.build(c)
  g = t.Generator().manual_seed(K32.zlib.crc32(c.name.encode()) ^ 0x5bf3)
  b.slab = None
  if c.op == "fwd":                     # (every forward row has both forms of its weights: the GPU module compares them)
    geo = b.geo
    desc, blocks = G.operand_table([(0, 0, geo, True)])
    b.slab = t.zeros(G.slab_entries(geo) * 32, dtype=t.uint8)
    _EMU.bf3_operands(b.wp, (t.as_tensor(desc), blocks), b.slab)
  sample_bias(b, g)
  if c.fuse == "bnbwd":                 # the BatchRenorm whose output gradient y is: its input (before the ReLU) and mu, rstd, r, d
    S = c.odims[0] * c.odims[1] * c.odims[2]
    b.bn_x = t.randn(c.B * b.ycout * S + 4, generator=g)
    b.bn_saved = t.cat([t.rand(b.ycout, generator=g) * 0.4, 1.0 / (t.rand(b.ycout, generator=g) * 0.5 + 0.3),
                        t.rand(b.ycout, generator=g) * 0.5 + 0.75, t.randn(b.ycout, generator=g) * 0.1]).contiguous()
  return b


def sample_bias(b, g):
  """Sets b.bias_sB, and for a bias_b row replaces the shared bias row by one row per sample (bias_sB = Npad)."""
  b.bias_sB = 0
  if b.case.bias_b:                     # rows of [B][Npad]; columns past Cout are never read for a real output
    b.bp = t.randn(b.case.B, b.npad, generator=g)
    b.bp[:, b.ycout:] = 0
    b.bias_sB = b.npad


def bias_logical(b, dtype=t.float64):
  if b.bp is None: return 0.0
  if b.case.bias_b: return b.bp[:, :b.ycout].to(dtype).view(b.case.B, -1, 1, 1, 1)
  return b.bp[:b.ycout].to(dtype).view(1, -1, 1, 1, 1)


def expected_y(b, conv_part, bias_times=1, accumulate=None):
  """float64 storage the call must leave: y0 outside the view, (y0 +) bias + conv inside."""
  acc = b.case.accumulate if accumulate is None else accumulate
  st = b.y0.double().clone()
  write_logical(yview(b, st), conv_part + bias_times * bias_logical(b), acc)
  return st


# ------------------------------------------------------------------------------------------------ the split model
def _split(v):
  """hi = bf16(v), lo = bf16(v - hi) of a float32 tensor, as float32 (round to nearest even, as split8 of csrc/bf3_common.h)."""
  hi = v.to(t.bfloat16).float()
  return hi, (v - hi).to(t.bfloat16).float()


def _x_operand(b):
  """T(x), zero-padded, in float32 with the kernel's roundings (multiply, then add: the library is built without contraction)."""
  xt = K32._transformed(b, K32.logical_x(b, t.float32))
  return F.pad(xt, K32._pads(b, xt, b.pad_lo))


def split_fwd(b, acc=t.float64, terms=(("h", "h"), ("h", "l"), ("l", "h")), lo_keep=None, wp=None):
  """The engine's arithmetic from the words of csrc/conv_bf3.hip's header, independent of kernel_contract_emu's conv path:
  both operands split into two bf16 terms, y = hi*hi + hi*lo + lo*hi, every product exact, summed in `acc` (float64: the split
  model; float32: the same with a float32 accumulator in torch's order).  Logical [B, ycout, D, H, W], no bias.
  terms / lo_keep (0/1 per input channel: whose lo term of x takes part): the knobs the sensitivity test turns."""
  xh, xl = _split(_x_operand(b))
  if lo_keep is not None: xl = xl * lo_keep.view(1, -1, 1, 1, 1)
  wk = (b.wp if wp is None else wp).view(b.ycin, *b.window, b.npad).permute(4, 0, 1, 2, 3)
  wh, wl = _split(wk)
  X = {"h": xh.to(acc), "l": xl.to(acc)}
  W = {"h": wh.to(acc).contiguous(), "l": wl.to(acc).contiguous()}
  y = None
  for a, w_ in terms:
    p = F.conv3d(X[a], W[w_])
    y = p if y is None else y + p
  return y[:, :b.ycout]


def split_wgrad(b, acc=t.float64):
  """The same for the weight gradient: T(x) and dy split, dw = hi*hi + hi*lo + lo*hi summed over samples and positions; packed
  [cin][T][npad] (every column past dy->C zero)."""
  xh, xl = _split(_x_operand(b))
  dh, dl = _split(logical(yview(b, b.dys)))
  corr = lambda a, d: F.conv3d(a.to(acc).transpose(0, 1).contiguous(), d.to(acc).transpose(0, 1).contiguous())    # [cin, cout, kd, kh, kw]
  gw = corr(xh, dh) + corr(xh, dl) + corr(xl, dh)
  out = t.zeros(b.ycin, b.window[0] * b.window[1] * b.window[2], b.npad, dtype=acc)
  out[:, :, :b.ycout] = gw.permute(0, 2, 3, 4, 1).reshape(b.ycin, -1, b.ycout)
  return out.reshape(-1)


# ------------------------------------------------------------------------------------------------ references
class FwdRef:
  """float64 reference of a forward row, computed once (torch's own operator on doubles, conv_fp32_cases.ref_fwd_logical), the
  split model of the same call, and the share of the error bars that belongs to the references themselves."""

  def __init__(self, b):
    conv = K32.ref_fwd_logical(b)
    self.conv = conv
    self.mask = inside_mask(b.case.yview, b.case.B, b.ycout, b.case.odims)
    self.want = expected_y(b, conv)
    self.range = float((conv + bias_logical(b)).abs().max())
    s64 = split_fwd(b)
    self.want_split = expected_y(b, s64)
    self.split_vs_f64 = float((s64 - conv).abs().max()) / self.range           # the reference's share of BAR
    self.f32_vs_split = float((split_fwd(b, t.float32).double() - s64).abs().max()) / self.range

  def check(self, b, got):
    """-> (max error inside the view against float64 / range, the same against the split model, outside bit-identical)."""
    got = got.detach().cpu()
    return (K32.err_inside(got, self.want, self.mask, self.range), K32.err_inside(got, self.want_split, self.mask, self.range),
            K32.outside_equal(got, b.y0, self.mask))


class WgradRef:
  def __init__(self, b):
    self.grad = K32.ref_wgrad_packed(b)                                       # autograd on doubles, in the packed layout
    self.real = K32.real_entries(b)
    self.range = float(self.grad.abs().max())
    base = b.dw0.double() if b.case.accumulate else 0.0
    self.want = self.grad + base
    s64 = split_wgrad(b)
    self.want_split = s64 + base
    self.split_vs_f64 = float((s64 - self.grad).abs()[self.real].max()) / self.range
    self.f32_vs_split = float((split_wgrad(b, t.float32).double() - s64).abs()[self.real].max()) / self.range

  def check(self, b, got):
    """-> (max error over the real entries against float64 / range, against the split model, the columns past dy->C right: no
    workgroup may add to them, so a zero_first call leaves 0 there and an accumulating one the bits it found.  Entries of real
    columns at structural zeros of a transposed convolution hold whatever the window correlation gives, or are skipped under tap
    boxes: not looked at, the un-pack never reads them)."""
    got = got.detach().cpu()
    pad = (t.arange(b.npad) >= b.ycout).expand(b.ycin, got.numel() // (b.ycin * b.npad), b.npad).reshape(-1)
    pad_ok = bool(t.equal(got[pad], b.dw0[pad])) if b.case.accumulate else bool((got[pad] == 0).all())
    return (K32.err_inside(got, self.want, self.real, self.range), K32.err_inside(got, self.want_split, self.real, self.range),
            pad_ok)


def make_ref(b):
  return FwdRef(b) if b.case.op == "fwd" else WgradRef(b)


# ------------------------------------------------------------------------------------------------ running and checking
WS_BYTES = lambda b: b.ycout * 4096 * 16          # room for 4096 parts per channel (the table's launches have 8 or 16)
NDSUM = 5


def fuse_request(b, ws, dsum=None, x=None, saved=None):
  """The crnBnBwdFuse of a fuse row over the given device (or CPU) buffers, its `decline` twist applied."""
  from corenet_amd import _lib
  c = b.case
  S = c.odims[0] * c.odims[1] * c.odims[2]
  f = _lib.CrnBnBwdFuse()
  f.pre_relu = 1
  f.ws, f.ws_bytes = ws.data_ptr(), ws.numel() * ws.element_size()
  if c.decline == "ws_short": f.ws_bytes = b.ycout * parts_of(c) * 16 - 1
  if c.fuse == "bnbwd":
    f.x, f.sB_x, f.saved = x.data_ptr(), b.ycout * S, saved.data_ptr()
    f.dsum, f.ndsum = dsum.data_ptr(), NDSUM
    if c.decline == "ndsum": f.ndsum = 513
    if c.decline == "x_misaligned": f.x = x.data_ptr() + 4
    if c.decline == "sB_x": f.sB_x = b.ycout * S + 2
  return f


def parts_of(c):
  """Workgroups along x of the row's launch = partial sums per channel of a fused epilogue."""
  td, th, tw = (4, 8, 16) if c.odims[2] % 16 == 0 else (8, 8, 8)
  return c.B * -(-c.odims[0] // td) * -(-c.odims[1] // th) * -(-c.odims[2] // tw)


def query_plan(be, b, xs, ys, wp, dw=None, slab=None, fuse=None):
  """The plan of the case's call on these storages (be: HipBackend; any device, CPU included)."""
  c = b.case
  tr = transform_of(b, xs.device)
  if c.op == "fwd":
    return be.conv_fwd_bf3_plan(xview(b, xs), tr, wp, b.npad, None if b.bp is None else wp, b.bias_sB, yview(b, ys), b.window,
                                b.pad_lo, c.accumulate, boxes=b.boxes, wslab=slab, fuse=fuse)
  return be.conv_wgrad_bf3_plan(xview(b, xs), tr, yview(b, ys), dw, b.npad, b.window, b.pad_lo, not c.accumulate, boxes=b.boxes)


def run_fwd(be, b, dev, slabs=None):
  """The case's crn_conv_fwd_bf3 / crn_conv_fwd_bf3_slabs call on device dev -> the output storage.  slabs: overrides the row's
  form of the weights."""
  c = b.case
  use_slab = c.slabs if slabs is None else slabs
  y = b.y0.to(dev).clone()
  _fwd_call(be, b, dev, y, b.slab.to(dev) if use_slab else None)
  return y


def _fwd_call(be, b, dev, y, slab):
  import ctypes as C
  from corenet_amd import _lib
  from corenet_amd.backend import _cview, _ctr, _ctapboxes
  c = b.case
  xs = b.xs.to(dev)
  wp = b.wp.to(dev)
  bp = None if b.bp is None else b.bp.to(dev)
  fn = be.lib.crn_conv_fwd_bf3_slabs if slab is not None else be.lib.crn_conv_fwd_bf3
  fn(C.byref(_cview(xview(b, xs))), _ctr(transform_of(b, dev)), slab.data_ptr() if slab is not None else wp.data_ptr(), b.npad,
     None if bp is None else bp.data_ptr(), b.bias_sB, C.byref(_cview(yview(b, y))), *b.window, *b.pad_lo, int(c.accumulate),
     _ctapboxes(b.boxes), _lib.stream())


def run_wgrad(be, b, dev):
  c = b.case
  dw = b.dw0.to(dev).clone()
  be.conv_wgrad(xview(b, b.xs.to(dev)), transform_of(b, dev), yview(b, b.dys.to(dev)), dw, b.npad, b.window, b.pad_lo,
                not c.accumulate, boxes=b.boxes, math="bf16x3")
  return dw


# ------------------------------------------------------------------------------------------------ rejections
def rejections(accepted=False):
  """[(what is wrong, fwd | wgrad, make(dev))]: the good call -- B 1, 8 -> 16 channels, a 4^3 window with pads 1 on plain views of
  (4, 8, 16) -- with ONE thing wrong per row, one row per rejection of bf3_fwd_select / bf3_wg_select (csrc/conv_bf3.hip).
  make(dev) -> dict(args: the C arguments without w (forward) and without the stream, w, out: the output storage, full of
  SENTINEL).  Unreachable, hence no row: both LDS bounds (see the table's comment).  accepted=True: the accepted calls next to
  them instead (the good call itself and the nearest shape on the other side of a bound)."""
  import ctypes as C
  from corenet_amd import _lib
  from corenet_amd.backend import _cview

  def mk(op, dev, B=1, xB=None, cin=8, cout=16, npad=16, k=(4, 4, 4), pad=(1, 1, 1), dims=(4, 8, 16), xd=None, xkind="plain",
         ykind="plain", boxes=None):
    xd = xd or dims
    xs = t.zeros(view_numel(xkind, xB or B, cin, xd) + 8, device=dev)
    ys = t.full((view_numel(ykind, B, cout, dims) + 8,), SENTINEL if op == "fwd" else 0.5, device=dev)
    xv, yv = _cview(make_view(xkind, xs, xB or B, cin, xd)), _cview(make_view(ykind, ys, B, cout, dims))
    tb = None
    if boxes is not None:
      tb = _lib.CrnTapBoxes(); tb.n_groups, tb.c_groups = boxes
    bx = None if tb is None else C.cast(C.pointer(tb), C.c_void_p)
    w = t.zeros(64, device=dev)
    if op == "fwd":
      return dict(args=(C.byref(xv), None, npad, None, 0, C.byref(yv), *k, *pad, 0, bx), w=w.data_ptr(), out=ys, keep=(xs, xv, yv, tb, w))
    dw = t.full((8 * 256 * 32,), SENTINEL, device=dev)
    return dict(args=(C.byref(xv), None, C.byref(yv), dw.data_ptr(), npad, *k, *pad, 1, bx), w=None, out=dw, keep=(xs, ys, xv, yv, tb))

  R, A = [], []
  ok = lambda name, op, **kw: A.append((f"{op}: {name}", op, lambda dev, op=op, kw=kw: mk(op, dev, **kw)))
  add = lambda name, op, **kw: R.append((f"{op}: {name}", op, lambda dev, op=op, kw=kw: mk(op, dev, **kw)))
  for op in ("fwd", "wgrad"):
    add("tap-box groups 9", op, boxes=(9, 0))
    add("tap-box groups -1", op, boxes=(0, -1))
    add("Npad 24", op, npad=24)
    add("batch mismatch", op, xB=2)
    add("x base off by 4 bytes", op, xkind="off1")
    add("x odd W", op, xd=(4, 8, 15))
    add("W 24 on a D of 4" if op == "wgrad" else "W 24", op, dims=(4, 8, 24))
    add("W 12", op, dims=(8, 8, 12))
    add("H 7", op, dims=(4, 7, 16))
    add("W 16 D 3", op, dims=(3, 8, 16))
    add("W 8 D 7", op, dims=(7, 8, 8))
    add("5x5 planes with kd 8: 1320 staging units", op, k=(8, 5, 5), pad=(3, 2, 2))
    add("5^3 with an odd pw on 16-wide tiles: 1056 staging units", op, k=(5, 5, 5), pad=(2, 2, 1))
  add("y->C 17 > Npad", "fwd", cout=17)
  add("Cin 513", "fwd", cin=513)
  add("W 8 H 9", "fwd", dims=(8, 9, 8))
  add("window planes of 9 taps", "fwd", k=(3, 3, 3))
  add("window planes of 30 taps", "fwd", k=(4, 5, 6), pad=(1, 2, 2))
  add("window planes of 20 taps", "fwd", k=(4, 4, 5), pad=(1, 1, 2))
  add("kd 9", "fwd", k=(9, 4, 4), pad=(4, 1, 1), dims=(8, 8, 8))
  add("Cin*T*Npad = 2^29", "fwd", cin=512, npad=8192, k=(8, 4, 4), pad=(3, 1, 1), dims=(8, 8, 8))
  add("stride-2 x under 5x5 planes", "fwd", xkind="s2co", k=(5, 5, 5), pad=(2, 2, 2))
  add("x with stride 2 and no channel table", "fwd", xkind="s2")
  add("dy base off by 4 bytes", "wgrad", ykind="off1")
  add("dy with stride 2 and no channel table", "wgrad", ykind="s2")
  add("x with stride 2", "wgrad", xkind="s2co")
  add("14 tap pairs: 2 per wave", "wgrad", k=(3, 3, 3))
  add("75 tap pairs: 10 per wave", "wgrad", k=(6, 5, 5), pad=(2, 2, 2), dims=(8, 8, 8))
  add("5^3 window on a stride-2 dy: no kernel with 8 pairs per wave", "wgrad", k=(5, 5, 5), pad=(2, 2, 2), ykind="co")
  add("4^3 window on a plain dy with W 8: no such kernel", "wgrad", dims=(8, 8, 8))
  ok("the good call", "fwd"); ok("the good call", "wgrad")
  ok("tap-box groups 8", "fwd", boxes=(8, 8)); ok("tap-box groups 8", "wgrad", boxes=(8, 8))
  ok("W 24 on a D of 8", "wgrad", k=(5, 5, 5), pad=(2, 2, 2), dims=(8, 8, 24))
  ok("W 8 H 10", "fwd", dims=(8, 10, 8))
  ok("5x5 planes with kd 5", "fwd", k=(5, 5, 5), pad=(2, 2, 2)); ok("5^3", "wgrad", k=(5, 5, 5), pad=(2, 2, 2))
  ok("5^3 with an odd pw on 8-wide tiles", "fwd", k=(5, 5, 5), pad=(2, 2, 1), dims=(8, 8, 8))
  ok("y->C 16 = Npad", "fwd", cout=16); ok("Cin 512", "fwd", cin=512)
  ok("kd 8", "fwd", k=(8, 4, 4), pad=(3, 1, 1), dims=(8, 8, 8))
  ok("Cin*T*Npad = 2^28", "fwd", cin=512, npad=4096, k=(8, 4, 4), pad=(3, 1, 1), dims=(8, 8, 8))
  ok("stride-2 x under 4x4 planes", "fwd", xkind="s2co")
  ok("4^3 window on a stride-2 dy with W 8", "wgrad", dims=(8, 8, 8), ykind="co")
  ok("4^3 window on a stride-2 dy", "wgrad", ykind="co")
  ok("5^3 window on a plain dy with W 8", "wgrad", k=(5, 5, 5), pad=(2, 2, 2), dims=(8, 8, 8))
  return A if accepted else R

