"""The ray-traced skip connection (csrc/ray_sample.hip: crn_ray_sample_fwd, crn_ray_sample_fwd_idx, crn_ray_project,
crn_ray_sample_bwd_idx, crn_ray_sample_bwd) on the GPU, every row of tests/ray_cases.py.  Indices and gathers bit for bit against
the oracle's index arithmetic; scatters against float64 index_add_ within the derived bound of tests/ray_cases.py
((n_p + 3) 2^-24 A_p + n_p 2^-43 max|dout| per element), bit-equal on integer-valued gradients, bit-identical between two runs in
deterministic mode, and the two entry points within the bound of each other.  Inputs hold NaN wherever their view does not
reach, outputs start at a sentinel or at random contents: whatever the output view does not address must come back bit-identical.
tests/test_ray_sample_plan_cpu.py shows that every row reaches the dispatch paths it names."""
import functools
import os
import time

import pytest
import torch as t

import ray_cases as K
from ray_cases import CASES, BY_NAME

pytestmark = pytest.mark.gpu

DEV = "cuda"
_DET_ENV = os.environ.get("CRN_DETERMINISTIC", "0") == "1"
MAXRATIO = {}          # path -> largest err / bound of the rows that name it


@pytest.fixture(scope="module")
def be():
  t0 = time.time()
  from corenet_amd.backend import HipBackend
  assert t.cuda.is_available(), "gpu tests need an MI355X"
  yield HipBackend()
  print("\nray scatter, largest err / bound per path (bound: (n_p + 3) 2^-24 A_p + n_p 2^-43 max|dout|)")
  for p in sorted(MAXRATIO):
    print(f"  {p:28s} {MAXRATIO[p]:.3f}")
  print(f"  module wall time {time.time() - t0:.1f} s")


@functools.lru_cache(maxsize=None)
def built(name, grad=None):
  return K.build(BY_NAME[name], grad)


@functools.lru_cache(maxsize=None)
def indices(name):
  return K.ref_indices(BY_NAME[name])[0]


@functools.lru_cache(maxsize=None)
def want_fwd(name):
  return K.want_fwd(BY_NAME[name], built(name), indices(name))


def _bits(a):
  return a.view(t.int32) if a.dtype == t.float32 else a


@pytest.mark.parametrize("name", [c.name for c in CASES if c.op == "fwd"])
def test_forward_case(be, name):
  """crn_ray_sample_fwd_idx, crn_ray_sample_fwd and crn_ray_project: the whole out and idx storages bit for bit (the view holds the
  reference, the rest the sentinel)."""
  c, b = BY_NAME[name], built(name)
  want_out, want_idx = want_fwd(name)
  out, ist = K.run_fwd(be, c, b, DEV, with_idx=True)
  assert t.equal(K.idx_view(c, ist), K.idx_view(c, want_idx)), f"{name}: the saved index tensor differs from the oracle's indices"
  assert t.equal(ist, want_idx), f"{name}: index elements outside the view changed"
  assert t.equal(_bits(K.out_view(c, out)), _bits(K.out_view(c, want_out))), f"{name}: the gather differs from the oracle's"
  assert t.equal(_bits(out), _bits(want_out)), f"{name}: output elements outside the view changed"
  out2, ist2 = K.run_fwd(be, c, b, DEV, with_idx=False)
  assert t.equal(_bits(out2), _bits(want_out)), f"{name}: crn_ray_sample_fwd differs"
  assert t.equal(ist2, b.idx_st)
  assert t.equal(K.run_project(be, c, b, DEV), want_idx), f"{name}: crn_ray_project differs from the oracle's indices"
  if c.same_as:
    a = BY_NAME[c.same_as]
    oa, ia = K.run_fwd(be, a, built(c.same_as), DEV, with_idx=True)
    assert t.equal(_bits(K.out_view(c, out)), _bits(K.out_view(a, oa))) and t.equal(K.idx_view(c, ist), K.idx_view(a, ia)), \
        f"{name}: not the bits of the aligned call {c.same_as}"


def _note(c, ratio, tag):
  for p in c.paths:
    MAXRATIO[p] = max(MAXRATIO.get(p, 0.0), ratio)
  print(f"{c.name} ({tag}): err / bound {ratio:.3f}")


@pytest.mark.parametrize("name", [c.name for c in CASES if c.op == "scatter"])
def test_scatter_case(be, name):
  c, b = BY_NAME[name], built(name)
  idx = indices(name)
  ref = K.ScatterRef(c, b, idx)
  entries = ("idx", "plain") if c.entry == "both" else ("plain",)
  be.set_deterministic(c.deterministic)
  try:
    got = {}
    for e in entries:
      st = got[e] = K.run_scatter(be, c, b, DEV, e, idx)
      ratio, kinds, rest = ref.check(c, b, st)
      _note(c, ratio, e)
      assert kinds, f"{name} ({e}): the positions or kinds of the non-finite outputs differ from index_add_'s"
      assert rest, f"{name} ({e}): elements outside the dmap view changed"
      assert ratio <= 1.0, f"{name} ({e}): {ratio:.3f} of the bound"
      if c.deterministic:
        again = K.run_scatter(be, c, b, DEV, e, idx)
        assert t.equal(_bits(again), _bits(st)), f"{name} ({e}): two deterministic runs differ"
    if len(got) == 2:          # the entry points agree to the same bound
      a, p = K.dmap_view(c, got["idx"]).double(), K.dmap_view(c, got["plain"]).double()
      f = t.isfinite(a) & t.isfinite(p)
      assert bool(((a - p).abs()[f] <= ref.bound.expand_as(a)[f]).all()), f"{name}: the two entry points differ by more than the bound"
      if c.deterministic:
        assert t.equal(_bits(got["idx"]), _bits(got["plain"])), f"{name}: the deterministic entry points differ"
    if c.grad == "randn":      # integer-valued gradients, also times 2^40 and 2^-40: every sum is exact on every path
      for ex in (0, 40, -40):
        bi = K.scaled(built(name, "int"), ex)
        ri = K.ScatterRef(c, bi, idx)
        for e in entries:
          st = K.run_scatter(be, c, bi, DEV, e, idx)
          assert ri.exact(c, st), f"{name} ({e}): integer gradients x 2^{ex} are not summed exactly"
          assert ri.check(c, bi, st)[2], f"{name} ({e}): elements outside the dmap view changed"
  finally:
    be.set_deterministic(_DET_ENV)
