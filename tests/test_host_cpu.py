"""CPU tests of the host side: conv geometries (views + packed weights) against
torch.nn.functional, the complete forward/backward plan of engine.py against the
oracle in float64 (far below fp32 rounding noise), and the C ABI surface."""
import ctypes
import subprocess
import os

import numpy as np
import pytest
import torch as t
import torch.nn.functional as F

from oracle import corenet_oracle as O
from kernel_contract_emu import EmuBackend
from corenet_amd import views as V
from corenet_amd.model import conv_geometry as G

EMU = EmuBackend()
DT = t.float64


def pack(w, index):
  out = t.zeros(len(index), dtype=w.dtype)
  EMU.gather(w.reshape(-1), t.as_tensor(index), out)
  return out


def err(a, b):
  return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("k,p", [(7, 3), (3, 1)])
def test_convtranspose_as_window_correlation(k, p):
  g = t.Generator().manual_seed(k)
  B, Cin, Cout, D = 2, 5, 3, 6
  x = t.randn(B, Cin, D, D, D, generator=g, dtype=DT)
  w = t.randn(Cin, Cout, k, k, k, generator=g, dtype=DT)
  bias = t.randn(Cout, generator=g, dtype=DT)
  fwd, dgr = G.convt_fwd(w.shape, p), G.convt_dgrad(w.shape, p)
  y = t.zeros(B, Cout + 2, 2 * D, 2 * D, 2 * D, dtype=DT)
  yv = V.space_to_depth_view(V.view_of(y).channels(0, Cout), (2, 2, 2), parity_major=True)
  EMU.conv_fwd(V.view_of(x), None, pack(w, fwd.index), fwd.npad, pack(bias, G.bias_index(Cout, 8, fwd.npad, parity_major=True)), 0,
               yv, fwd.window, fwd.pad_lo)
  ref = F.conv_transpose3d(x, w, bias, stride=2, padding=p, output_padding=1)
  assert err(y[:, :Cout], ref) < 1e-12 and float(y[:, Cout:].abs().max()) == 0
  dy = t.randn(ref.shape, generator=g, dtype=DT)
  dyb = t.zeros_like(y); dyb[:, :Cout] = dy
  dyv = V.space_to_depth_view(V.view_of(dyb).channels(0, Cout), (2, 2, 2), parity_major=True)
  dx = t.zeros_like(x)
  EMU.conv_fwd(dyv, None, pack(w, dgr.index), dgr.npad, None, 0, V.view_of(dx), dgr.window, dgr.pad_lo)
  xr = x.clone().requires_grad_(True); wr = w.clone().requires_grad_(True)
  F.conv_transpose3d(xr, wr, None, stride=2, padding=p, output_padding=1).backward(dy)
  assert err(dx, xr.grad) < 1e-12
  dw = t.zeros(len(fwd.index), dtype=DT)
  EMU.conv_wgrad(V.view_of(x), None, dyv, dw, fwd.npad, fwd.window, fwd.pad_lo, True)
  gw = t.zeros(w.numel(), dtype=DT); EMU.scatter(dw, t.as_tensor(fwd.index), gw)
  assert err(gw.view(w.shape), wr.grad) < 1e-12
  # the forward pack index is injective on the reference weight (doubles as the un-pack scatter)
  valid = fwd.index[fwd.index >= 0]
  assert len(np.unique(valid)) == len(valid) == w.numel()


def test_conv_stem_strided_and_1to4():
  g = t.Generator().manual_seed(1)
  x = t.randn(2, 3, 20, 20, generator=g, dtype=DT); w = t.randn(8, 3, 7, 7, generator=g, dtype=DT)
  geo = G.stem_fwd(w.shape, 3)
  y = t.zeros(2, 8, 10, 10, dtype=DT)
  EMU.conv_fwd(V.space_to_depth_view(V.view_of(x), (1, 2, 2)), None, pack(w, geo.index), geo.npad, None, 0,
               V.view_of(y), geo.window, geo.pad_lo)
  assert err(y, F.conv2d(F.pad(x, [3, 3, 3, 3]), w, None, stride=2)) < 1e-12
  x = t.randn(2, 6, 8, 8, generator=g, dtype=DT); w = t.randn(5, 6, 1, 1, generator=g, dtype=DT)
  geo, dgeo = G.conv_fwd(w.shape, 0), G.conv_dgrad(w.shape, 0)
  y = t.zeros(2, 5, 4, 4, dtype=DT)
  EMU.conv_fwd(V.strided_view(V.view_of(x), (1, 2, 2)), None, pack(w, geo.index), geo.npad, None, 0, V.view_of(y),
               geo.window, geo.pad_lo)
  assert err(y, F.conv2d(x, w, None, stride=2)) < 1e-12
  dy = t.randn(y.shape, generator=g, dtype=DT); dx = t.zeros_like(x)
  EMU.conv_fwd(V.view_of(dy), None, pack(w, dgeo.index), dgeo.npad, None, 0, V.strided_view(V.view_of(dx), (1, 2, 2)),
               dgeo.window, dgeo.pad_lo, accumulate=True)
  xr = x.clone().requires_grad_(True); F.conv2d(xr, w, None, stride=2).backward(dy)
  assert err(dx, xr.grad) < 1e-12
  x = t.randn(3, 7, generator=g, dtype=DT); w = t.randn(7, 4, 4, 4, 4, generator=g, dtype=DT)
  geo = G.convt_1to4_fwd(w.shape)
  y = t.zeros(3, 4, 4, 4, 4, dtype=DT)
  EMU.conv_fwd(V.view_of(x.view(3, 7, 1, 1, 1)), None, pack(w, geo.index), geo.npad, None, 0,
               V.flat_channel_view(V.view_of(y)), geo.window, geo.pad_lo)
  assert err(y, F.conv_transpose3d(x.view(3, 7, 1, 1, 1), w, None, stride=4)) < 1e-12


def test_conv3d_k5_dgrad_geometry():
  g = t.Generator().manual_seed(2)
  x = t.randn(1, 4, 6, 6, 6, generator=g, dtype=DT); w = t.randn(3, 4, 5, 5, 5, generator=g, dtype=DT)
  dgeo = G.conv_dgrad(w.shape, 2)
  dy = t.randn(1, 3, 6, 6, 6, generator=g, dtype=DT); dx = t.zeros_like(x)
  EMU.conv_fwd(V.view_of(dy), None, pack(w, dgeo.index), dgeo.npad, None, 0, V.view_of(dx), dgeo.window, dgeo.pad_lo)
  xr = x.clone().requires_grad_(True); F.conv3d(xr, w, None, padding=2).backward(dy)
  assert err(dx, xr.grad) < 1e-12


def test_engine_plan_matches_oracle_fp64():
  """Whole forward + loss + backward plan (views, packs, fused BN transforms, skips,
  residuals, scatter of packed grads) vs the oracle, float64, r/d clamps active."""
  from corenet_amd.model.engine import Engine, LOSS_KINDS
  t.set_num_threads(min(8, os.cpu_count() or 1))
  B, C = 1, 2
  eng = Engine(C, device="cpu", backend=EmuBackend(), dtype=DT)
  sd = O.make_state(0, C, nbt=30000)
  for k, v in sd.items():
    eng.store.view(k).copy_(v)
  image, v2s, off, grid = O.synthetic_batch(B, 0, C)
  plan = eng.plan(B)
  logits = plan.forward(image, v2s, off, training=True)
  s = {k: (v.detach().clone().to(DT) if v.dtype == t.float32 else v.clone()) for k, v in sd.items()}
  for k in s:
    if s[k].dtype == DT and "running" not in k:
      s[k].requires_grad_(True)
  feats, avg = O.resnet50_features(O.preprocess_image_caffe(image).to(DT), s, True)
  lo = O.decoder_forward(feats, avg, s, v2s, off, (128, 128, 128), True)
  assert err(logits, lo.detach()) < 1e-6
  O.iou_fgbg(grid, lo).backward()
  plan.gt.copy_(grid.to(t.int32))
  eng.be.loss_fwd_bwd(LOSS_KINDS["iou_fgbg"], plan.logits, plan.gt, B, C, 128 ** 3, plan.loss, plan.glogits, 1.0)
  plan.backward(plan.glogits)
  for k, v in s.items():
    if v.grad is None or k.endswith("conv.bias") or k.endswith("c1.bias"):
      continue          # biases feeding a train-mode BatchRenorm have zero true gradient
    gmax = float(v.grad.abs().max())
    if gmax < 1e-14:
      continue
    assert err(eng.store.view(k, grad=True), v.grad) < 1e-5, k
  for k in ("decoder.stage_6.b1.running_mean", "encoder.stage5.c.op_c.bn.running_var"):
    assert float((eng.store.view(k) - s[k]).abs().max()) < 1e-8
  assert int(eng.store.view("decoder.stage_1.b1.num_batches_tracked")) == 30001
  # bucketed backward (overlapped gradient exchange): every bucket handed to the hook is already final when
  # the hook runs, the buckets tile the slab from the top down, and the slab ends up identical
  ref = eng.store.grads.clone()
  eng.store.grads.fill_(float("nan"))
  seen = []
  plan.backward(plan.glogits, grad_hook=lambda g: seen.append((g.storage_offset(), g.clone())))
  assert t.equal(eng.store.grads.nan_to_num(0.0), ref.nan_to_num(0.0))
  hi = ref.numel()
  assert len(seen) == len(eng.grad_buckets) >= 6
  for off, g in seen:
    assert off + g.numel() == hi and t.equal(g.nan_to_num(0.0), ref[off:hi].nan_to_num(0.0))
    hi = off
  assert hi == 0


def test_autograd_path_with_fused_adam_two_steps():
  """The reference's train loop body (pipeline.py:224-230: zero_grad, forward, loss, backward, step) through the
  drop-in's autograd node + FusedAdam, over the contract emulator: two steps must land on the parameters of two
  fused `train_step`s (the gradient slab is reused by every backward, so `.grad` must never alias it: ADVICE r1),
  gradient accumulation adds up, and a backward whose forward was overwritten raises instead of returning
  gradients of the wrong activations."""
  from corenet_amd import state as S
  from corenet_amd.model.core_net import CoreNet, CoreNetConfig, DecoderConfig
  t.set_num_threads(min(8, os.cpu_count() or 1))
  sd = O.make_state(0, 2, nbt=0)
  cfg = CoreNetConfig(DecoderConfig((128, 128, 128), 2, 2, 64, 0.75))
  ma, mb = (CoreNet(cfg, device="cpu", backend=EmuBackend()) for _ in range(2))
  ma.load_state_dict(sd); mb.load_state_dict(sd)
  ma.train(); mb.train()
  image, v2s, off, grid = O.synthetic_batch(1, 0, 2)
  opt = S.FusedAdam(ma, lr=4e-4, eps=1e-4)
  for step in range(2):
    opt.zero_grad()
    loss = O.iou_fgbg(grid, ma(image, v2s, off))
    loss.backward()
    opt.step()
    # the gradients are views of ONE slab-shaped tensor: step() moves them with a single copy (the test on
    # `._base` never fired, AccumulateGrad detaches), and zero_grad() of the second iteration zeroes that tensor once
    assert opt.gather_copies == 1
    lb = mb.train_step(image, v2s, off, grid.to(t.int32), "iou_fgbg", lr=4e-4, adam_eps=1e-4)
    assert abs(float(loss) - float(lb)) < 1e-5 * abs(float(lb)), (step, float(loss), float(lb))
  pa, pb = ma.engine.store.params, mb.engine.store.params
  # Adam moves every parameter by <= lr per step; 2x gradients on step 2 would not change m/sqrt(v) by much, so
  # compare the first moments too (they are linear in the gradient)
  assert float((pa - pb).abs().max()) < 1e-6
  assert float((ma.engine.adam_m - mb.engine.adam_m).abs().max()) <= 1e-5 * float(mb.engine.adam_m.abs().max())
  # .grad does not alias the slab
  g = ma.get_parameter("decoder.stage_6.t1.weight").grad
  assert g.data_ptr() != ma.engine.store.view("decoder.stage_6.t1.weight", grad=True).data_ptr()
  # gradient accumulation (no zero_grad in between): g1 + g2
  g1 = g.clone()
  loss = O.iou_fgbg(grid, ma(image, v2s, off)); loss.backward()
  g12 = ma.get_parameter("decoder.stage_6.t1.weight").grad
  opt.zero_grad(set_to_none=True)
  loss = O.iou_fgbg(grid, ma(image, v2s, off)); loss.backward()
  g2 = ma.get_parameter("decoder.stage_6.t1.weight").grad
  assert float((g12 - (g1 + g2)).abs().max()) <= 1e-5 * float(g12.abs().max())
  # no per-step growth of the plan's view cache (one pinned glogits tensor per step)
  n_views = len(ma.engine.plan(1)._views)
  loss = O.iou_fgbg(grid, ma(image, v2s, off)); loss.backward()
  assert len(ma.engine.plan(1)._views) == n_views
  # stale forward
  l1 = O.iou_fgbg(grid, ma(image, v2s, off))
  with t.no_grad():
    ma(image, v2s, off)
  with pytest.raises(RuntimeError, match="overwritten"):
    l1.backward()


def test_c_abi_surface():
  """The shared library loads (no GPU needed) and exports every symbol of include/corenet_hip.h."""
  import re
  from corenet_amd import _lib, build as B
  if not os.path.exists(B.LIB):
    B.build(verbose=False)
  lib = ctypes.CDLL(B.LIB)
  hdr = open(os.path.join(os.path.dirname(B.HERE), "include", "corenet_hip.h")).read()
  tools_block = re.search(r"#ifdef CRN_TOOLS.*?#endif", hdr, re.S).group(0)     # tuning aids: tools build only
  declared = set(re.findall(r"\b(crn_[a-z0-9_]+)\s*\(", hdr.replace(tools_block, "")))
  assert declared == set(_lib.ALL_SYMBOLS), declared ^ set(_lib.ALL_SYMBOLS)
  for sym in declared:
    getattr(lib, sym)
  # the drop-in surface is ALL the product library exports: no probe, no stamp read-backs
  exported = set(subprocess.run(["nm", "-D", "--defined-only", B.LIB], capture_output=True, text=True, check=True).stdout.split())
  assert {s for s in exported if s.startswith("crn_")} == declared
  assert set(re.findall(r"\b(crn_[a-z0-9_]+)\s*\(", tools_block)) == set(_lib.TOOL_SYMBOLS)
  lib.crn_version.restype = ctypes.c_char_p
  assert b"gfx950" in lib.crn_version()


def test_product_has_no_cpu_fallback():
  """corenet_amd never imports the oracle / emulator, and CPU tensors are rejected."""
  import corenet_amd.cc.fill_voxels as fv
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  for dp, _, files in os.walk(os.path.join(root, "corenet_amd")):
    for f in files:
      if f.endswith(".py"):
        src = open(os.path.join(dp, f)).read()
        import re
        assert not re.search(r"^\s*(from|import)\s+(oracle|kernel_contract_emu|tests)\b", src, re.M), f
  with pytest.raises(ValueError):
    fv.fill_inside_voxels_gpu(t.zeros(1, 2, 2, 2))


def test_fill_inside_voxels_cpu_operator():
  """The boundary's host operator `fill_inside_voxels_cpu` (cc/module.cc:24-29, fill_voxels_cpu.cc:158-183), the
  library's own C++ (crn_fill_voxels_cpu): the reference's grid1/grid2 vectors (voxelization_test.py:152-214),
  bit-exact against the C oracle on random grids of every dispatched dtype, the CPU-only semantics (reached voxels
  keep their input value: SURVEY Q10 probe `[0.5,-3,0,2] -> [1,-3,0,1]`), clone ownership and the ValueErrors."""
  import fill_oracle_c
  from reference_known_answers import fill_grids
  from corenet_amd.cc import fill_voxels as fv
  g1, g2, e1, e2 = fill_grids()
  got = fv.fill_inside_voxels_cpu(t.tensor(np.stack([g1, g2])))
  np.testing.assert_array_equal(got.numpy(), np.stack([e1, e2]))
  rng = np.random.RandomState(3)
  for shape in ((3, 5, 6, 7), (2, 33, 31, 65), (1, 9, 9, 130), (5, 24, 40, 64), (2, 7, 7, 7), (1, 3, 200, 3)):
    for dens in (0.2, 0.45, 0.7):
      g = (rng.rand(*shape) < dens).astype(np.float32)
      g[0].flat[::7] = -3.0                                    # non-positive values count as empty
      want = np.where(fill_oracle_c.fill(g) == 0, g, 1)        # oracle: GPU {0,1} semantics -> CPU semantics
      for dt in (t.float32, t.float64, t.int32, t.int64, t.int16, t.int8):
        x = t.tensor(g).to(dt)
        keep = x.clone()
        out = fv.fill_inside_voxels_cpu(x)
        assert out.dtype == dt and out.data_ptr() != x.data_ptr() and t.equal(x, keep)
        np.testing.assert_array_equal(out.numpy(), want.astype(out.numpy().dtype))
      u = t.tensor(np.maximum(g, 0)).to(t.uint8)
      np.testing.assert_array_equal(fv.fill_inside_voxels_cpu(u).numpy(), fill_oracle_c.fill(g).astype(np.uint8))
  assert fv.fill_inside_voxels_cpu(t.tensor([0.5, -3, 0, 2]).reshape(1, 1, 1, 4)).flatten().tolist() == [1, -3, 0, 1]
  nc = t.tensor(g).permute(0, 1, 3, 2)                         # non-contiguous input: cloned contiguous
  np.testing.assert_array_equal(fv.fill_inside_voxels_cpu(nc).numpy(),
                                np.where(fill_oracle_c.fill(nc.contiguous().numpy()) == 0, nc.numpy(), 1))
  with pytest.raises(ValueError):
    fv.fill_inside_voxels_cpu(t.zeros(2, 2, 2))
  assert fv.fill_inside_voxels_cpu(t.zeros(0, 4, 4, 4)).shape == (0, 4, 4, 4)


def test_get_module_is_shaped_like_corenet_cpp():
  """`corenet.cc.fill_voxels.get_module()` returns the extension module `corenet_cpp` and its two callers are written
  against that object (cc/fill_voxels.py:98-107: `get_module().fill_inside_voxels_cpu(grid)`,
  `get_module().fill_inside_voxels_gpu(grid, inplace)`; cc/module.cc:18-29).  The same two statements run verbatim on
  what `corenet_amd.cc.fill_voxels.get_module()` returns; the C-ABI library is its `.lib`."""
  from reference_known_answers import fill_grids
  from corenet_amd.cc import fill_voxels as fv
  from corenet_amd import _lib
  mod = fv.get_module()
  assert mod is fv.get_module(verbose=True)                      # one module object per process, like the reference's global
  assert callable(mod.fill_inside_voxels_gpu) and callable(mod.fill_inside_voxels_cpu)
  assert mod.lib is _lib.lib()
  g1, g2, e1, e2 = fill_grids()
  grid = t.tensor(np.stack([g1, g2]))
  np.testing.assert_array_equal(mod.fill_inside_voxels_cpu(grid).numpy(), np.stack([e1, e2]))   # cc/fill_voxels.py:99
  with pytest.raises(ValueError):
    mod.fill_inside_voxels_gpu(grid, False)                      # :107 on a CPU tensor: the op's own ValueError
  with pytest.raises(ValueError):
    mod.fill_inside_voxels_gpu(grid, inplace=True)
  with pytest.raises(ValueError):
    mod.fill_inside_voxels_cpu(grid[0])                          # rank 3


def test_tap_boxes_cover_every_real_weight():
  """crnTapBoxes contract (include/corenet_hip.h): for output group g (forward geometry) / input group g
  (data-gradient geometry) every packed weight with a tap OUTSIDE the box is a structural zero (index -1),
  and the boxes are tight.  k=7 -> 343 = (4+3)^3 real taps out of 8 * 4^3."""
  from corenet_amd.model import conv_geometry as G
  for wshape, pad in (((16, 16, 7, 7, 7), 3), ((32, 2, 7, 7, 7), 3), ((8, 32, 3, 3, 3), 1)):
    cin, cout = wshape[0], wshape[1]
    fwd, dgr = G.convt_fwd(wshape, pad), G.convt_dgrad(wshape, pad)
    nw = fwd.window[0]
    assert len(fwd.n_boxes) == 8 and not fwd.c_boxes and len(dgr.c_boxes) == 8 and not dgr.n_boxes
    fi = fwd.index.reshape(cin, nw, nw, nw, fwd.npad)[..., :8 * cout].reshape(cin, nw, nw, nw, 8, cout)
    di = dgr.index.reshape(8, cout, nw, nw, nw, dgr.npad)[..., :cin]
    vol = 0
    for g in range(8):
      d0, d1, h0, h1, w0, w1 = fwd.n_boxes[g]
      inside = np.zeros((nw, nw, nw), bool); inside[d0:d1, h0:h1, w0:w1] = True
      real = (fi[:, :, :, :, g, :] >= 0)
      assert (real == inside[None, :, :, :, None]).all()          # exactly the box, for every (c, n)
      vol += inside.sum()
      d0, d1, h0, h1, w0, w1 = dgr.c_boxes[g]
      inside = np.zeros((nw, nw, nw), bool); inside[d0:d1, h0:h1, w0:w1] = True
      assert ((di[g] >= 0) == inside[None, :, :, :, None]).all()
    assert vol == wshape[2] ** 3                                    # every kernel tap appears exactly once
    # both packings address every parameter exactly once
    for idx in (fwd.index, dgr.index):
      v = np.sort(idx[idx >= 0])
      assert (v == np.arange(np.prod(wshape))).all()


def test_checkpoint_interop_and_fused_adam():
  """N4: a checkpoint in the reference's format (state.py:74-97: torch.save of global_step,
  model_state, model_config, optimizer_state = torch.optim.Adam.state_dict(), extra_metadata) loads into the
  drop-in; the fused optimizer continues exactly where torch.optim.Adam would; encode -> decode round-trips."""
  import io
  from corenet_amd import state as S
  from corenet_amd.model.core_net import CoreNet, CoreNetConfig, DecoderConfig
  sd = O.make_state(3, 2, nbt=7)
  keys = list(sd.keys())
  pkeys = [k for k in keys if sd[k].dtype == t.float32 and "running" not in k]
  # what the reference would have saved after two Adam steps on these parameters
  g = t.Generator().manual_seed(11)
  params = [sd[k].clone().requires_grad_(True) for k in pkeys]
  opt = t.optim.Adam(params, lr=4e-4, eps=1e-4)
  for _ in range(2):
    for p in params: p.grad = t.randn(p.shape, generator=g) * 0.01
    opt.step()
  model_state = {k: (params[pkeys.index(k)].detach().clone() if k in pkeys else sd[k].clone()) for k in keys}
  cfg = {"decoder": {"resolution": (128, 128, 128), "num_output_channels": 2, "last_upscale_factor": 2,
                     "latent_channels": 64, "skip_fraction": 0.75}}
  buf = io.BytesIO()
  t.save({"global_step": 1234, "model_state": model_state, "model_config": cfg, "optimizer_state": opt.state_dict(),
          "extra_metadata": {"note": "ref"}}, buf)
  st = S.decode_state(buf.getvalue(), "cpu", backend=EMU)
  assert st.global_step == 1234 and st.extra_metadata == {"note": "ref"}
  assert [k for k, _ in st.model.named_parameters()] == pkeys            # torch's positional optimizer state needs this
  got = st.model.state_dict()
  assert list(got.keys()) == keys and all(t.equal(got[k], model_state[k]) for k in keys)
  assert st.model.engine.adam_t == 2
  # one more step: fused Adam (kernel contract) vs torch.optim.Adam continuing from the same state
  grads = [t.randn(p.shape, generator=g) * 0.01 for p in params]
  for p, gr in zip(params, grads): p.grad = gr
  opt.step()
  for k, gr in zip(pkeys, grads): st.model.engine.store.view(k, grad=True).copy_(gr)
  st.optimizer.step()
  for k, p in zip(pkeys, params):
    assert float((st.model.state_dict()[k] - p.detach()).abs().max()) < 1e-6, k
  # our own checkpoint: same format, round trip, and the saved optimizer state is torch.optim.Adam's
  raw = S.encode_state(st)
  d = t.load(io.BytesIO(raw), weights_only=False)
  assert set(d) == {"global_step", "model_state", "model_config", "optimizer_state", "extra_metadata"}
  opt2 = t.optim.Adam([p.detach().clone().requires_grad_(True) for p in params], lr=1.0)
  opt2.load_state_dict(d["optimizer_state"])                             # loads into the reference's optimizer
  assert opt2.param_groups[0]["lr"] == 4e-4 and opt2.param_groups[0]["eps"] == 1e-4
  ref_sd = opt.state_dict()
  for i in range(len(pkeys)):
    assert float((d["optimizer_state"]["state"][i]["exp_avg"] - ref_sd["state"][i]["exp_avg"]).abs().max()) < 1e-7
    assert float((d["optimizer_state"]["state"][i]["exp_avg_sq"] - ref_sd["state"][i]["exp_avg_sq"]).abs().max()) < 1e-9
    assert int(d["optimizer_state"]["state"][i]["step"]) == 3
  st2 = S.decode_state(raw, "cpu", backend=EMU)
  assert st2.model.engine.adam_t == 3 and all(t.equal(st2.model.state_dict()[k], st.model.state_dict()[k]) for k in keys)


def test_bf3_operand_layouts_round_trip():
  """The two pre-arranged weight formats of crn_bf3_operands as include/corenet_hip.h describes them, on the CPU:
  an entry = 8 bf16 hi + 8 bf16 lo of 8 consecutive input channels (w = hi + lo, hi = bf16(w));  encoder operand
  blocks: entry ((cb*T + t)*(Npad/16) + ntile)*64 + kk*16 + i = column 16*ntile + i, tap t, channels 32*cb + 8*kk..;
  decoder slabs: entry ((chunk*kd + zd)*TP + tp)*Npad + n = column n, tap zd*KHW + tp, channels 8*chunk...
  The emulator writes them element by element from that text, reads them back, and a convolution on the read-back
  weights equals the convolution on the fp32 weights to the 2^-17 of the split."""
  g = t.Generator().manual_seed(3)
  # encoder engine: 3x3, 64 -> 64
  wshape = (64, 64, 3, 3)
  w = t.randn(wshape, generator=g) * 0.1
  fwd = G.conv_fwd(wshape, 1)
  wf = pack(w, fwd.index)
  assert G.operand_eligible(fwd) and G.operand_entries(fwd) == 2 * 9 * 4 * 64
  desc, blocks = G.operand_table([(0, 0, fwd)])
  assert desc.shape == (1, 7) and blocks == (G.operand_entries(fwd) + 255) // 256
  wop = t.zeros(G.operand_entries(fwd) * 32, dtype=t.uint8)
  EMU.bf3_operands(wf, (t.as_tensor(desc), blocks), wop)
  ent = wop.view(t.int16).view(t.bfloat16).view(-1, 2, 8).float()
  cb, tap, ntile, kk, i = 1, 5, 2, 3, 7                    # one entry, straight from the header's formula
  e = ((cb * 9 + tap) * 4 + ntile) * 64 + kk * 16 + i
  ref = wf.view(64, 9, 64)[32 * cb + 8 * kk:32 * cb + 8 * kk + 8, tap, 16 * ntile + i]
  assert t.equal(ent[e, 0], ref.to(t.bfloat16).float())
  assert float((ent[e, 0] + ent[e, 1] - ref).abs().max()) <= float(ref.abs().max()) * 2.0 ** -16
  x = t.randn(2, 64, 8, 8, generator=g)
  y0, y1 = t.zeros(2, 64, 8, 8), t.zeros(2, 64, 8, 8)
  EMU.conv_fwd(V.view_of(x), None, wf, fwd.npad, None, 0, V.view_of(y0), fwd.window, fwd.pad_lo)
  EMU.conv2d_bf3(V.view_of(x), None, wop, fwd.npad, None, 0, V.view_of(y1), fwd.window, fwd.pad_lo)
  assert err(y1, y0) < 2e-5
  # decoder slabs: Conv3d k5, 12 -> 16 channels (a partial chunk: zeros past Cin, 3 empty tap slots per plane)
  wshape = (16, 12, 5, 5, 5)
  w = t.randn(wshape, generator=g) * 0.05
  fwd = G.conv_fwd(wshape, 2)
  wf = pack(w, fwd.index)
  assert G.slab_entries(fwd) == 2 * 5 * 28 * 16
  desc, blocks = G.operand_table([(0, 0, fwd, True)])
  assert int(desc[0, 6]) == 25
  slabs = t.zeros(G.slab_entries(fwd) * 32, dtype=t.uint8)
  EMU.bf3_operands(wf, (t.as_tensor(desc), blocks), slabs)
  ent = slabs.view(t.int16).view(t.bfloat16).view(-1, 2, 8).float()
  chunk, zd, tp, n = 1, 3, 17, 9
  e = ((chunk * 5 + zd) * 28 + tp) * 16 + n
  ref = t.zeros(8)
  ref[:4] = wf.view(12, 125, 16)[8:12, zd * 25 + tp, n]    # channels 8..11 exist, 12..15 are zeros
  assert t.equal(ent[e, 0], ref.to(t.bfloat16).float())
  assert float(ent[((0 * 5 + 0) * 28 + 26) * 16].abs().max()) == 0.0        # tap slot 26 of a 25-tap plane
  x = t.randn(1, 12, 4, 8, 16, generator=g)
  y0, y1 = t.zeros(1, 16, 4, 8, 16), t.zeros(1, 16, 4, 8, 16)
  EMU.conv_fwd(V.view_of(x), None, wf, fwd.npad, None, 0, V.view_of(y0), fwd.window, fwd.pad_lo)
  EMU.conv_fwd(V.view_of(x), None, None, fwd.npad, None, 0, V.view_of(y1), fwd.window, fwd.pad_lo, wslab=slabs)
  assert err(y1, y0) < 2e-5


def test_mat_index_blocks_equal_tiles():
  """conv_geometry.mat_index (the LDS block copies of crn_copy_mats_f32) against tile_index on the emulator of both
  contracts: forward + data-gradient packs and the gradient un-pack of 1x1 / 3x3 / 3x3x3 / 5x5x5 layers (ragged channel
  counts included) move exactly the same elements; transposed convolutions, the stem and repeated biases are left to the
  tiles; the kernel's multiply-high reciprocals divide every element count of a block exactly."""
  def both(parts, nflat, npacked, reverse):
    d, m, ex = G.tile_index(parts)
    full = (t.as_tensor(d), t.as_tensor(m.view(np.int64)), t.as_tensor(ex if ex.size else np.zeros(1, np.int32)))
    mats, rest = G.mat_index(parts)
    d2, m2, ex2 = G.tile_index(rest)
    new = (t.as_tensor(d2), t.as_tensor(m2.view(np.int64)), t.as_tensor(ex2 if ex2.size else np.zeros(1, np.int32)),
           t.as_tensor(mats))
    g = t.Generator().manual_seed(1)
    if not reverse:
      src = t.randn(nflat, generator=g, dtype=DT)
      a, b = t.zeros(npacked, dtype=DT), t.zeros(npacked, dtype=DT)
    else:
      src = t.randn(npacked, generator=g, dtype=DT)
      a, b = t.zeros(nflat, dtype=DT), t.zeros(nflat, dtype=DT)
    EMU.copy_tiles(src, a, full, reverse); EMU.copy_tiles(src, b, new, reverse)
    assert t.equal(a, b)
    return mats, d2.shape[0]
  for shape, p in (((64, 64, 3, 3), 1), ((256, 64, 1, 1), 0), ((16, 28, 5, 5, 5), 2), ((67, 130, 3, 3), 1), ((64, 96, 3, 3, 3), 1)):
    fw, dg = G.conv_fwd(shape, p), G.conv_dgrad(shape, p)
    n = int(np.prod(shape))
    parts = [(0, fw.index, fw.npad, 0), (fw.index.size + 5, dg.index, dg.npad, dg.taps if dg.taps > 1 else 0)]
    mats, left = both(parts, n, parts[1][0] + dg.index.size, False)
    assert mats.shape[0] and not left
    both(parts[:1], n, fw.index.size, True)
    for r in mats.view(np.uint32).astype(np.int64):
      xs = np.arange(int(r[2] * r[0] * r[1]) + 1)
      for q, magic in ((r[0] * r[1], r[10]), (r[1], r[11]), (r[0], r[12])):
        assert q == 1 or np.array_equal((xs * magic) >> 32, xs // q)
  ct = G.convt_fwd((32, 16, 7, 7, 7), 3)
  for part in ((0, ct.index, ct.npad, 0), (0, G.stem_fwd().index, G.stem_fwd().npad, 0),
               (0, G.bias_index(16, 8, 128, True).astype(np.int64), 128, 0)):
    assert G.mat_index([part])[0].shape[0] == 0 and len(G.mat_index([part])[1]) == 1


def test_gradient_bars_catch_a_glitched_scatter():
  """Fault injection: the round-3/4 glitch made a few hundred of the 98 k elements of the 64^3 skip map's
  gradient wrong by up to 6 % of the map's range, in ~90 % of the training steps, and every golden test passed.  Here the same
  fault is put into the ORACLE's scatter (the gradient arriving at the compressed 64 x 64 map of rt_skip_5 is perturbed on a few
  pixel clusters) and the per-tensor bars of tests/test_model_gpu.py::test_decoder_gradients_every_element_vs_oracle are
  evaluated against the clean oracle run: the glitched run must fail them (and the clean run, compared with itself, passes)."""
  import importlib
  tm = importlib.import_module("test_model_gpu")
  z = np.load(os.path.join(os.path.dirname(__file__), "golden", "model_h7_train_b2_nbt30k.npz"))
  sd = O.make_state(0, 2, nbt=30000)
  image, v2s, off, grid = O.synthetic_batch(2, 0, 2)

  class Glitch(t.autograd.Function):
    @staticmethod
    def forward(ctx, x):
      return x.view_as(x)
    @staticmethod
    def backward(ctx, g):
      if tuple(g.shape[1:]) != (12, 64, 64):        # only the 64^3 skip's compressed map
        return g
      gen = t.Generator().manual_seed(3)
      g = g.clone()
      rng = float(g.max() - g.min())
      for _ in range(6):                            # six tiles' pixel windows, ~50 elements each: ~300 of 98 k
        b, c = int(t.randint(0, g.shape[0], (1,), generator=gen)), int(t.randint(0, 12, (1,), generator=gen))
        y0, x0 = int(t.randint(0, 56, (1,), generator=gen)), int(t.randint(0, 56, (1,), generator=gen))
        g[b, c, y0:y0 + 7, x0:x0 + 7] += (t.rand(7, 7, generator=gen) * 2 - 1) * 0.06 * rng
      return g

  def run(glitch):
    so = {k: v.clone() for k, v in sd.items()}
    for k in so:
      if so[k].dtype == t.float32 and "running" not in k: so[k].requires_grad_(True)
    orig = O.ray_sample
    if glitch:
      O.ray_sample = lambda grid2d, *a, **kw: orig(Glitch.apply(grid2d), *a, **kw)
    try:
      O.iou_fgbg(grid, O.corenet_forward(so, image, v2s, off, training=True)).backward()
    finally:
      O.ray_sample = orig
    return {k: v.grad for k, v in so.items() if v.dtype == t.float32 and v.requires_grad}

  clean, bad = run(False), run(True)
  names = tm.decoder_weight_names(clean)
  bars = tm.decoder_gradient_bars(z, names, "bf16x3")          # the LOOSER of the two modes' bars
  gmax = max(float(z[k]) for k in z.files if k.startswith("gmax::"))
  flagged = {}
  for n in names:
    scale = max(float(clean[n].abs().max()), 1e-3 * gmax)
    err = float((bad[n].double() - clean[n].double()).abs().max()) / scale
    if err > bars[n]:
      flagged[n] = err
  print("tensors over their bar with the glitch injected:", {k: f"{v:.1e}" for k, v in flagged.items()})
  assert "decoder.rt_skip_5.compress_channels.weight" in flagged, flagged


def test_no_mfma_hazard_in_the_shipped_conv_objects():
  """csrc/conv_bf3.hip issues the three products of an accumulator as one inline-asm block of MFMAs, which the compiler's hazard
  recognizer cannot see into: the wait states between such an MFMA and the next access to its destination registers are checked on
  the disassembly of the shipped objects (tools/check_mfma_hazards.py; the rules are LLVM's for the gfx940 family)."""
  import importlib.util
  from corenet_amd import build as B
  if not os.path.exists(B.LIB):
    B.build(verbose=False)
  spec = importlib.util.spec_from_file_location("check_mfma_hazards", os.path.join(os.path.dirname(B.HERE), "tools", "check_mfma_hazards.py"))
  chk = importlib.util.module_from_spec(spec); spec.loader.exec_module(chk)
  total = 0
  insts = ["conv_inst_%s_%d_%d.o" % (kind, m, n) for kind in ("fwd", "wgrad") for m, n in B.CONV_CONFIGS]
  for obj in ["conv_bf3.o", "conv_e2d.o", "conv_igemm.o", "stem_conv.o"] + insts:
    n, bad = chk.check(os.path.join(B.LIBDIR, obj))
    assert not bad, (obj, bad[:3])
    total += n
  # (the split-bf16 decoder kernels hold ~3500 MFMAs, the stem's two kernels ~700, the 18 conv engine instances ~7200)
  assert total > 10000


@pytest.mark.parametrize("hw", [(96, 160), (100, 68)])
def test_engine_plan_other_image_sizes_fp64(hw):
  """The encoder is fully convolutional (resnet50.py:176-186): a plan for another image size (96 x 160 is not square, 100 x 68
  leaves odd extents from stage 3 on; 224 x 224 and 320 x 256 run on the GPU, tests/test_model_gpu.py) must reproduce the oracle's forward, loss gradient and running statistics like the 256 x 256 plan does (float64 over the
  contract emulator: the host wiring -- buffer shapes, strides, stride-2 compaction, skip-map extents -- not the kernels)."""
  from corenet_amd.model.engine import Engine, LOSS_KINDS
  t.set_num_threads(min(8, os.cpu_count() or 1))
  B, C = 1, 2
  eng = Engine(C, device="cpu", backend=EmuBackend(), dtype=DT)
  sd = O.make_state(0, C, nbt=30000)
  for k, v in sd.items():
    eng.store.view(k).copy_(v)
  _, v2s, off, grid = O.synthetic_batch(B, 0, C)
  image = t.randint(0, 256, (B, 3) + hw, generator=t.Generator().manual_seed(5), dtype=t.uint8)
  plan = eng.plan(B, hw)
  assert plan is not eng.plan(B) and plan is eng.plan(B, hw)
  logits = plan.forward(image, v2s, off, training=True)
  s = {k: (v.detach().clone().to(DT) if v.dtype == t.float32 else v.clone()) for k, v in sd.items()}
  for k in s:
    if s[k].dtype == DT and "running" not in k:
      s[k].requires_grad_(True)
  feats, avg = O.resnet50_features(O.preprocess_image_caffe(image).to(DT), s, True)
  assert tuple(feats[3].shape[2:]) == plan.stage_hw["stage5"] and tuple(feats[0].shape[2:]) == plan.stage_hw["stage2"]
  lo = O.decoder_forward(feats, avg, s, v2s, off, (128, 128, 128), True)
  assert err(logits, lo.detach()) < 1e-6
  O.iou_fgbg(grid, lo).backward()
  plan.gt.copy_(grid.to(t.int32))
  eng.be.loss_fwd_bwd(LOSS_KINDS["iou_fgbg"], plan.logits, plan.gt, B, C, 128 ** 3, plan.loss, plan.glogits, 1.0)
  plan.backward(plan.glogits)
  for k, v in s.items():
    if v.grad is None or k.endswith("conv.bias") or k.endswith("c1.bias") or float(v.grad.abs().max()) < 1e-14:
      continue
    assert err(eng.store.view(k, grad=True), v.grad) < 1e-5, k
  with pytest.raises(ValueError):
    eng.plan(B, (250, 256))                       # not a multiple of 4
  with pytest.raises(ValueError):
    plan.forward(t.zeros(B, 3, 256, 256, dtype=t.uint8), v2s, off, training=False)     # a plan refuses other sizes
