#!/usr/bin/env python
"""Mesh clean-up (corenet_amd.mesh_ops): every native call against the obvious torch formulation on the
same tensors and against the time of copying the bytes the call has to touch.

  python tools/bench_mesh_ops.py [--iters 10] [--small]      # device-event times, JSON lines

Workloads: the marching-cubes meshes of the grids of tools/bench_mesh.py, 4 objects at 128^3 and 52 objects at 256^3;
--small leaves the second one out.

Per workload, milliseconds (median, min, max over --iters runs after two warm-up runs) of
  topology   mesh_topology, the whole call with its one read-back, against torch: a sort of the corners by vertex,
             torch.unique over the directed-edge keys for the neighbour lists and the edge counts behind `irregular`;
  taubin     one iteration (a lam and a mu step) against index_add_ over the directed edge list;
  normals    vertex_normals against cross products and three index_add_ over the faces;
  decimate   the clustering of cluster_decimate at cell 2 (tables, positions, faces: everything but the normals of the
             result) and the whole call, against torch.unique(dim=0, return_inverse=True) over the (object, cell) rows,
             index_add_ of the coordinates and the face filter.
The torch results are checked against the native ones in the same run (integers exactly, floats to 1e-4).  The floor of
a call is the bytes of its inputs and outputs over the rate of a device-to-device copy of 1 GiB measured in this run
(read plus write bytes over time)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch as t

from bench_mesh import WORKLOADS, fields


def timed(fn, iters, warm=2):
  for _ in range(warm):
    out = fn()
  t.cuda.synchronize()
  ts = []
  for _ in range(iters):
    e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    t.cuda.synchronize()
    ts.append(e0.elapsed_time(e1))
  return {"ms_median": float(np.median(ts)), "ms_min": min(ts), "ms_max": max(ts)}, out


def copy_rate(iters):
  src = t.ones(1 << 28, dtype=t.int32, device="cuda")
  dst = t.empty_like(src)
  med = timed(lambda: dst.copy_(src), iters)[0]["ms_median"]
  return 2 * src.numel() * 4 / (med * 1e-3)


def global_faces(m):
  voff = t.cumsum(m.num_vertices, 0) - m.num_vertices
  obj = t.repeat_interleave(t.arange(len(m.num_faces), device=m.faces.device), m.num_faces, output_size=m.faces.shape[0])
  return m.faces.to(t.int64) + voff[obj][:, None], obj


def torch_topology(g, V):
  src, nxt, prv = g.reshape(-1), g.roll(-1, 1).reshape(-1), g.roll(1, 1).reshape(-1)
  n = src.numel()
  vf_corners = t.sort(src * n + t.arange(n, device=g.device)).indices
  vf_offsets = t.cumsum(t.bincount(src, minlength=V), 0)
  outk, ink = src * V + nxt, src * V + prv
  pairs = t.unique(t.cat([outk, ink]))
  ko, co = t.unique(outk, return_counts=True)
  ki, ci = t.unique(ink, return_counts=True)
  nout, nin = t.zeros_like(pairs), t.zeros_like(pairs)
  nout[t.searchsorted(pairs, ko)] = co
  nin[t.searchsorted(pairs, ki)] = ci
  pv, pw = pairs // V, pairs % V
  irregular = t.zeros(V, dtype=t.bool, device=g.device)
  irregular[pv[(nout != 1) | (nin != 1) | (pv == pw)]] = True
  keep = pv != pw
  return vf_offsets, vf_corners, t.cumsum(t.bincount(pv[keep], minlength=V), 0), pv[keep], pw[keep], irregular


def torch_smooth(v, pv, pw, k, factors):
  for f in factors:
    s = t.zeros_like(v).index_add_(0, pv, v[pw])
    v = t.where(k[:, None] > 0, v + f * (s / k.clamp(min=1)[:, None] - v), v)
  return v


def torch_normals(v, g):
  a, b, c = v[g[:, 0]], v[g[:, 1]], v[g[:, 2]]
  fn = t.linalg.cross(b - a, c - a)
  n = t.zeros_like(v)
  for i in range(3):
    n.index_add_(0, g[:, i], fn)
  ln = n.norm(dim=1, keepdim=True)
  return t.where(ln > 0, n / ln.clamp(min=1e-30), t.zeros_like(n))


def torch_cluster(v, vobj, g, cell):
  rows = t.cat([vobj[:, None], t.floor(v / cell).to(t.int64)], 1)
  uniq, inv = t.unique(rows, dim=0, return_inverse=True)
  count = t.bincount(inv, minlength=uniq.shape[0])
  pos = t.zeros((uniq.shape[0], 3), dtype=v.dtype, device=v.device).index_add_(0, inv, v) / count[:, None]
  m = inv[g]
  keep = (m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 0] != m[:, 2])
  return pos, m[keep], count


def report(name, m, iters, rate):
  from corenet_amd import mesh_ops as M
  V, F = m.vertices.shape[0], m.faces.shape[0]
  g, fobj = global_faces(m)
  vobj = t.repeat_interleave(t.arange(len(m.num_vertices), device=g.device), m.num_vertices, output_size=V)
  res = {"objects": len(m.num_vertices), "vertices": V, "faces": F}

  def entry(key, native, torch_, nbytes):
    floor = nbytes / rate * 1e3
    res[key] = {"native": native, "torch": torch_, "torch_over_native": torch_["ms_median"] / native["ms_median"],
                "bytes": nbytes, "copy_floor_ms": floor, "native_over_copy_floor": native["ms_median"] / floor}

  nat, topo = timed(lambda: M.mesh_topology(m.faces, m.num_vertices, m.num_faces, total_vertices=V), iters)
  tor, ref = timed(lambda: torch_topology(g, V), iters)
  E = topo.vv_neighbours.numel()
  assert t.equal(topo.vv_offsets[1:], ref[2]) and t.equal(topo.vv_neighbours.to(t.int64), ref[4]) and t.equal(topo.irregular, ref[5])
  assert t.equal(topo.vf_offsets[1:], ref[0]) and t.equal(topo.vf_corners.to(t.int64), ref[1])
  res["neighbour_entries"] = E
  res["valence_max"] = int((topo.vv_offsets[1:] - topo.vv_offsets[:-1]).max()) if V else 0
  entry("topology", nat, tor, 12 * F + 16 * (V + 1) + 12 * F + 4 * E + V)

  k = (topo.vv_offsets[1:] - topo.vv_offsets[:-1]).to(t.float32)
  nat, sm = timed(lambda: M.taubin_smooth(m.vertices, topo, 1), iters)
  tor, sm_ref = timed(lambda: torch_smooth(m.vertices, ref[3], ref[4], k, (0.5, -0.53)), iters)
  assert t.allclose(sm, sm_ref, rtol=1e-4, atol=1e-4)
  entry("taubin_iteration", nat, tor, 12 * V + 2 * (24 * V + 8 * (V + 1) + 4 * E))          # the copy, then two steps

  nat, nrm = timed(lambda: M.vertex_normals(m.vertices, m.faces, topo), iters)
  tor, nrm_ref = timed(lambda: torch_normals(m.vertices, g), iters)
  assert t.allclose(nrm, nrm_ref, rtol=1e-4, atol=1e-4)
  entry("vertex_normals", nat, tor, 24 * V + 24 * F + 8 * (V + 1))
  del topo, ref, sm, sm_ref, nrm, nrm_ref
  t.cuda.empty_cache()

  cell = 2.0
  nat, part = timed(lambda: M._decimate_chunk(m.vertices, m.faces, m.num_vertices, m.num_faces, cell, "bench"), iters)
  full, dec = timed(lambda: M.cluster_decimate(m.vertices, m.faces, m.num_vertices, m.num_faces, cell), iters)
  tor, cl = timed(lambda: torch_cluster(m.vertices, vobj, g, cell), iters)
  V2, F2 = dec.meshes.vertices.shape[0], dec.meshes.faces.shape[0]
  assert cl[0].shape[0] == V2 and cl[1].shape[0] == F2 and t.equal(t.sort(cl[2]).values, t.sort(dec.cluster_size.to(t.int64)).values)
  res["decimated_vertices"], res["decimated_faces"] = V2, F2
  entry("decimate_clustering", nat, tor, 12 * V + 12 * F + 4 * V + 16 * V2 + 12 * F2)
  res["decimate_whole_call"] = dict(full, torch_over_native=tor["ms_median"] / full["ms_median"])
  print(json.dumps({name: res}), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--iters", type=int, default=10)
  ap.add_argument("--small", action="store_true")
  args = ap.parse_args()
  if not t.cuda.is_available():
    raise SystemExit("bench_mesh_ops needs a GPU: it measures the kernels")
  from corenet_amd import mesh_ops as M
  from corenet_amd.visualization import marching_cubes
  rate = copy_rate(args.iters)
  print(json.dumps({"tiles": M.mesh_ops_tiles()._asdict(), "iters": args.iters, "copy_rate_TBps_this_run": rate / 1e12}), flush=True)
  for name, n, size in WORKLOADS:
    if args.small and size == 256:
      continue
    m = marching_cubes(fields(n, size, seed=7))
    t.cuda.empty_cache()
    report(name, m, args.iters, rate)
    del m
    t.cuda.empty_cache()


if __name__ == "__main__":
  main()
