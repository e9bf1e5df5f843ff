"""Topology of voxel grids: the histogram of 2x2x2 voxel configurations and what is linear in it (volume, exposed faces,
Euler characteristic, a Crofton surface area), and the Betti numbers b0 (pieces), b1 (handles, tunnels), b2 (cavities).

configuration_histogram counts, for N grids, how often each of the 256 configurations of 2x2x2 neighbouring voxels
occurs.  CUDA(HIP) tensors run the kernel of csrc/voxel_topology.hip, CPU tensors the library's host twin
(csrc/voxel_topology_cpu.cpp).  Both give the same tensors exactly; a CUDA tensor never goes to the host twin.

Contract:
  * grid: [N, D, H, W], N independent grids; every voxel outside a grid is background.  Rank other than 4 raises
    ValueError, so does an empty extent -- except that N == 0 returns empty results -- and D*H*W > 2^31 - 1.  W stride 1
    (a view with another W stride is copied first), N / D / H strides arbitrary.
  * Cell (d, h, w), 0 <= d <= D, 0 <= h <= H, 0 <= w <= W, holds the eight voxels (d - 1 + i, h - 1 + j, w - 1 + k),
    i, j, k in {0, 1}; for a mask X its code is the sum of X << (4 i + 2 j + k).  A grid has (D + 1)(H + 1)(W + 1) cells,
    every voxel lies in 8 of them, an axis-adjacent pair of voxels in 4, a face-diagonal pair in 2, a body-diagonal pair
    in 1.
  * table: int64 [N, L + 1, 256] with L = num_labels.  Row 0 counts the mask value != 0 (any object), row l the mask
    value == l.  Every row sums to the number of cells.  bad: int64 [N], the voxels with value < 0 or value > L; they
    are background everywhere else.
  * bool and floating grids are the mask grid > 0 (NaN is background) with L = 0 and nothing bad; they take no
    num_labels.  uint8 and int32 grids are taken as they are, other integer types become int32.  num_labels=None on an
    integer grid is the call's maximum clamped at 0: one extra pass and one read-back.  num_labels above
    topology_tiles().max_labels raises ValueError: the rows of a workgroup live in LDS.
  * Integer adds only: identical from run to run and between GPU and host twin; nothing depends on
    crn_set_deterministic.  The kernels are queued on the current stream.

Everything derived from the table is exact in int64 and runs in torch on the table's device."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, NamedTuple, Optional, Tuple

import torch as t

_MAX_VOXELS = (1 << 31) - 1
_CHUNK_BYTES = 1 << 30

# Voronoi weights of the 13 lattice directions, per direction: 3 axes, 6 face diagonals, 4 body diagonals
CROFTON_WEIGHTS = (2 * 0.04577789120476, 2 * 0.03698062787608, 2 * 0.03519563978232)
assert abs(3 * CROFTON_WEIGHTS[0] + 6 * CROFTON_WEIGHTS[1] + 4 * CROFTON_WEIGHTS[2] - 1.0) < 1e-12


class ConfigHistogram(NamedTuple):
  table: t.Tensor             # i64 [N, L + 1, 256]
  bad: t.Tensor               # i64 [N]


class Betti(NamedTuple):
  b0: t.Tensor                # i64 [N, L + 1] pieces
  b1: t.Tensor                # i64 [N, L + 1] handles / tunnels
  b2: t.Tensor                # i64 [N, L + 1] cavities
  chi: t.Tensor               # i64 [N, L + 1] b0 - b1 + b2


class TopologyTiles(NamedTuple):
  brick_d: int                # a workgroup owns brick_d x brick_h x brick_w cells
  brick_h_int32: int
  brick_h_uint8: int
  brick_w: int
  max_labels: int
  batch: int                  # grids per launch


def _lib():
  from corenet_amd import _lib as L
  return L.lib()


def topology_tiles() -> TopologyTiles:
  out = (C.c_int32 * 6)()
  _lib().crn_voxel_topology_tiles(C.addressof(out))
  return TopologyTiles(*(int(x) for x in out))


def _build_luts() -> Dict[str, t.Tensor]:
  pos = [(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)]
  bit = {p: 4 * p[0] + 2 * p[1] + p[2] for p in pos}
  pairs = {1: [], 2: [], 3: []}                                             # by the number of coordinates that differ
  for a in pos:
    for b in pos:
      if bit[a] < bit[b]:
        pairs[sum(x != y for x, y in zip(a, b))].append((bit[a], bit[b]))
  assert [len(pairs[n]) for n in (1, 2, 3)] == [12, 12, 4]
  halves = [[bit[p] for p in pos if p[axis] == side] for axis in range(3) for side in (0, 1)]      # also the 6 faces of the cell
  names = ("popcount", "axis_mixed", "face_diag_mixed", "body_diag_mixed", "chi26_x8", "chi6_x8")
  lut = {n: [0] * 256 for n in names}
  for c in range(256):
    b = [(c >> p) & 1 for p in range(8)]
    pop = sum(b)
    lut["popcount"][c] = pop
    for name, n in (("axis_mixed", 1), ("face_diag_mixed", 2), ("body_diag_mixed", 3)):
      lut[name][c] = sum(b[p] != b[q] for p, q in pairs[n])
    e = sum(any(b[p] for p in h) for h in halves)
    f = sum(b[p] | b[q] for p, q in pairs[1])
    lut["chi26_x8"][c] = 8 * (c != 0) - 4 * e + 2 * f - pop
    both = sum(b[p] & b[q] for p, q in pairs[1])
    full = sum(all(b[p] for p in h) for h in halves)
    lut["chi6_x8"][c] = pop - 2 * both + 4 * full - 8 * (c == 255)
  return {n: t.tensor(v, dtype=t.int64) for n, v in lut.items()}


_LUTS = _build_luts()


def lookup_tables() -> Dict[str, t.Tensor]:
  """The 256-entry int64 tables over the cell codes: popcount; axis_mixed / face_diag_mixed / body_diag_mixed, the pairs
  of that kind (12, 12, 4 per cell) whose voxels differ; chi26_x8 and chi6_x8, eight times the cell's share of the Euler
  characteristic of the complex of closed voxels (26-connectivity) and of the complex of voxel centres, 6-adjacent pairs,
  full 2x2 squares and full 2x2x2 blocks (6-connectivity)."""
  return {n: v.clone() for n, v in _LUTS.items()}


def _dot(table: t.Tensor, name: str) -> t.Tensor:
  table = t.as_tensor(table)
  if table.dtype != t.int64 or table.dim() < 1 or table.shape[-1] != 256:
    raise ValueError(f"expected an int64 table [..., 256], got {table.dtype} {tuple(table.shape)}")
  return (table * _LUTS[name].to(table.device)).sum(-1)


def _exact_div(x: t.Tensor, k: int, what: str) -> t.Tensor:
  assert bool((x % k == 0).all()), f"{what}: the table is not the histogram of a grid"
  return x // k


def volume(table) -> t.Tensor:
  """The number of voxels of every row."""
  return _exact_div(_dot(table, "popcount"), 8, "volume")


def exposed_faces(table) -> t.Tensor:
  """The number of voxel faces between the mask and its complement, the border of the grid included."""
  return _exact_div(_dot(table, "axis_mixed"), 4, "exposed_faces")


def euler_characteristic(table, connectivity: int = 26) -> t.Tensor:
  """The Euler characteristic of every row under 26- or 6-connectivity."""
  if connectivity not in (6, 26):
    raise ValueError(f"euler_characteristic: connectivity must be 6 or 26, got {connectivity}")
  return _exact_div(_dot(table, "chi26_x8" if connectivity == 26 else "chi6_x8"), 8, "euler_characteristic")


def crofton_area(table, voxel_size=1.0) -> t.Tensor:
  """float64 surface area of every row from the intersection counts along the 13 lattice directions (Crofton formula with
  Voronoi weights): voxel_size^2 * 2 * (c1 nA + c2 nF / sqrt 2 + c3 nB / sqrt 3).  voxel_size: a number or a tensor that
  broadcasts against table[..., 0]."""
  nA = _exact_div(_dot(table, "axis_mixed"), 4, "crofton_area").to(t.float64)
  nF = _exact_div(_dot(table, "face_diag_mixed"), 2, "crofton_area").to(t.float64)
  nB = _dot(table, "body_diag_mixed").to(t.float64)
  c1, c2, c3 = CROFTON_WEIGHTS
  size = t.as_tensor(voxel_size, dtype=t.float64).to(nA.device)
  return size * size * 2.0 * (c1 * nA + c2 * nF / math.sqrt(2.0) + c3 * nB / math.sqrt(3.0))


def _check(grid: t.Tensor, what: str):
  if grid.dim() != 4:
    raise ValueError(f"{what} expects a rank-4 grid [N, D, H, W], got shape {tuple(grid.shape)}")
  N, D, H, W = grid.shape
  if grid.device.type not in ("cuda", "cpu"):
    raise ValueError(f"{what}: unsupported device {grid.device}")
  if N and (D == 0 or H == 0 or W == 0):
    raise ValueError(f"{what}: empty grid extent {tuple(grid.shape)}")
  if D * H * W > _MAX_VOXELS:
    raise ValueError(f"{what}: grid of {D}x{H}x{W} too large (at most 2^31 - 1 voxels per grid)")


def _prepare(grid: t.Tensor, num_labels, what: str) -> Tuple[t.Tensor, int, bool]:
  """(the uint8 / int32 tensor with W stride 1 the library takes, L, whether it is a mask grid)."""
  if grid.dtype.is_complex:
    raise ValueError(f"{what}: complex grids have no foreground")
  mask = grid.dtype == t.bool or grid.dtype.is_floating_point
  if mask:
    if num_labels not in (None, 0):
      raise ValueError(f"{what}: a {grid.dtype} grid is a mask (grid > 0) and takes no num_labels, got {num_labels}")
    grid, L = (grid > 0).to(t.uint8), 0
  else:
    if grid.dtype not in (t.uint8, t.int32):
      grid = grid.to(t.int32)
    if num_labels is None:
      L = max(int(grid.max()), 0) if grid.numel() else 0                     # the extra pass and the read-back
    else:
      if int(num_labels) != num_labels or num_labels < 0:
        raise ValueError(f"{what}: num_labels must be a non-negative integer, got {num_labels}")
      L = int(num_labels)
    cap = topology_tiles().max_labels
    if L > cap:
      raise ValueError(f"{what}: {L} labels, at most {cap} (max_labels) are counted per call")
  if grid.stride(-1) != 1:
    grid = grid.contiguous()
  return grid, L, mask


def _histogram(grid: t.Tensor, L: int, mask: bool) -> ConfigHistogram:
  N, D, H, W = grid.shape
  dev = grid.device
  table = t.empty((N, L + 1, 256), dtype=t.int64, device=dev)
  bad = t.empty((N,), dtype=t.int64, device=dev)
  if N == 0:
    return ConfigHistogram(table, bad)
  if grid.is_cuda:
    from corenet_amd.backend import default_backend
    default_backend().voxel_topology(grid, L, mask, table, bad)
  else:
    from corenet_amd.backend import _DTYPE_CODE
    st = (C.c_int64 * 4)(*grid.stride())
    _lib().crn_voxel_topology_cpu(grid.data_ptr(), st, _DTYPE_CODE[grid.dtype], N, D, H, W, L, int(mask), table.data_ptr(),
                                  bad.data_ptr(), t.get_num_threads())
  return ConfigHistogram(table, bad)


def configuration_histogram(grid, num_labels: Optional[int] = None) -> ConfigHistogram:
  """The configuration histogram of N grids (see the module docstring for the contract)."""
  grid = t.as_tensor(grid)
  _check(grid, "configuration_histogram")
  grid, L, mask = _prepare(grid, num_labels, "configuration_histogram")
  return _histogram(grid, L, mask)


def _betti(grid: t.Tensor, L: int, mask: bool, connectivity: int, chunk_bytes: int) -> Tuple[Betti, ConfigHistogram]:
  from corenet_amd.voxel_components import component_stats, connected_components
  N, D, H, W = grid.shape
  dev = grid.device
  hist = _histogram(grid, L, mask)
  chi = euler_characteristic(hist.table, connectivity)
  dual = 6 if connectivity == 26 else 26
  if mask:
    lab = grid
  else:
    lab = t.where((grid < 0) | (grid > L), t.zeros_like(grid), grid) if grid.dtype == t.int32 else t.where(grid > L, t.zeros_like(grid), grid)
  b0 = t.zeros((N, L + 1), dtype=t.int64, device=dev)
  b2 = t.zeros((N, L + 1), dtype=t.int64, device=dev)
  if N:
    b0[:, 0] = connected_components(lab, connectivity, by_value=False).num_components
    if L:
      comps = connected_components(lab, connectivity, by_value=True)
      stats = component_stats(comps, lab)
      K = stats.value.numel()
      g = t.repeat_interleave(t.arange(N), stats.offsets[1:] - stats.offsets[:-1], output_size=K).to(dev)
      b0.view(-1).index_add_(0, g * (L + 1) + stats.value.to(t.int64), t.ones(K, dtype=t.int64, device=dev))
    # the cavities of mask (n, l): the components of its complement in the padded grid, less the one outside
    per_mask = 10 * (D + 2) * (H + 2) * (W + 2)                               # the mask, its int32 labels, the workspace
    step = max(1, int(chunk_bytes) // per_mask)
    M = N * (L + 1)
    rows = t.arange(L + 1, device=dev, dtype=lab.dtype)
    for m0 in range(0, M, step):
      idx = t.arange(m0, min(m0 + step, M), device=dev)
      n, l = idx // (L + 1), rows[idx % (L + 1)][:, None, None, None]
      fg = t.where(l == 0, lab[n] != 0, lab[n] == l)
      comp = t.ones((idx.numel(), D + 2, H + 2, W + 2), dtype=t.uint8, device=dev)
      comp[:, 1:-1, 1:-1, 1:-1] = (~fg).to(t.uint8)
      b2.view(-1)[idx] = connected_components(comp, dual, by_value=False).num_components - 1
  b1 = b0 + b2 - chi
  assert bool((b1 >= 0).all()), "betti_numbers: negative b1"
  return Betti(b0, b1, b2, chi), hist


def betti_numbers(grid, connectivity: int = 26, num_labels: Optional[int] = None, _chunk_bytes: int = _CHUNK_BYTES) -> Betti:
  """(b0, b1, b2, chi), int64 [N, L + 1] each, of the masks of configuration_histogram's rows.  Foreground connectivity
  26 pairs with background connectivity 6, and 6 with 26: b0 is the number of components of the mask
  (voxel_components.connected_components; the label rows from one by_value call), b2 the number of components of its
  complement under the dual connectivity in the grid padded by one voxel, minus the one that holds the padding, and
  b1 = b0 + b2 - chi.  The complements of the N (L + 1) masks are labelled in chunks of at most _chunk_bytes."""
  if connectivity not in (6, 26):
    raise ValueError(f"betti_numbers: connectivity must be 6 or 26, got {connectivity}")
  grid = t.as_tensor(grid)
  _check(grid, "betti_numbers")
  grid, L, mask = _prepare(grid, num_labels, "betti_numbers")
  return _betti(grid, L, mask, connectivity, _chunk_bytes)[0]
