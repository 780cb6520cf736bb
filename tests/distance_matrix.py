"""Which compiled instances a call of the n x n squared-distance pass runs (csrc/gram_bf16.hip, csrc/pairwise.hip),
seeded stacks that reach every one of them, and the float64 reference they are held to (a helper module, not a
conftest; the column kernels' counterpart is tests/instance_matrix.py).

One call of `gars.pairwise_sqdist` runs, invisibly to the caller,
  * one Gram kernel `gram3_partial_kernel<K, NPL, ALIGNED>`: K = ceil(n / 4), NPL = 3 bf16 planes below 2^20 total
    coordinates and 2 from there on, a 16-byte-aligned form with a condition-free steady-state loop that a wave only
    enters when it owns more than 2 NSETS - 1 whole chunks, and an unaligned form;
  * the reduction of the partial Gram matrices in 1..8 slices, whose last workgroup forms the distances and lists the
    rows of nearly coincident pairs (the accuracy gate), and ranks the rows when asked to and nothing is listed;
  * the direct-difference kernel on the listed rows, with the geometry (strips, slots) of THEIR count, decided on the
    device — or, under BM_PAIR_MODE=1, on the whole stack.

Three parts:
  * a mirror of those rules: `instances(case, cus)`; tests/test_distance_matrix_cpu.py holds its constants and
    expressions to the sources and the case lists below to every instance the sources can reach;
  * seeded stacks on the GPU, cut out of one flat allocation at byte offsets 0 / 4 / 8 / mixed by
    `instance_matrix.place` (the same values at every offset; aliased rows are the same tensor object);
  * the float64 direct-difference reference and the suite's bars (tests/pair_mode_check.py: every off-diagonal squared
    distance within 1e-5 of the float64 value relative to itself, a bitwise symmetric matrix with a zero diagonal,
    exact zeros between aliased rows and bitwise-equal distances from them to every third row;
    tests/test_gpu_parity.py::test_seeded_stack_100k: 1e-6 for plain seeded stacks).

`python tests/distance_matrix.py GROUP` (with BM_* knobs in the environment) runs GROUP's cases, holds every output to
its bar and prints one JSON line: the SHA-256 of every output, the cases that missed their bar, and the worst relative
error per (form, K, NPL, bar) — how the knob tests compare a knob's instances with the defaults, one process per knob (the library
reads its knobs once per process).
"""

import hashlib
import json
import math
import os
import sys
from collections import namedtuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from tests.instance_matrix import place, row_offsets, rows_of, vec_width  # noqa: E402

DEV = "cuda:0"

# ---------------------------------------------------------------------------------------------------------------------
# Mirror of the rules (gram_bf16.hip: gram3_partials, B3Shape, b3_workgroups_per_cu, gram_finish; pairwise.hip:
# pair_geometry, pair_grid_blocks)

BM_MAX_ROWS = 64
B3_CASES = tuple(range(1, 17))   # BM_B3_CASE(K)
PLANE_THRESHOLD = 1 << 20        # total coordinates from which the split keeps two planes
K_B3_CHUNK = 64
K_B3_WAVES = 4
K_B3_MAX_BLOCKS = 1024
K_GRAM_SLICES_MAX = 8
GRAM_SLICE_WORKGROUPS = 64       # slices = 64 / chunks of 64 entries ...
GRAM_SLICE_MIN_BLOCKS = 32       # ... with at least 32 partial blocks each
PAIR_CAND = ((2, 8), (4, 8), (8, 8), (1, 16), (2, 16), (4, 16))
K_PAIR_MAX_THREADS = 512
PAIR_LDS_LIMIT = 32 * 1024
K_DMA_BLOCK = 1024
K_DMA_PITCH = 1024 + 16
PAIR_GRID_MAX = 256 * 4
PAIR_TAU = 2e-3                  # BM_PAIR_TAU's default: a pair below tau (G_ii + G_jj) has its rows listed

DEFAULT_KNOBS = {"BM_PAIR_MODE": 0, "BM_GRAM_STEADY": 1}


def b3_workgroups_per_cu(K, NPL):
  return 3 if (K <= 6 or (K == 7 and NPL == 2) or (K == 8 and NPL == 3)) else 2


def b3_nsets(K, NPL):
  return 2 if (K <= 8 and (NPL == 2 or K * NPL <= 21)) else 1


def planes(d_total):
  return 2 if d_total >= PLANE_THRESHOLD else 3


def gram_blocks(n, d, npl, cus):
  """The grid of gram3_partials."""
  K = (n + 3) // 4
  chunks = (d + K_B3_CHUNK - 1) // K_B3_CHUNK
  blocks = min(cus * b3_workgroups_per_cu(K, npl), K_B3_MAX_BLOCKS)
  need = (chunks + K_B3_WAVES - 1) // K_B3_WAVES
  if blocks > need:
    blocks = need if need > 0 else 1
  return blocks


def gram_slices(n, blocks):
  """The slice rule of gram_finish."""
  per_block = n * (n + 1) // 2
  chunks = (per_block + 63) // 64
  slices = min(GRAM_SLICE_WORKGROUPS // chunks, K_GRAM_SLICES_MAX, blocks // GRAM_SLICE_MIN_BLOCKS)
  if slices < 1 or blocks + slices > K_B3_MAX_BLOCKS:
    slices = 1
  return slices


def gram_loops(n, d, npl, aligned, cus, steady=1):
  """(waves that enter the steady-state loop, waves that run iterations of the generic loop, waves) of the Gram kernel."""
  K = (n + 3) // 4
  nsets = b3_nsets(K, npl)
  nw = gram_blocks(n, d, npl, cus) * K_B3_WAVES
  nchunks = (d + K_B3_CHUNK - 1) // K_B3_CHUNK
  full = d // K_B3_CHUNK
  in_steady = in_generic = 0
  for gw in range(nw):
    c = gw
    if aligned and steady and c + (2 * nsets - 1) * nw < full:
      in_steady += 1
      while True:
        c += nsets * nw
        if not c + (2 * nsets - 1) * nw < full:
          break
      c += nsets * nw  # the drain
    if c < nchunks:
      in_generic += 1
  return in_steady, in_generic, nw


def steady_length(K, npl, cus):
  """The smallest d at which EVERY wave of the (K, NPL) instance enters the steady-state loop, plus 64 * 7 + 5
  coordinates: a drain, leftovers for the generic loop in some waves and a ragged last chunk."""
  nw = min(cus * b3_workgroups_per_cu(K, npl), K_B3_MAX_BLOCKS) * K_B3_WAVES
  return K_B3_CHUNK * 2 * b3_nsets(K, npl) * nw + K_B3_CHUNK * 7 + 5


PairGeom = namedtuple("PairGeom", "n ng tiles ut strips slots threads width row_bytes rb nb")


def pair_geometry(n):
  ng = (n + 3) // 4
  tiles = ng * (ng + 1) // 2
  ut = (tiles + 15) // 16
  best, best_bytes, best_num, best_den = -1, 0, -1, 1
  for c, (st, sl) in enumerate(PAIR_CAND):
    lanes = 16 * ut * st
    thr = (lanes + 63) // 64 * 64
    rowb = 16 * sl * st
    tile_bytes = ng * (4 * rowb // K_DMA_BLOCK) * K_DMA_PITCH
    if thr > K_PAIR_MAX_THREADS or 2 * tile_bytes > PAIR_LDS_LIMIT:
      continue
    lhs, rhs = lanes * best_den, best_num * thr
    if best < 0 or lhs > rhs or (lhs == rhs and tile_bytes > best_bytes):
      best, best_num, best_den, best_bytes = c, lanes, thr, tile_bytes
  if best < 0:
    best = 0
  strips, slots = PAIR_CAND[best]
  row_bytes = 16 * slots * strips
  rb = K_DMA_BLOCK // row_bytes
  return PairGeom(n, ng, tiles, ut, strips, slots, (16 * ut * strips + 63) // 64 * 64, 4 * slots * strips, row_bytes,
                  rb, ng * (4 // rb))


def pair_grid(n, d):
  """Workgroups of the whole-stack call of the direct kernel (pair_grid_blocks)."""
  chunks = (d + pair_geometry(n).width - 1) // pair_geometry(n).width
  return max(1, min(PAIR_GRID_MAX, chunks))


def probe_rows(n):
  """The three rows whose coordinate-wise median centres the Gram kernel's rows."""
  K = (n + 3) // 4
  if K >= 3:
    return (0, 4 * (K // 3), 4 * (2 * K // 3))
  if K == 2:
    return (0, 2, 4)
  return (0, 1, 2) if n >= 3 else (0, 0, 0)


# A case: one call.  offset: 0 / 4 / 8 bytes for every row or "mixed"; kind: how the stack is made (see `values`);
# knobs: the BM_* values its process runs with (() = defaults); group: the test that runs it.
Case = namedtuple("Case", "group n d d_total offset kind knobs")


def clique_rows(n, k, where):
  """The k rows rewritten as near-duplicates of one base row."""
  if where == "first":
    return tuple(range(k))
  if where == "last":
    return tuple(range(n - k, n))
  if where == "stride":
    return tuple((i * n) // k for i in range(k))
  if where == "offprobe":  # the rows that are no probe of the centre first
    probes = set(probe_rows(n))
    return tuple(sorted(([r for r in range(n) if r not in probes] + sorted(probes))[:k]))
  raise ValueError(where)


def pair_groups(m):
  """Rows 0 .. m-1 in consecutive pairs, the last three together when m is odd."""
  return [tuple(range(j, j + 2)) if j + 3 != m else (j, j + 1, j + 2) for j in range(0, m - 1, 2)]


def near_groups(case):
  """The groups of rows a stack rewrites as near-duplicates (base + 1e-4 noise) of one base per group, or None."""
  kind = case.kind[0]
  if kind in ("clique", "clique_alias"):
    return [clique_rows(case.n, case.kind[1], case.kind[2])]
  if kind == "pairs":  # ("pairs", m): the first m rows in pairs around as many bases, the rest left alone
    return pair_groups(case.kind[1])
  return None


def expected_listed(case):
  """The rows the accuracy gate lists for a clique / pairs stack, or None where the stack does not decide it.

  The centre is the coordinate-wise median of three probe rows.  With two or three probes inside one group the median
  lies within that group's own spread (1e-4), its rows are as far from the centre as from each other and the Gram form
  is accurate for them: they are not listed.  A group with one probe or none inside has its rows at O(1) from the
  centre in most coordinates and at 1e-4 from each other: a ratio of 1e-8 against a tau of 2e-3 .. 2e-2, all of them
  listed.  Rows outside the groups are at O(1) from everything.

  So a clique reaches k = 2 .. n - 2 only; pairs around unrelated bases, whose probes fall in three different groups,
  list every row they touch: k = n, and k = n - 1 with one row left alone.  (Five rows cannot all be listed: their
  probes are rows 0, 2 and 4, each would need a near partner that is near no other probe, six rows in all.)"""
  groups = near_groups(case)
  if groups is None:
    return None
  probes = set(probe_rows(case.n))
  return tuple(sorted(r for g in groups if len(probes & set(g)) <= 1 for r in g))


def instances(case, cus=256):
  """The instances the call of `case` runs, under the case's knobs, on a device with `cus` compute units:
  ("gram", K, NPL, aligned, "generic" | "steady"), ("gram_reduce", slices),
  ("direct", strips, slots, aligned, "whole" | "gated")."""
  knobs = dict(DEFAULT_KNOBS, **dict(case.knobs))
  aligned = vec_width(row_offsets(case.offset, case.n)) == 4
  if knobs["BM_PAIR_MODE"] == 1:
    g = pair_geometry(case.n)
    return {("direct", g.strips, g.slots, aligned, "whole")}
  K = (case.n + 3) // 4
  npl = planes(case.d if case.d_total is None else case.d_total)
  out = set()
  in_steady, in_generic, _ = gram_loops(case.n, case.d, npl, aligned, cus, knobs["BM_GRAM_STEADY"])
  if in_steady:
    out.add(("gram", K, npl, aligned, "steady"))
  if in_generic or not in_steady:
    out.add(("gram", K, npl, aligned, "generic"))
  out.add(("gram_reduce", gram_slices(case.n, gram_blocks(case.n, case.d, npl, cus))))
  listed = expected_listed(case)
  if listed:
    g = pair_geometry(len(listed))
    out.add(("direct", g.strips, g.slots, aligned, "gated"))
  return out


# ---------------------------------------------------------------------------------------------------------------------
# The case lists (every GPU test of tests/test_gpu_distance_matrix.py runs exactly the cases of its group)

# the tails of a 64-coordinate Gram chunk and of each of the three direct tile widths 64 / 128 / 256
D_TAILS = (1, 3, 63, 64, 65, 127, 129, 255, 257, 515, 4099)
D_OTHER_OFFSETS = 257            # offsets 8 and mixed
D_TWO_PLANES = (65536 + 37, 131072)
D_GATED = 2051
D_GATED_LONG = 70001
D_RANK = 515
GATED_N = (5, 13, 25, 51, 64)
PLACEMENTS = ("first", "last", "stride", "offprobe")
NONFINITE_N = (3, 6, 11, 26, 64)
NONFINITE_D = 64 * 3 + 37
PLAIN = ("plain",)


def direct_long_cases(group, knobs):
  """One row count per tile width of the direct kernel with d = (2 * 1024 + 1) * width + 9: the first workgroup makes
  three whole trips through both tile buffers, the second one ends on a ragged tile."""
  out, seen = [], set()
  for n in range(1, BM_MAX_ROWS + 1):
    w = pair_geometry(n).width
    if w not in seen:
      seen.add(w)
      out.append(Case(group, n, (2 * PAIR_GRID_MAX + 1) * w + 9, None, 0, PLAIN, knobs))
  return out


def slice_cases(cus):
  """(n, d) with 1, 2 and 8 slices of the Gram reduction, picked with the mirror: the first row count of 9 / 40 / 24
  rows upwards and the shortest odd d that gives the slice count."""
  out = []
  for want, n0 in ((1, 9), (2, 40), (8, 24)):
    found = None
    for n in range(n0, BM_MAX_ROWS + 1):
      for blocks in range(1, 513):
        d = K_B3_CHUNK * K_B3_WAVES * blocks - 61
        if gram_slices(n, gram_blocks(n, d, 3, cus)) == want and blocks >= (1, 64, 256)[(1, 2, 8).index(want)]:
          found = (n, d)
          break
      if found:
        break
    assert found, want
    out.append(found)
  return out


def cases(group, cus=256):
  out = []
  if group in ("rows3", "direct_whole"):
    knobs = (("BM_PAIR_MODE", 1),) if group == "direct_whole" else ()
    for n in range(1, BM_MAX_ROWS + 1):
      for off in (0, 4):
        for d in D_TAILS:
          out.append(Case(group, n, d, None, off, PLAIN, knobs))
      for off in (8, "mixed"):
        out.append(Case(group, n, D_OTHER_OFFSETS, None, off, PLAIN, knobs))
    if group == "direct_whole":
      out += direct_long_cases(group, knobs)
  elif group == "planes2":
    for K in B3_CASES:
      for n in (4 * K - 3, 4 * K):
        for d in D_TWO_PLANES:
          for off in (0, 4):
            out.append(Case(group, n, d, PLANE_THRESHOLD, off, PLAIN, ()))
  elif group in ("steady", "knob_steady"):
    knobs = (("BM_GRAM_STEADY", 0),) if group == "knob_steady" else ()
    for K in B3_CASES:
      for npl in (3, 2):
        d = steady_length(K, npl, cus)
        assert d < PLANE_THRESHOLD
        out.append(Case(group, 4 * K, d, PLANE_THRESHOLD if npl == 2 else None, 0, PLAIN, knobs))
  elif group == "gated":
    for n in GATED_N:
      for k in range(2, n + 1):
        for where in PLACEMENTS:
          out.append(Case(group, n, D_GATED, None, 0, ("clique", k, where), ()))
      out.append(Case(group, n, D_GATED_LONG, None, 0, ("clique", 2, "last"), ()))
      out.append(Case(group, n, D_GATED_LONG, None, 0, ("clique", n, "first"), ()))
      out.append(Case(group, n, D_GATED, None, 0, ("clique_alias", max(3, n // 2), "offprobe"), ()))
      for k in range(2, n - 1):
        if n == 13 or k % 8 == 6:
          out.append(Case(group, n, D_GATED, None, 4, ("clique", k, "offprobe"), ()))
      # every row listed (and every row but the last): near-duplicate pairs around as many bases, at both lengths — at
      # the long one a workgroup goes more than once through the tile buffers of a geometry chosen on the device
      for m in (n, n - 1):
        for d in (D_GATED, D_GATED_LONG):
          out.append(Case(group, n, d, None, 0, ("pairs", m), ()))
  elif group == "rank_plain":
    for n in range(1, BM_MAX_ROWS + 1):
      out.append(Case(group, n, D_RANK, None, 0, PLAIN, ()))
  elif group == "rank_gated":
    for n in GATED_N:
      for k in range(2, n + 1):
        out.append(Case(group, n, D_GATED, None, 0, ("clique", k, "offprobe"), ()))
  elif group == "slices":
    for n, d in slice_cases(cus):
      out.append(Case(group, n, d, None, 0, PLAIN, ()))
  elif group == "nonfinite":
    for n in NONFINITE_N:
      for what in ("nan", "+inf", "-inf"):
        for row in sorted(set(probe_rows(n)) | {n - 1}):
          out.append(Case(group, n, NONFINITE_D, None, 0, ("nonfinite", what, row), ()))
  else:
    raise ValueError(group)
  return out


GROUPS = ("rows3", "direct_whole", "planes2", "steady", "knob_steady", "gated", "rank_plain", "rank_gated", "slices",
          "nonfinite")


def all_cases(cus=256):
  return [c for g in GROUPS for c in cases(g, cus)]


def rank_shape(n):
  """(f, m) the ranking tests use at n rows, valid for Krum and Bulyan (n >= 4 f + 3, m = n - f - 2 >= 1), or None."""
  if n < 3:
    return None
  f = (n - 3) // 4
  return f, n - f - 2


# ---------------------------------------------------------------------------------------------------------------------
# Seeded stacks (on the GPU)

def aliases(n):
  """Aliased Byzantine rows of a plain stack: none below three rows, then at least two."""
  return 0 if n < 3 else max(2, n // 5)


def plain_values(n, d, seed):
  """(distinct u x d float32, rowmap): oracle.make_stack's "hetero" distribution on the GPU — mu = 0.1 randn, honest
  rows mu + sigma_i randn with sigma from 0.5 to 1.5 — and aliases(n) Byzantine rows that are ONE row, -0.1 times the
  honest mean."""
  gen = torch.Generator(device=DEV).manual_seed(seed)
  b = aliases(n)
  h = n - b
  mu = 0.1 * torch.randn(d, device=DEV, generator=gen)
  vals = torch.empty(h + (1 if b else 0), d, device=DEV)
  sig = torch.linspace(0.5, 1.5, h).tolist()
  for i in range(h):
    vals[i] = mu + sig[i] * torch.randn(d, device=DEV, generator=gen)
  if b:
    vals[h] = -0.1 * vals[:h].mean(dim=0)
  return vals, list(range(h)) + [h] * b


def clique_values(case):
  """n distinct hetero rows; the rows of the clique rewritten as base + 1e-4 noise (pair_mode_check.py's colluding
  workers), base being the first of them.  "clique_alias": the clique's second row IS its first (one tensor)."""
  n, d = case.n, case.d
  kind = case.kind[0]
  gen = torch.Generator(device=DEV).manual_seed(7000 + 101 * n + (d % 997))
  mu = 0.1 * torch.randn(d, device=DEV, generator=gen)
  sig = torch.linspace(0.5, 1.5, n).tolist()
  vals = torch.empty(n, d, device=DEV)
  for i in range(n):
    vals[i] = mu + sig[i] * torch.randn(d, device=DEV, generator=gen)
  rowmap = list(range(n))
  if kind == "pairs":
    for members in pair_groups(case.kind[1]):
      base = vals[members[0]].clone()
      for r in members:
        vals[r] = base + 1e-4 * torch.randn(d, device=DEV, generator=gen)
    return vals, rowmap
  rows = clique_rows(n, case.kind[1], case.kind[2])
  base = vals[rows[0]].clone()
  for r in rows:
    vals[r] = base + 1e-4 * torch.randn(d, device=DEV, generator=gen)
  if kind == "clique_alias":
    rowmap[rows[1]] = rows[0]
  return vals, rowmap


def nonfinite_coordinates(d):
  """Every lane position 0..63 of a 64-coordinate chunk once (position p in chunk p % 3) and the last coordinate of the
  ragged tail."""
  return [K_B3_CHUNK * (p % 3) + p for p in range(K_B3_CHUNK)] + [d - 1]


def nonfinite_values(case):
  vals, _ = plain_values(case.n, case.d, 9000 + case.n)
  vals = torch.cat([vals, torch.randn(case.n - vals.shape[0], case.d, device=DEV,
                                      generator=torch.Generator(device=DEV).manual_seed(case.n))])  # no aliases
  what, row = case.kind[1], case.kind[2]
  bad = {"nan": math.nan, "+inf": math.inf, "-inf": -math.inf}[what]
  vals[row, torch.tensor(nonfinite_coordinates(case.d), device=DEV)] = bad
  return vals, list(range(case.n))


def values(case):
  kind = case.kind[0]
  if kind == "plain":
    return plain_values(case.n, case.d, 1000 + case.n)
  if kind in ("clique", "clique_alias", "pairs"):
    return clique_values(case)
  if kind == "nonfinite":
    return nonfinite_values(case)
  raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------------------------
# Reference and bars

def sqdist_f64_on_gpu(rows):
  """n x n float64 squared distances, direct differences in fp64 on the GPU (no Gram, no cancellation)."""
  n = len(rows)
  st = torch.stack([r.double() for r in rows])
  out = np.zeros((n, n))
  for i in range(n - 1):
    diff = st[i + 1:] - st[i]
    vals = (diff * diff).sum(dim=1).cpu().numpy()
    out[i, i + 1:] = vals
    out[i + 1:, i] = vals
    del diff
  return out


TOL = 1e-5        # pair_mode_check.py: relative to the distance itself
TOL_PLAIN = 1e-6  # test_seeded_stack_100k's, relative to the distance itself, for plain stacks


def tolerance(case):
  """1e-6 for plain seeded stacks from 63 coordinates on; 1e-5 for cliques, and for plain stacks of 1 or 3 coordinates:
  up to 64 rows of so few random numbers DO hold near-duplicates by chance, pairs just above the accuracy gate, where
  the Gram form of a one-chunk row is good to 2 * 1.2e-7 / 0.1 = 2.4e-6 of the distance (gate_tau, pairwise.hip)."""
  return TOL_PLAIN if case.kind[0] in ("plain", "nonfinite") and case.d >= 63 else TOL


def same_bits64(a, b):
  return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def check_matrix(sq, want, rowmap, tol, bad_row=None):
  """The bars on one matrix `sq` (n x n float64, on the host) against `want` (float64 reference): returns (list of
  what failed, worst relative error).  bad_row: a row with non-finite coordinates — every entry that involves it (off
  the diagonal) must be non-finite, the rest is held to the bars."""
  n = sq.shape[0]
  want = torch.as_tensor(want)
  fails = []
  good = torch.ones(n, dtype=torch.bool)
  if bad_row is not None:
    good[bad_row] = False
    others = torch.arange(n) != bad_row
    if bool(torch.isfinite(sq[bad_row, others]).any()) or bool(torch.isfinite(sq[others, bad_row]).any()):
      fails.append("a finite entry with the non-finite row")
  pair = good[:, None] & good[None, :] & ~torch.eye(n, dtype=torch.bool)
  if not same_bits64(sq, sq.T):
    fails.append("not bitwise symmetric")
  if not bool((sq.diagonal() == 0).all()):
    fails.append("non-zero diagonal")
  if not bool(torch.isfinite(sq[pair]).all()):
    fails.append("non-finite entries")
    return fails, math.inf
  pos = pair & (want > 0)
  rel = ((sq - want).abs()[pos] / want[pos])
  worst = float(rel.max()) if rel.numel() else 0.0
  if worst > tol:
    i, j = [int(x) for x in torch.nonzero(pos)[int(rel.argmax())]]
    fails.append(f"relative error {worst:.3e} > {tol:g} at ({i}, {j}): {sq[i, j].item()!r} for {want[i, j].item()!r}")
  zero = pair & (want == 0)
  if bool((sq[zero] != 0).any()):
    fails.append("non-zero distance where the reference is 0")
  groups = {}
  for r in range(n):
    if good[r]:
      groups.setdefault(rowmap[r], []).append(r)
  for members in (g for g in groups.values() if len(g) > 1):
    third = torch.tensor([r for r in range(n) if r not in members], dtype=torch.long)
    mine = sq[members]
    if bool((mine[:, members] != 0).any()) or not same_bits64(mine[:, third], mine[:1, third].expand(len(members), -1)):
      fails.append(f"aliased rows {members}")
  return fails, worst


# ---------------------------------------------------------------------------------------------------------------------
# Running one case

def _bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


def device_rows(case, vals=None, rowmap=None):
  if vals is None:
    vals, rowmap = values(case)
  return rows_of(place(vals, case.offset), rowmap), rowmap


def run_case(case, vals=None, rowmap=None):
  """(squared distances on the device, rows, rowmap) of one case."""
  bm = _bm()
  rows, rowmap = device_rows(case, vals, rowmap)
  return bm.gars.pairwise_sqdist(rows, d_total=case.d_total), rows, rowmap


def listed_rows(rows):
  """The row list the accuracy gate of the LAST distance call on these rows left in its workspace (pairwise.hip:
  flag[0] = how many, flag[1..] = their indices, ascending)."""
  from byzantinemomentum_amd import _lib, gars
  n, d, device = gars._validate(rows)
  flag = gars._workspace(device, _lib.WS_PAIRWISE, n, d, "ws_pair")[:512].view(torch.int32).cpu()
  return tuple(flag[1:1 + int(flag[0])].tolist())


def rank_with_sqdist(rows, f, m, mode, d_total=None):
  """bm_pairwise_rank with its distance output: (order, scores, squared distances) — gars._rank, which drops the matrix."""
  from byzantinemomentum_amd import _lib, gars
  n, d, device = gars._validate(rows)
  lib = _lib.load()
  sq = torch.empty((n, n), dtype=torch.float64, device=device)
  order = torch.empty(_lib.MAX_ROWS, dtype=torch.int32, device=device)
  scores = torch.empty(_lib.MAX_ROWS, dtype=torch.float64, device=device)
  ws = gars._workspace(device, _lib.WS_PAIRWISE, n, d, "ws_pair")
  with torch.cuda.device(device):
    _lib.check(lib.bm_pairwise_rank(_lib.pointer_table(rows), n, d, d if d_total is None else int(d_total), f, m, mode,
                                    gars._ptr(sq), gars._ptr(order), gars._ptr(scores), gars._ptr(ws),
                                    gars._stream(device)), "bm_pairwise_rank")
  return order, scores, sq


def case_key(case):
  return "/".join(str(x) for x in (case.n, case.d, case.d_total, case.offset) + tuple(case.kind))


def _sha(t):
  return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


class Worst:
  """Worst relative error of a squared distance seen per (form, K, NPL, bar)."""

  def __init__(self):
    self.table = {}

  def add(self, case, rel):
    mode1 = dict(case.knobs).get("BM_PAIR_MODE", 0) == 1
    npl = 0 if mode1 else planes(case.d if case.d_total is None else case.d_total)
    self.merge([["direct" if mode1 else "gram", (case.n + 3) // 4, npl, tolerance(case), rel]])

  def merge(self, entries):
    for form, K, npl, bar, rel in entries:
      key = (form, K, npl, bar)
      self.table[key] = max(self.table.get(key, 0.0), rel)

  def entries(self):
    return [list(k) + [v] for k, v in sorted(self.table.items())]

  def lines(self):
    return [f"{form:6s} K={K:2d} NPL={npl}  worst relative error {rel:.3e}  bar {bar:g}"
            for form, K, npl, bar, rel in self.entries()]


ERRORS = Worst()  # what the sweeps of this process (and the children a test merges in) have seen


def check_case(case, sq, rows, rowmap, worst=ERRORS):
  """Hold one output to its bar; returns the list of failures (strings)."""
  bad_row = case.kind[2] if case.kind[0] == "nonfinite" else None
  want = sqdist_f64_on_gpu(rows)
  fails, rel = check_matrix(sq.cpu(), want, rowmap, tolerance(case), bad_row)
  if worst is not None and math.isfinite(rel):
    worst.add(case, rel)
  return [f"{case_key(case)}: {f}" for f in fails]


def sweep(todo, worst=ERRORS, digests=None):
  """Run the cases of `todo`, generating the values of a plain stack once per row count (at the longest d; shorter
  cases take a prefix of the columns, so that one input runs at every offset).  Returns the failures; fills `digests`
  {case key: SHA-256 of the matrix}."""
  fails = []
  cache = {}
  for case in todo:
    vals = rowmap = None
    if case.kind == PLAIN and case.d <= max(D_TAILS):
      if case.n not in cache:
        cache.clear()
        cache[case.n] = plain_values(case.n, max(D_TAILS), 1000 + case.n)
      full, rowmap = cache[case.n]
      vals = full[:, :case.d].contiguous()
    sq, rows, rowmap = run_case(case, vals, rowmap)
    fails += check_case(case, sq, rows, rowmap, worst)
    if digests is not None:
      digests[case_key(case)] = _sha(sq)
  return fails


def differing_offsets(todo, digests):
  """Cases whose matrix differs in any bit from the one of the same input at offset 0."""
  return [case_key(c) for c in todo if c.offset != 0 and
          digests[case_key(c)] != digests[case_key(c._replace(offset=0))]]


if __name__ == "__main__":
  torch.cuda.init()
  group = sys.argv[1]
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  digests = {}
  failures = sweep(cases(group, cus), ERRORS, digests)
  torch.cuda.synchronize()
  print(json.dumps({"group": group, "knobs": {k: os.environ.get(k) for k in DEFAULT_KNOBS}, "digests": digests,
                    "failures": failures, "worst": ERRORS.entries()}))
