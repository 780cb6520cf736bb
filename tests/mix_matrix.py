"""Which compiled instance of the two mixing kernels a call lands in, seeded inputs and mask sets that reach all 300 of
them, and the expected values the instance tests compare against (a helper module, not a conftest; the shape of
tests/instance_matrix.py, whose `vec_width`, `row_offsets` and `place` it reuses).

  mix_rows_kernel<N, VEC>            (mix_rows.hip)                 N = 1..64, VEC 4 / 2 / 1 up to 28 rows, 2 / 1 beyond
  colwise_mixed_kernel<N, OP, VEC>   (colwise_mixed_dispatch.h)     N = 1..36, median and trimmed mean, VEC 2 / 1

Three parts:
  * a mirror of the launchers: `launches(case)` gives, per launch piece, the width (the widest EVERY input and EVERY
    output pointer allows at the piece's first column, capped per kernel; Tail::kRides never narrows it), the number of
    column groups, whether a tail group exists and whether it shares a wave with body groups; `instances(case)` the
    compiled instances.  tests/test_mix_matrix_cpu.py holds the mirror to the sources and to the code object;
  * seeded inputs: float32 rows of ordinary scale with SPECIAL columns (KINDS) at column 0, in the middle of a wave, at
    the end of the body and in the trailing columns, each kind in every lane position of a 16-byte group; and the mask
    sets (one-hot, complements, neighbour masks, random with an empty mask, buckets, n_out = 64 and n_out = 1);
  * expected values made of the inputs alone: the float32 loop of the contract (nnm_cases.mix_reference) for
    bm_mix_rows; for the fused kernels the lower median / the oracle's trimmed mean of those numpy-mixed values.
"""

import functools
import math
import os
import sys
from collections import namedtuple
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from tests import instance_matrix as M  # noqa: E402
from tests import nnm_cases as nc  # noqa: E402

# ---------------------------------------------------------------------------------------------------------------------
# Mirror of the launchers (mix_rows.hip: launch_mix_n; colwise_mixed_dispatch.h: launch_mixed_n; launch_plan.h)

MIX_ROWS, FUSED = "mix_rows", "colwise_mixed"
MEDIAN, TRMEAN = M.MEDIAN, M.TRMEAN
FUSED_RULES = (MEDIAN, TRMEAN)

BM_MAX_ROWS = 64
K_MIX_WIDE_ROWS = 28           # mix_max_vec<N>: 4 up to here, 2 beyond
K_MIXED_MAX_ROWS = 36          # kMixedMaxRows
K_MIXED_MAX_VEC = 2            # kMixedMaxVec
TAIL_RIDES = True              # Tail::kRides: the trailing d % VEC columns are one more group of the same launch
K_COL_BLOCK = 256
K_COL_MAX_BLOCKS = 256 * 64
K_MAX_COLS_PER_LAUNCH = 1 << 29
WAVE = 64
TRIP = K_COL_MAX_BLOCKS * K_COL_BLOCK   # column groups one trip of the grid-stride loop covers at the capped grid


def mix_max_vec(n):
  return 4 if n <= K_MIX_WIDE_ROWS else 2


def universe():
  """Every compiled instance: 156 + 144."""
  out = {(MIX_ROWS, n, v) for n in range(1, BM_MAX_ROWS + 1) for v in (4, 2, 1) if v <= mix_max_vec(n)}
  out |= {(FUSED, n, rule, v) for n in range(1, K_MIXED_MAX_ROWS + 1) for rule in FUSED_RULES
          for v in (2, 1) if v <= K_MIXED_MAX_VEC}
  return out


# A case: one call of one entry point.  offset / out_offset: bytes behind a 16-byte boundary of every input row / every
# output (the wrappers allocate outputs at 0); piece: BM_WSUM_PIECE (0 = the default 2^29 columns); masks: the name of
# a mask set of mask_sets(kernel, n); f: the rule's f (fused trimmed mean, else 0).
Case = namedtuple("Case", "group kernel rule n d offset out_offset piece masks f")

# One launch: columns [lo, lo + count) at width vec: nvec whole groups, `tail` trailing columns in the group nvec.
Launch = namedtuple("Launch", "lo count vec nvec tail grid groups tail_shares_wave body_trips")


def n_out_of(case):
  return len(mask_sets(case.kernel, case.n)[case.masks]) if case.kernel == MIX_ROWS else 1


def launches(case):
  cap = mix_max_vec(case.n) if case.kernel == MIX_ROWS else K_MIXED_MAX_VEC
  piece = case.piece if case.piece > 0 else K_MAX_COLS_PER_LAUNCH
  n_out = n_out_of(case)
  out = []
  for lo in range(0, case.d, piece):
    count = min(case.d - lo, piece)
    pointers = [(o + 4 * lo) % 16 for o in M.row_offsets(case.offset, case.n) + M.row_offsets(case.out_offset, n_out)]
    vec = min(M.vec_width(pointers), cap)
    nvec = count // vec
    tail = count - nvec * vec
    assert TAIL_RIDES
    grid = min(max(-(-nvec // K_COL_BLOCK), 1), K_COL_MAX_BLOCKS)
    stride = grid * K_COL_BLOCK
    # the tail group is group nvec: it sits in the wave of group nvec - 1 unless it is a wave's first lane
    out.append(Launch(lo, count, vec, nvec, tail, grid, nvec + (1 if tail else 0), tail > 0 and nvec % WAVE != 0,
                      -(-nvec // stride)))
  return out


def instances(case):
  if case.kernel == MIX_ROWS:
    return {(MIX_ROWS, case.n, l.vec) for l in launches(case)}
  return {(FUSED, case.n, case.rule, l.vec) for l in launches(case)}


def input_width(case, lo=0):
  """The width the INPUT pointers alone would allow at column lo (what an output-forced case must stay below)."""
  cap = mix_max_vec(case.n) if case.kernel == MIX_ROWS else K_MIXED_MAX_VEC
  return min(M.vec_width([(o + 4 * lo) % 16 for o in M.row_offsets(case.offset, case.n)]), cap)


# ---------------------------------------------------------------------------------------------------------------------
# Inputs

KINDS = ("nan", "inf", "zeros", "cancel", "tiny", "ties", "huge")
#  nan     a NaN in one row (row c % n of column c): some masks include it, some exclude it
#  inf     +inf in row c % n, -inf in row (c + 1) % n
#  zeros   every row a zero, the odd rows -0
#  cancel  rows c % n and (c + 1) % n hold x and -x, the others +0: a sum that cancels is +0
#  tiny    every row about 2^-124: a subnormal quotient takes the division itself
#  ties    every row k 2^-149, k = 1..12: sums whose quotient is an exact tie between two subnormals whenever the count
#          is even (at counts 6, 10, 12, ... the Markstein quotient of div_small_int rounds such a tie the wrong way)
#  huge    every row in [2.7e38, 3.0e38]: finite on entry, the partial sum of two of them is +inf
NK = len(KINDS)
SITE = 16 * (NK - 1) + 5 * 3 + 1       # columns a site spans: kind k, repeat r at site + 16 k + 5 r (lane positions 0..3)
END = 36                               # the last END columns: column d - 1 - j holds slot j % 9, slots 7 and 8 ordinary


def site_starts(d):
  """Column 0; the middle of the first wave of 16-byte groups; the boundary between two trips of the grid-stride loop."""
  out = [0, 128]
  if d > TRIP + 64:
    out.append(TRIP - 64)
  return out


def special_columns(n, d):
  """{column: index into KINDS}.  The end of the row is laid out backwards from the last column, one kind per column
  with a period of 9 (so that a kind meets all four lane positions), rotated by n — and by 3 more at d > 8 — so that
  the trailing columns of d = 3 and of d = 1027 hold six of the seven kinds between them at every n, and all seven over
  consecutive n."""
  out = {}
  for s in site_starts(d):
    for k in range(NK):
      for r in range(4):
        c = s + 16 * k + 5 * r
        if c < d:
          out[c] = k
  rot = n + (3 if d > 8 else 0)
  for j in range(min(d, END)):
    c = d - 1 - j
    if j % 9 < NK:
      out[c] = (j % 9 + rot) % NK
    else:
      out.pop(c, None)
  return out


@functools.lru_cache(maxsize=8)
def values(n, d):
  """The n x d float32 input of every case of (n, d), whatever its offsets: seeded normal rows, the special columns
  written over them."""
  rng = np.random.default_rng(7919 * n + d % 1000003)
  vals = rng.standard_normal(size=(n, d), dtype=np.float32)
  for c, k in special_columns(n, d).items():
    a, b = c % n, (c + 1) % n
    kind = KINDS[k]
    if kind == "nan":
      vals[a, c] = math.nan
    elif kind == "inf":
      vals[b, c] = -math.inf
      vals[a, c] = math.inf
    elif kind == "zeros":
      vals[:, c] = 0.0
      vals[1::2, c] = -0.0
    elif kind == "cancel":
      x = vals[a, c]
      vals[:, c] = 0.0
      vals[b, c] = -x
      vals[a, c] = x
    elif kind == "tiny":
      vals[:, c] *= np.float32(2.0 ** -124)
    elif kind == "ties":
      vals[:, c] = (rng.integers(1, 13, size=n) * 2.0 ** -149).astype(np.float32)
    else:
      vals[:, c] = rng.uniform(2.7e38, 3.0e38, size=n).astype(np.float32)
  vals.setflags(write=False)
  return vals


def ordinary_mask(n, d):
  m = np.ones(d, dtype=bool)
  m[list(special_columns(n, d))] = False
  return m


def columns_of_kind(n, d, kind):
  k = KINDS.index(kind)
  return sorted(c for c, v in special_columns(n, d).items() if v == k)


# ---------------------------------------------------------------------------------------------------------------------
# Mask sets

def _distances(n):
  rng = np.random.default_rng(4 * n + 1)
  a = rng.uniform(0.5, 2.0, size=(n, n))
  a = (a + a.T) / 2
  np.fill_diagonal(a, 0.0)
  return a


@functools.lru_cache(maxsize=None)
def mask_sets(kernel, n):
  """{name: tuple of 64-bit words}.  bm_mix_rows takes any number of masks; the fused kernels take exactly n."""
  full = (1 << n) - 1
  sets = {"onehot": [1 << r for r in range(n)],
          "complement": [full & ~(1 << r) for r in range(n)]}
  for f in nc.f_values(n):
    sets[f"nnm-f{f}"] = nc.masks_reference(_distances(n), n, f)
  count = min(n, 9) if kernel == MIX_ROWS else n - 1
  rnd = (nc.random_masks(n, count, seed=n) if count else []) + [0]            # the last mask is empty: 0 / 0
  if n < 64:
    rnd[0] |= 1 << n | 1 << 63                                                 # bits at positions >= n are ignored
  sets["random"] = rnd
  if kernel == MIX_ROWS:
    if n >= 2:
      perm = np.random.default_rng(n).permutation(n).tolist()
      sets["buckets"] = [sum(1 << j for j in perm[lo:lo + 2]) for lo in range(0, n, 2)]     # n_out < n
    if n == 3:
      sets["wide"] = [1 + r % 7 for r in range(BM_MAX_ROWS)]                                # n_out = 64 at N = 3
    if n == BM_MAX_ROWS:
      sets["single"] = [full & ~(1 << 31)]                                                  # n_out = 1 at N = 64
  return {k: tuple(v) for k, v in sets.items()}


def masks_f(name):
  """The f of a neighbour mask set, else None."""
  return int(name[5:]) if name.startswith("nnm-f") else None


def runs(kernel, rule, n, long=False):
  """(mask set, rule f) pairs a (kernel, rule, n) is run with.  The fused trimmed mean takes f = 0, 1 and (n - 1) // 2
  on the neighbour masks of EVERY mixing f (the rule's f differs from the masks'), the masks' own f where the rule
  admits it, and (n - 1) // 4 on the other sets."""
  names = list(mask_sets(kernel, n))
  if long:
    names = [s for s in names if s in ("onehot", "complement", "random", "nnm-f1")]
  if kernel == MIX_ROWS or rule == MEDIAN:
    return [(s, 0) for s in names]
  out = []
  for s in names:
    mf = masks_f(s)
    fs = {(n - 1) // 4} if mf is None else {0, 1, (n - 1) // 2, mf}
    out += [(s, f) for f in sorted(fs) if n >= 2 * f + 1]
  return out


# ---------------------------------------------------------------------------------------------------------------------
# The case lists (every GPU test of tests/test_gpu_mix_matrix.py runs exactly the cases of its group)

OFFSETS = (0, 8, 4)
D_EVERY = (3, 1027)            # the tail group alone; one workgroup of 16-byte groups + the tail on a second trip, the
                               # tail in a wave with body groups at 8 bytes
D_FLAGSHIP = (1, 259, 3074)
FLAGSHIP = (3, 11, 25, 28, 29, 36, 64)
D_LONG = TRIP + 259            # 4-byte rows: the body's grid-stride loop takes a second trip
FORCED = ((MIX_ROWS, 11), (MIX_ROWS, 29), (FUSED, 11))
PIECES = ((1002, 3074), (7, 63))
GROUPS = ("every_n", "flagship", "out_forced", "pieces", "long")


def _kernels(n):
  out = [(MIX_ROWS, None)]
  if n <= K_MIXED_MAX_ROWS:
    out += [(FUSED, r) for r in FUSED_RULES]
  return out


def cases(group):
  out = []

  def add(kernel, rule, n, d, offset, out_offset=0, piece=0, long=False):
    for name, f in runs(kernel, rule, n, long):
      out.append(Case(group, kernel, rule, n, d, offset, out_offset, piece, name, f))

  if group == "every_n":
    for n in range(1, BM_MAX_ROWS + 1):
      for kernel, rule in _kernels(n):
        for d in D_EVERY:
          for off in OFFSETS:
            add(kernel, rule, n, d, off)
  elif group == "flagship":
    for n in FLAGSHIP:
      for kernel, rule in _kernels(n):
        for d in D_FLAGSHIP:
          for off in OFFSETS:
            add(kernel, rule, n, d, off)
  elif group == "out_forced":
    for kernel, n in FORCED:
      for rule in ((None,) if kernel == MIX_ROWS else FUSED_RULES):
        for d in D_EVERY:
          for out_off in (4, 8):
            add(kernel, rule, n, d, 0, out_offset=out_off)
  elif group == "pieces":
    for kernel, rule in _kernels(11):
      for piece, d in PIECES:
        add(kernel, rule, 11, d, 0, piece=piece)
  elif group == "long":
    for kernel, rule in _kernels(3):
      add(kernel, rule, 3, D_LONG, 4, long=True)
  else:
    raise ValueError(group)
  return out


def all_cases():
  return [c for g in GROUPS for c in cases(g)]


# ---------------------------------------------------------------------------------------------------------------------
# Expected values, from the inputs alone

@functools.lru_cache(maxsize=64)
def mixed_reference(kernel, n, d, name):
  """The float32 loop of the contract on values(n, d): len(masks) x d."""
  vals = values(n, d)
  out = np.stack(nc.mix_reference([vals[i] for i in range(n)], list(mask_sets(kernel, n)[name])))
  out.setflags(write=False)
  return out


def lower_median(mixed):
  """The lower median of every column (rank (n - 1) // 2), NaN where any value is NaN."""
  n = mixed.shape[0]
  with np.errstate(all="ignore"):
    srt = np.sort(mixed, axis=0)                     # NaN last
  out = srt[(n - 1) // 2].copy()
  out[np.isnan(mixed).any(axis=0)] = np.nan
  return out


def first_difference(got, want):
  """The first column where two float32 arrays differ (a NaN matching any NaN), or None."""
  got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
  gn, wn = np.isnan(got), np.isnan(want)
  bad = (gn != wn) | (~wn & (got.view(np.uint32) != want.view(np.uint32)))
  hit = np.flatnonzero(bad)
  return int(hit[0]) if hit.size else None


# ---------------------------------------------------------------------------------------------------------------------
# Numpy twins of three deliberate defects of mix_one (mix_kernels.h), for tests/test_mix_matrix_cpu.py: the case lists
# must tell each of them from the reference.

def _members(word, n):
  return [j for j in range(n) if (word >> j) & 1]


def broken_keep_dropped(vals, words, vec=1):
  """`keep` dropped in the non-finite path: in a wave that loaded a non-finite value every row is added, whatever the
  mask says.  (Twin at the granularity of a lane: the `vec` columns of a group that holds one.)"""
  n, d = vals.shape
  want = np.stack(nc.mix_reference(list(vals), list(words)))
  odd = ~np.isfinite(vals).all(axis=0)
  group = np.zeros(d, dtype=bool)
  for c in np.flatnonzero(odd):
    group[c // vec * vec: c // vec * vec + vec] = True
  with np.errstate(all="ignore"):
    acc = np.zeros(d, dtype=np.float32)
    for j in range(n):
      acc = acc + vals[j]
    for r, w in enumerate(words):
      want[r, group] = (acc / np.float32(len(_members(w, n))))[group]
  return want


def broken_hi_word(vals, words):
  """`e.hi` read for j < 32 as well: row j < 32 is added iff bit 32 + j is set; the count stays that of the mask."""
  n, d = vals.shape
  out = []
  with np.errstate(all="ignore"):
    for w in words:
      w &= (1 << n) - 1
      acc = np.zeros(d, dtype=np.float32)
      for j in range(n):
        if (w >> (32 + j % 32)) & 1:
          acc = acc + vals[j]
      out.append(acc / np.float32(len(_members(w, n))))
  return np.stack(out)


def _round_f32(v):
  """A Fraction rounded to the nearest float32, ties to even, subnormals included (no overflow handling)."""
  if v == 0:
    return Fraction(0)
  e = max(math.floor(math.log2(abs(v))), -126)
  while abs(v) >= Fraction(2) ** (e + 1):
    e += 1
  while e > -126 and abs(v) < Fraction(2) ** e:
    e -= 1
  q = Fraction(2) ** (e - 23)
  k = v / q
  lo = math.floor(k)
  rem = k - lo
  if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and lo % 2):
    lo += 1
  return lo * q


def div_small_int_exact(x, m):
  """div_small_int(x, m, 1.0f / m) of bm_common.h in exact arithmetic, for a finite float32 x: q = x * rm;
  r = fma(-q, m, x); q1 = fma(r, rm, q)."""
  x, rm = Fraction(float(x)), Fraction(float(np.float32(1.0) / np.float32(m)))
  q = _round_f32(x * rm)
  r = _round_f32(x - q * m)
  return float(_round_f32(q + r * rm))


def broken_division(vals, words, columns):
  """div_small_int taken unconditionally: the mixed values of `columns` (finite sums only)."""
  n = vals.shape[0]
  out = np.zeros((len(words), len(columns)), dtype=np.float32)
  for r, w in enumerate(words):
    members = _members(w, n)
    for i, c in enumerate(columns):
      acc = np.float32(0.0)
      for j in members:
        acc = np.float32(acc + vals[j, c])
      out[r, i] = div_small_int_exact(acc, len(members)) if members else np.nan
  return out


# ---------------------------------------------------------------------------------------------------------------------
# Running one case on the GPU

DEV = "cuda:0"


def _bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


def upload(n, d, offset):
  """values(n, d) on the device, every row `offset` bytes behind a 16-byte boundary (instance_matrix.place)."""
  import torch
  return M.place(torch.tensor(values(n, d), device=DEV), offset)


def device_masks(words):
  import torch
  return torch.tensor(nc.to_int64(list(words)), dtype=torch.int64, device=DEV)


def _offset_rows(count, d, offset):
  """`count` fresh rows of d floats cut from one allocation, each `offset` bytes behind a 256-byte boundary."""
  import torch
  per = -(-(d + 4) // 64) * 64
  pool = torch.empty(count * per, dtype=torch.float32, device=DEV)
  rows = [pool[r * per + offset // 4: r * per + offset // 4 + d] for r in range(count)]
  assert all(v.data_ptr() % 16 == offset for v in rows)
  return rows


def run(case, rows=None):
  """The output of one case as a numpy array: n_out x d (bm_mix_rows) or d (fused).  With every output at a 16-byte
  boundary the call goes through gars.mix_rows / gars.colwise_mixed; an output offset is only reachable through the C
  entry points, whose pointers are the caller's."""
  import ctypes
  import torch
  bm = _bm()
  lib = bm._lib.load()
  if rows is None:
    rows = upload(case.n, case.d, case.offset)
  words = mask_sets(case.kernel, case.n)[case.masks]
  masks = device_masks(words)
  if case.piece:
    assert lib.bm_tuning_set(b"BM_WSUM_PIECE", case.piece) == 0
  try:
    if case.kernel == MIX_ROWS:
      if case.out_offset == 0:
        outs = bm.gars.mix_rows(rows, masks, len(words))
      else:
        outs = _offset_rows(len(words), case.d, case.out_offset)
        rc = lib.bm_mix_rows(bm._lib.pointer_table(rows), case.n, ctypes.c_void_p(masks.data_ptr()), len(words), case.d,
                             bm._lib.pointer_table(outs), None)
        assert rc == 0, (case, rc)
      return torch.stack(list(outs)).cpu().numpy()
    if case.out_offset == 0:
      out = bm.gars.colwise_mixed(case.rule, rows, masks, case.f)
    else:
      out = _offset_rows(1, case.d, case.out_offset)[0]
      op = {MEDIAN: bm._lib.OP_MEDIAN, TRMEAN: bm._lib.OP_TRMEAN}[case.rule]
      rc = lib.bm_colwise_mixed(op, bm._lib.pointer_table(rows), case.n, ctypes.c_void_p(masks.data_ptr()), case.d,
                                case.f, ctypes.c_void_p(out.data_ptr()), None)
      assert rc == 0, (case, rc)
    return out.cpu().numpy()
  finally:
    if case.piece:
      assert lib.bm_tuning_set(b"BM_WSUM_PIECE", 0) == 0
