"""Numpy restatements of the nearest-neighbour mixing contract (include/bm_gar.h: bm_nnm_masks, bm_mix_rows) and the
crafted inputs the CPU and the GPU tests of it share.  TEST INFRASTRUCTURE: nothing here is used by the product."""

import math

import numpy as np

MAX_ROWS = 64
U = 2.0 ** -24   # the unit roundoff of float32


# ---------------------------------------------------------------------------- #
# The contract, restated

def masks_reference(sq, n, f):
  """N_i = {i} + the n - f - 1 OTHER rows of smallest sq[i][j]: ties to the lower index, NaN last in index order (+inf
  before NaN).  Returns n Python integers (bit j of word i: j in N_i)."""
  sq = np.asarray(sq, dtype=np.float64).reshape(n, n)
  words = []
  for i in range(n):
    others = [j for j in range(n) if j != i]
    # a total order written out: (is NaN, key, index) — Python's sort is stable, the index makes it explicit
    others.sort(key=lambda j: (1, 0.0, j) if math.isnan(sq[i, j]) else (0, sq[i, j], j))
    word = 1 << i
    for j in others[:n - f - 1]:
      word |= 1 << j
    words.append(word)
  return words


def mix_reference(rows, masks):
  """The float32 loop of the contract: per output row acc = +0, acc = acc + x_j over the rows in the mask ascending, then
  one division by their count.  rows: list of float32 arrays; masks: Python integers.  Rows outside a mask are not
  touched; bits at positions >= n are ignored; an empty mask gives NaN."""
  n, d = len(rows), rows[0].shape[0]
  outs = []
  with np.errstate(all="ignore"):
    for word in masks:
      members = [j for j in range(n) if (word >> j) & 1]
      acc = np.zeros(d, dtype=np.float32)
      for j in members:
        acc = acc + rows[j]
      outs.append(acc / np.float32(len(members)))
  return outs


def mix_reference64(rows, masks):
  """(y64, bound): the same averages in float64 and the bar a float32 sequential sum of m terms and one division must
  keep, |y - y64| <= (m + 1) 2^-24 sum_{j in mask} |x_j| / m — m - 1 additions and one division, each within one unit
  roundoff of a partial sum that never exceeds sum |x_j| (to first order; the spare unit covers the second-order terms)."""
  n, d = len(rows), rows[0].shape[0]
  ys, bounds = [], []
  for word in masks:
    members = [j for j in range(n) if (word >> j) & 1]
    m = len(members)
    stack = np.stack([rows[j].astype(np.float64) for j in members]) if m else np.zeros((0, d))
    ys.append(stack.sum(axis=0) / m if m else np.full(d, np.nan))
    bounds.append((m + 1) * U * np.abs(stack).sum(axis=0) / m if m else np.zeros(d))
  return ys, bounds


def same_bits(got, want):
  """Bit for bit, a NaN matching any NaN (IEEE 754 leaves the sign and payload of a generated NaN to the implementation:
  x86 and the GPU differ there, and no rule of the project reads them)."""
  got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
  if got.shape != want.shape:
    return False
  nan = np.isnan(want)
  if not np.array_equal(np.isnan(got), nan):
    return False
  return np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def to_int64(words):
  """64-bit patterns as the signed words an int64 tensor holds."""
  return [w - (1 << 64) if w >= (1 << 63) else w for w in words]


def from_int64(values):
  return [int(v) & ((1 << 64) - 1) for v in values]


# ---------------------------------------------------------------------------- #
# Crafted distance matrices (test 1 of the feature; the GPU test compares the device form on the same)

def _sym(rng, n, scale=1.0):
  a = rng.uniform(0.5, 2.0, size=(n, n)) * scale
  a = (a + a.T) / 2
  np.fill_diagonal(a, 0.0)
  return a


def mask_cases():
  """(name, sq float64[n, n], n, f)"""
  rng = np.random.default_rng(2023)
  cases = []
  # exact ties: the all-zero block of f aliased rows, and a matrix of one value
  n, f = 11, 3
  sq = _sym(rng, n)
  sq[n - f:, n - f:] = 0.0
  sq[:, n - f:] = sq[:, [n - f]]
  sq[n - f:, :] = sq[[n - f], :]
  sq[n - f:, n - f:] = 0.0
  cases.append(("aliased-block", sq.copy(), n, f))
  cases.append(("all-equal", np.full((7, 7), 3.5), 7, 2))
  # signed zeros are one key
  z = _sym(rng, 5)
  z[0, 1], z[0, 2], z[0, 3] = 0.0, -0.0, 0.0
  cases.append(("signed-zeros", z, 5, 2))
  # a NaN row and column
  sq = _sym(rng, 11)
  sq[4, :] = np.nan
  sq[:, 4] = np.nan
  cases.append(("nan-row", sq, 11, 2))
  # several NaN keys in one row: index order among themselves
  sq = _sym(rng, 9)
  sq[0, [2, 5, 7]] = np.nan
  cases.append(("nan-keys", sq, 9, 1))
  # a +inf entry: before NaN, after every finite key
  sq = _sym(rng, 9)
  sq[1, 3] = np.inf
  sq[1, 2] = np.nan
  sq[1, 8] = np.inf
  cases.append(("inf-and-nan", sq, 9, 2))
  # D[i][i] != 0: row i is still taken
  sq = _sym(rng, 11)
  np.fill_diagonal(sq, 100.0)
  sq[3, 3] = np.nan
  sq[5, 5] = np.inf
  cases.append(("diagonal", sq, 11, 4))
  # f = 0 (full masks), f = n - 1 (self only), n = 1, n = 64
  cases.append(("f0", _sym(rng, 11), 11, 0))
  cases.append(("self-only", _sym(rng, 11), 11, 10))
  cases.append(("n1", np.zeros((1, 1)), 1, 0))
  cases.append(("n64", _sym(rng, 64), 64, 13))
  cases.append(("n64-f0", _sym(rng, 64), 64, 0))
  cases.append(("n64-self", _sym(rng, 64), 64, 63))
  cases.append(("n25", _sym(rng, 25, 1e6), 25, 5))
  return cases


REFUSED = [(0, 0), (65, 0), (11, -1), (11, 11), (1, 1), (-3, 0)]   # (n, f) outside 1 <= n <= 64, 0 <= f < n


# ---------------------------------------------------------------------------- #
# Rows for the mixing tests

def random_rows(n, d, seed):
  rng = np.random.default_rng(seed)
  return [rng.normal(size=d).astype(np.float32) for _ in range(n)]


def random_masks(n, n_out, seed):
  rng = np.random.default_rng(seed)
  return [int(rng.integers(1, 1 << min(n, 62))) | (int(rng.integers(0, 4)) << 62 if n == 64 else 0) for _ in range(n_out)]


def f_values(n):
  return sorted({f for f in (0, 1, (n - 1) // 2, n - 1) if 0 <= f < n})


def sqdist64(rows):
  x = np.stack([r.astype(np.float64) for r in rows])
  diff = x[:, None, :] - x[None, :, :]
  return (diff * diff).sum(axis=2)


def ladder_rows(n, d, ratio, seed):
  """Rows 0.3 g + s_i g_i, s_i a shuffled geometric ladder: every row's neighbours are well separated in distance."""
  rng = np.random.default_rng(seed)
  g = rng.normal(size=d)
  s = ratio ** np.arange(n)
  rng.shuffle(s)
  return [(0.3 * g + s[i] * rng.normal(size=d)).astype(np.float32) for i in range(n)]


def neighbour_gap(sq, n, f):
  """The smallest relative gap, over the rows, between the last included and the first excluded distance (inf when no
  row is excluded)."""
  gap = math.inf
  for i in range(n):
    keys = sorted(sq[i, j] for j in range(n) if j != i)
    k = n - f - 1
    if 0 < k < len(keys):
      gap = min(gap, (keys[k] - keys[k - 1]) / keys[k])
  return gap


def separated_case(n, f, d, ratio, min_gap=1e-2):
  """The first seed (from 1) whose ladder rows have a neighbour gap >= min_gap in float64: (rows, sq64, seed, gap).  A
  condition on the INPUTS: with it the float32 distance pass (relative error about 2e-6 at these lengths) must find the
  float64 neighbour sets exactly."""
  for seed in range(1, 200):
    rows = ladder_rows(n, d, ratio, seed)
    sq = sqdist64(rows)
    gap = neighbour_gap(sq, n, f)
    if gap >= min_gap:
      return rows, sq, seed, gap
  raise AssertionError("no seed below 200 separates the neighbours")
