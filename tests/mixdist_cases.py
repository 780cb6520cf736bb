"""The contract of bm_mixed_sqdist / bm_mix_weights (include/bm_gar.h) restated as loops over Python floats — IEEE
doubles, one rounding per operation, in the stated order — plus the bars and the crafted inputs the CPU and the GPU tests
share.  TEST INFRASTRUCTURE: nothing here is used by the product."""

import ctypes
import functools
import math

import numpy as np

from tests import nnm_cases as nc

MAX_ROWS = 64
EPS64 = 2.0 ** -53
SUM_BAR = 2.0 ** -40     # three sequential sums of at most 4 096 non-negative fp64 terms: 3 * 4096 * 2^-53 < 2^-40
PASS_BAR = 1e-5          # the distance pass's own committed relative bar (tests/test_gpu_distance_matrix.py)


# ---------------------------------------------------------------------------- #
# The contract, restated

def members(word, n_in):
  return [j for j in range(n_in) if (word >> j) & 1]


def _sums(D, n_in, words):
  """(Q, P): Q[i][b] and the function P(a, b), in the definition's order."""
  n_out = len(words)
  sets = [members(w, n_in) for w in words]
  Q = [[0.0] * n_out for _ in range(n_in)]
  for i in range(n_in):
    for b in range(n_out):
      s = 0.0
      for j in sets[b]:
        if j != i:
          s = s + D[min(i, j)][max(i, j)]
      Q[i][b] = s

  def P(a, b):
    s = 0.0
    for i in sets[a]:
      s = s + Q[i][b]
    return s

  return Q, P


def mixed_reference(sq, n_in, words):
  """out[a][b] of bm_mixed_sqdist as a list of lists of Python floats, and per pair the three terms
  (P_ab / (c_a c_b), P_aa / (2 c_a^2), P_bb / (2 c_b^2)) whose sum scales the rounding bar (None where the pair takes no
  arithmetic: the diagonal, equal or empty masks, a non-finite sum)."""
  D = [[float(v) for v in row] for row in np.asarray(sq, dtype=np.float64).reshape(n_in, n_in)]
  n_out = len(words)
  _, P = _sums(D, n_in, words)
  diag = [P(a, a) for a in range(n_out)]
  count = [float(bin(w).count("1")) for w in words]
  out = [[0.0] * n_out for _ in range(n_out)]
  terms = [[None] * n_out for _ in range(n_out)]
  for a in range(n_out):
    out[a][a] = 0.0 if words[a] else math.nan
    for b in range(a + 1, n_out):
      if not words[a] or not words[b]:
        v = math.nan
      elif words[a] == words[b]:
        v = 0.0
      else:
        x, y = (a, b) if words[a] < words[b] else (b, a)       # the smaller mask word walks the outer sum
        p = P(x, y)
        if not (math.isfinite(p) and math.isfinite(diag[a]) and math.isfinite(diag[b])):
          v = math.nan
        else:
          t1 = p / (count[x] * count[y])
          t2 = 0.5 * diag[x] / (count[x] * count[x])
          t3 = 0.5 * diag[y] / (count[y] * count[y])
          v = t1 - t2 - t3
          v = 0.0 if v <= 0.0 else v
          terms[a][b] = terms[b][a] = (t1, t2, t3)
      out[a][b] = out[b][a] = v
  return out, terms


def weights_reference(words, n_in, w=None, sel=None, m=None):
  """w_out of bm_mix_weights: 64 Python floats."""
  n_out = len(words)
  ok = True
  if sel is not None:
    sel = [int(t) for t in sel[:m]]
    ok = all(0 <= t < n_out for t in sel)
    w = [0.0] * n_out
    if ok:
      for t in sel:
        w[t] = w[t] + 1.0 / float(m)
  ok = ok and all(w[r] == 0.0 or words[r] for r in range(n_out))
  out = [0.0] * MAX_ROWS
  for j in range(n_in):
    s = 0.0
    for r in range(n_out):
      if w[r] != 0.0 and (words[r] >> j) & 1:
        s = s + w[r] / float(bin(words[r]).count("1"))
    out[j] = s if ok else math.nan
  return out


def same_bits64(got, want):
  """Bit for bit in float64, a NaN matching any NaN (its sign and payload are the implementation's)."""
  got = np.ascontiguousarray(np.asarray(got, dtype=np.float64))
  want = np.ascontiguousarray(np.asarray(want, dtype=np.float64))
  if got.shape != want.shape:
    return False
  nan = np.isnan(want)
  if not np.array_equal(np.isnan(got), nan):
    return False
  return np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan])


# ---------------------------------------------------------------------------- #
# The library's host forms on numpy arrays

def _p(a):
  return a.ctypes.data_as(ctypes.c_void_p)


def host_mixed(lib, sq, n_in, words, n_out=None):
  """(code, out float64 (n_out, n_out)) of bm_mixed_sqdist; buffers of exactly the documented sizes."""
  n_out = len(words) if n_out is None else n_out
  sq = np.ascontiguousarray(sq, dtype=np.float64)
  masks = np.array(words, dtype=np.uint64)
  out = np.full((max(n_out, 0), max(n_out, 0)), -7.0)
  return lib.bm_mixed_sqdist(_p(sq), n_in, _p(masks), n_out, _p(out)), out


def host_weights(lib, words, n_in, w=None, sel=None, m=0, n_out=None):
  """(code, w_out float64[64]) of bm_mix_weights."""
  n_out = len(words) if n_out is None else n_out
  masks = np.array(words, dtype=np.uint64)
  out = np.full(MAX_ROWS, -7.0)
  wv = None if w is None else np.array(w, dtype=np.float64)
  sv = None if sel is None else np.array(sel, dtype=np.int32)
  code = lib.bm_mix_weights(_p(masks), n_in, n_out, None if wv is None else _p(wv), None if sv is None else _p(sv), m,
                            _p(out))
  return code, out


# ---------------------------------------------------------------------------- #
# Mask sets

def bucket_words(n, s, seed):
  perm = np.random.default_rng(seed).permutation(n).tolist()
  return [sum(1 << int(j) for j in perm[lo:lo + s]) for lo in range(0, n, s)]


def visible(words, n_in):
  return [w & ((1 << n_in) - 1) for w in words]


ROW_COUNTS = (1, 2, 7, 11, 25, 51, 64)


@functools.lru_cache(maxsize=None)
def mask_sets(n):
  """((name, words), ...) for n_in = n original rows: the neighbour masks of a float64 matrix, random masks with
  n_out != n_in, buckets with an uneven last one."""
  sq = nc.sqdist64(nc.random_rows(n, 16, seed=n))
  sets = [(f"nnm-f{f}", tuple(nc.masks_reference(sq, n, f))) for f in nc.f_values(n)]
  sets.append(("random-fewer", tuple(visible(nc.random_masks(n, max(1, n // 2), seed=3 * n), n))))
  sets.append(("random-more", tuple(visible(nc.random_masks(n, min(MAX_ROWS, n + 5), seed=5 * n), n))))
  if n >= 3:
    sets.append(("buckets-2", tuple(bucket_words(n, 2, n))))
    sets.append(("buckets-3", tuple(bucket_words(n, 3, n + 1))))
  return tuple(sets)


# ---------------------------------------------------------------------------- #
# Bars

def weights_of(word, n_in):
  c = bin(word).count("1")
  return np.array([(1.0 / c if (word >> j) & 1 else 0.0) for j in range(n_in)])


def pass_bar(sq64, n_in, wa, wb):
  """1/2 sum_ij |w_i| |w_j| D_ij with w = W_a - W_b: what a relative error of 1 in every entry of D can move
  -1/2 w' D w by (the rows common to both masks cancel in w, whatever the order of evaluation)."""
  w = np.abs(weights_of(wa, n_in) - weights_of(wb, n_in))
  return 0.5 * float(w @ np.asarray(sq64)[:n_in, :n_in] @ w)


def mixed_rows64(rows, words):
  ys, _ = nc.mix_reference64(rows, words)
  return ys


# ---------------------------------------------------------------------------- #
# Krum in float64 on a matrix of squared distances

def krum_scores64(sq, n, f):
  dist = np.sqrt(np.asarray(sq, dtype=np.float64))
  dist = np.where(np.isfinite(dist), dist, np.inf)
  scores = []
  for i in range(n):
    others = sorted(dist[i, j] for j in range(n) if j != i)
    s = 0.0
    for v in others[:n - f - 1]:
      s = s + v
    scores.append(s)
  order = sorted(range(n), key=lambda i: (scores[i], i))
  return scores, order


# ---------------------------------------------------------------------------- #
# Crafted inputs on which both forms must select the same rows (conditions on the INPUTS, from float64 alone)

def line_rows(n, d, seed):
  """Rows p_i u + 0.05 noise_i: u one Gaussian direction, p_i uniform in [0, sqrt(n)] — neighbourhoods are intervals of
  the line, so few distinct masks, and the mixed rows are spread along it."""
  rng = np.random.default_rng(seed)
  u = rng.normal(size=d)
  p = rng.uniform(0.0, math.sqrt(n), size=n)
  return [(p[i] * u + 0.05 * rng.normal(size=d)).astype(np.float32) for i in range(n)]


def selection_margin(rows, n, f, m):
  """(neighbour gap, score margin, words, order) in float64: the margin is the smallest relative gap between the scores
  of two rows adjacent in the Krum order of the mixed rows up to position m (the last selected against the first
  rejected included), pairs with equal masks — exact ties in both forms, resolved by index — left out."""
  sq = nc.sqdist64(rows)
  gap = nc.neighbour_gap(sq, n, f)
  words = nc.masks_reference(sq, n, f)
  mixed = mixed_rows64(rows, words)
  scores, order = krum_scores64(nc.sqdist64(mixed), n, f)
  margin = math.inf
  for t in range(min(m, n - 1)):
    a, b = order[t], order[t + 1]
    if words[a] != words[b]:
      margin = min(margin, (scores[b] - scores[a]) / scores[b])
  return gap, margin, words, order


@functools.lru_cache(maxsize=None)
def crafted_case(n, f, d, min_gap=1e-2):
  """The first seed (from 1) whose line rows meet both conditions at >= min_gap: (rows, words, order, seed, gap, margin)."""
  m = n - f - 2
  for seed in range(1, 200):
    rows = line_rows(n, d, seed)
    gap, margin, words, order = selection_margin(rows, n, f, m)
    if gap >= min_gap and margin >= min_gap:
      return rows, words, order, seed, gap, margin
  raise AssertionError("no seed below 200 meets the conditions")
