"""Cases and the float64 reference shared by the tests of the spectral filtering rules CAF and DnC
(test_spectral_cpu.py, test_spectral_rules_cpu.py, test_gpu_spectral.py).

The rules are defined on the vectors; the library evaluates them on the squared distances of the rows
(csrc/spectral_core.h).  `vector_spectral` is the definition, in float64 numpy, on rows, differences and sums only.
The cases are those of tests/center_cases.py (n = 11, 25, 51; d = 4099, 1027).
"""

import collections
import ctypes
import math

import numpy as np

from tests import center_cases as cc

MODES = {"caf": 0, "dnc": 1}
POWER_ITERS = (1, 16, 32)
T_END_TO_END = 16

# A committed case must be decided by more than this (Reference.margins): below it the fp32 pipeline could take another
# branch than the float64 reference and the comparison of the outputs would say nothing about the kernels.
MIN_MARGIN = 1e-5

# Bar of the GPU tests (b) and (g): |out - ref| / |ref| of the fp32 output vector against `vector_spectral`, 4 x the
# worst error measured on an MI355X over the committed cases at T = 16 (profiles/spectral_errors.txt; the kernels are
# deterministic: the margin is for other seeds).  Measured worst: caf 1.018e-07 (n51-k12-far), dnc 9.743e-08
# (n51-k12-empire) — the rounding of the fp32 output and of the fp32 weights, as for geomed (1.020e-07).
BAR_B = {"caf": 4 * 1.018e-07, "dnc": 4 * 9.743e-08}

cases, case_id, make_rows, exact_sqdist = cc.cases, cc.case_id, cc.make_rows, cc.exact_sqdist
combine, relative_error = cc.combine, cc.relative_error

Reference = collections.namedtuple("Reference", "weights out rounds kept lam usable margins")


def count_of(case, mode):
  """The `count` of the issue's cases: CAF f = the Byzantine rows, DnC k = ceil(1.0 * f) = the same."""
  return case.k


def usable_rows(x):
  """The predicate of csrc/center_core.h on the vectors: a row is unusable when its distance to at least one and to at
  least half of the other rows is non-finite."""
  n = x.shape[0]
  ok = np.ones(n, dtype=bool)
  for i in range(n):
    with np.errstate(invalid="ignore", over="ignore"):
      diff = x - x[i]
      sq = np.einsum("ij,ij->i", diff, diff)
    bad = int(sum(1 for j in range(n) if j != i and not math.isfinite(sq[j])))
    ok[i] = not (bad > 0 and 2 * bad >= n - 1)
  return ok


def evaluate(x, c, T):
  """One evaluation E(c) on the vectors: None when degenerate, else (g, lam) with g_i = <y_i, v>."""
  live = c > 0
  C = c.sum()
  mu = (c[live, None] * x[live]).sum(axis=0) / C
  y = np.zeros_like(x)
  y[live] = x[live] - mu
  key = np.where(live, c * np.einsum("ij,ij->i", y, y), 0.0)
  j = int(np.argmax(key))  # the first of the largest
  if not key[j] > 0:
    return None
  v = y[j].copy()
  for _ in range(T):
    w = ((c[live] * (y[live] @ v))[:, None] * y[live]).sum(axis=0) / C
    norm = math.sqrt(float(w @ w))
    if norm == 0:
      break
    v = w / norm
  v = v / math.sqrt(float(v @ v))
  g = np.where(live, y @ v, 0.0)
  # bit-identical rows have ONE projection (a blocked matrix product may round them apart): that of the first of them
  first = {}
  for i in range(x.shape[0]):
    g[i] = g[first.setdefault(x[i].tobytes(), i)]
  return g, float((c * g * g).sum() / C)


def vector_spectral(rows, mode, count, T):
  """CAF (count = f) or DnC (count = k) ON THE VECTORS in float64: a Reference.  Rows of weight 0 take no part in an
  evaluation: the largest tau is taken over the rows that still have weight.  `margins`: how far each decision was from
  going the other way — "lambda": the gap between the two smallest lambda, relative; "mass": the distance of sum c from
  n - 2f at each check, over n; "dnc": the gap between the tau of the last row removed and of the first row kept where
  the two rows differ, over the largest tau (inf where there was no such decision)."""
  x = np.asarray(rows, dtype=np.float64)
  n = x.shape[0]
  ok = usable_rows(x)
  U = int(ok.sum())
  margins = {"lambda": math.inf, "mass": math.inf, "dnc": math.inf}
  if U == 0:
    return Reference(np.full(n, math.nan), np.full(x.shape[1], math.nan), 0, -1, math.inf, 0, margins)
  c = ok.astype(np.float64)
  best, lam_best, kept, rounds = c / c.sum(), math.inf, -1, 0
  if mode == "caf":
    lams = []
    for rnd in range(n):
      C = c.sum()
      margins["mass"] = min(margins["mass"], abs(C - (n - 2 * count)) / n)
      if not C > n - 2 * count:
        break
      ev = evaluate(x, c, T)
      if ev is None:
        break
      g, lam = ev
      rounds += 1
      lams.append(lam)
      if lam < lam_best:
        lam_best, best, kept = lam, c / C, rnd
      tau = g * g
      tmax = tau[c > 0].max()
      if not tmax > 0:
        break
      ratio = np.where(tau == tmax, 1.0, tau / tmax)
      c = np.where(c > 0, c * (1.0 - ratio), 0.0)
    if len(lams) > 1:
      low = sorted(lams)
      margins["lambda"] = (low[1] - low[0]) / low[1]
  else:
    ev = evaluate(x, c, T)
    tau = np.zeros(n)
    if ev is not None:
      tau, lam_best, kept, rounds = ev[0] ** 2, ev[1], 0, 1
    drop = max(0, count - (n - U))
    order = sorted((i for i in range(n) if ok[i]), key=lambda i: (-tau[i], -i))  # largest tau first, then higher index
    gone = order[:drop]
    if 0 < drop < U:
      last, first = gone[-1], order[drop]
      if not np.array_equal(x[last], x[first]) and tau.max() > 0:
        margins["dnc"] = (tau[last] - tau[first]) / tau.max()
    best = ok.astype(np.float64)
    best[gone] = 0.0
    best /= U - drop
  live = best > 0
  out = (best[live, None] * x[live]).sum(axis=0)
  return Reference(best, out, rounds, kept, lam_best, U, margins)


def host_weights(lib, sq, n, mode, count, T):
  """bm_spectral_weights on a float64 numpy matrix: (code, weights (64,), info (4,))."""
  sq = np.ascontiguousarray(sq, dtype=np.float64)
  weights = np.full(64, -7.0)
  info = np.full(4, -7.0)
  code = lib.bm_spectral_weights(sq.ctypes.data_as(ctypes.c_void_p), int(n), MODES[mode], int(count), int(T),
                                 weights.ctypes.data_as(ctypes.c_void_p), info.ctypes.data_as(ctypes.c_void_p))
  return code, weights, info


def with_nan_rows(sq, which):
  sq = np.array(sq, dtype=np.float64)
  sq[which, :] = math.nan
  sq[:, which] = math.nan
  return sq


def sixty_four_rows():
  """64 rows, the last nine being copies of one far row."""
  big = np.random.default_rng(64).normal(size=(64, 37)).astype(np.float32)
  big[-9:] = big[-1] + 20.0
  return big


def crafted():
  """[(name, sq, n, mode, count)]: the crafted matrices of the CPU tests, which the GPU test (a) runs bit for bit."""
  rng = np.random.default_rng(7)
  out = []
  out.append(("one-row", np.zeros((1, 1)), 1, "caf", 0))
  out.append(("one-row-dnc", np.zeros((1, 1)), 1, "dnc", 0))
  out.append(("two-rows", np.array([[0.0, 9.0], [9.0, 0.0]]), 2, "caf", 0))
  out.append(("two-rows-dnc", np.array([[0.0, 9.0], [9.0, 0.0]]), 2, "dnc", 1))
  three = exact_sqdist(rng.normal(size=(3, 5)).astype(np.float32))
  out.append(("three-rows", three, 3, "caf", 1))
  out.append(("three-rows-dnc", three, 3, "dnc", 2))
  big = sixty_four_rows()
  out.append(("sixty-four", exact_sqdist(big), 64, "caf", 9))
  out.append(("sixty-four-f31", exact_sqdist(big), 64, "caf", 31))
  out.append(("sixty-four-dnc", exact_sqdist(big), 64, "dnc", 9))
  eleven = rng.normal(size=(11, 9)).astype(np.float32)
  out.append(("f-zero", exact_sqdist(eleven), 11, "caf", 0))
  out.append(("k-zero", exact_sqdist(eleven), 11, "dnc", 0))
  out.append(("all-equal", np.zeros((7, 7)), 7, "caf", 2))
  out.append(("all-equal-dnc", np.zeros((7, 7)), 7, "dnc", 2))
  far = eleven.copy()
  far[8:] = far[8] + 50.0
  out.append(("far-copies", exact_sqdist(far), 11, "caf", 3))
  out.append(("far-copies-dnc", exact_sqdist(far), 11, "dnc", 3))
  out.append(("nan-rows", with_nan_rows(exact_sqdist(far), [2, 5]), 11, "caf", 3))
  out.append(("nan-rows-mean", with_nan_rows(exact_sqdist(eleven), [8, 9, 10]), 11, "caf", 1))  # U = 8 <= 11 - 2
  out.append(("nan-rows-at-floor", with_nan_rows(exact_sqdist(eleven), [9, 10]), 11, "caf", 1))    # U = 9 = 11 - 2
  out.append(("nan-rows-dnc", with_nan_rows(exact_sqdist(far), [2, 5]), 11, "dnc", 3))
  out.append(("no-usable-row", np.full((5, 5), math.nan), 5, "caf", 1))
  out.append(("no-usable-row-dnc", np.full((5, 5), math.nan), 5, "dnc", 1))
  return out
