"""Cases and float64 references shared by the tests of the geometric median and centered clipping
(test_center_weights_cpu.py, test_center_rules_cpu.py, test_gpu_center_*.py).

The rules are defined on the vectors; the library iterates on the weights of an affine combination of the rows
(csrc/center_core.h).  `vector_iteration` is the definition, in float64 numpy, on the vectors themselves.
"""

import collections
import ctypes
import math

import numpy as np

Case = collections.namedtuple("Case", "n k d attack seed")

SHAPES = ((11, 2, 4099), (25, 5, 4099), (25, 11, 4099), (51, 12, 1027))
ATTACKS = ("empire", "little", "far", "duplicate")
GEOMED_ITERS, CCLIP_ITERS = 32, 3


# Bars of the GPU tests, each 4 x the worst error measured on an MI355X over the committed seeds (the margin is for other
# seeds: the kernels are deterministic); every measured figure is in profiles/center_errors.txt.
#   BAR_B       |out - ref| / |ref| of the fp32 output of a rule against the float64 iteration on the vectors
#               (tests/test_gpu_center_rules.py (b)); also the bar of the step's defense vector and update against the
#               oracle-backed step (tests/test_gpu_center_step.py).  Measured worst: geomed 1.020e-07, cclip 1.062e-07.
#   FLOATS_BAR  the study row of the step (`floats()`) against the oracle-backed step's, every quantity normalised as
#               oracle.step_oracle.assert_floats_close normalises it (float_errors below).  Measured worst over every
#               quantity, step and case: 1.943e-07 (curv_sampled; defense_norm_max 1.932e-07, defense_norm_avg
#               1.216e-07, every quantity that does not involve the rule below 1.1e-08).
BAR_B = {"geomed": 4 * 1.020e-07, "cclip": 4 * 1.062e-07}
FLOATS_BAR = 4 * 1.943e-07


def float_errors(got, want):
  """{quantity: error} of a study row against the expected one, each error normalised as
  oracle.step_oracle.assert_floats_close normalises it (relative to the value with a floor of 1e-3 for the norms,
  absolute for the cosines, ...).  A NaN that is expected and found counts 0, a NaN on one side alone counts inf."""
  from oracle.step_oracle import COS_KEYS, FLOAT_KEYS

  def err(key, scale):
    g, w = got[key], want[key]
    if math.isnan(w) or math.isnan(g):
      return 0.0 if math.isnan(w) and math.isnan(g) else math.inf
    if scale(w) == 0:  # (an l2 from the origin that is exactly zero must be found exactly)
      return 0.0 if g == w else math.inf
    return abs(g - w) / scale(w)

  out = {key: err(key, lambda w: max(abs(w), 1e-3)) for key in FLOAT_KEYS}
  avg = want["attack_norm_avg"]
  out["attack_norm_dev"] = err("attack_norm_dev", lambda w: avg if not math.isnan(avg) else 1.0)
  out.update({key: err(key, lambda w: 1.0) for key in COS_KEYS})
  out["curv_sampled"] = err("curv_sampled", lambda w: max(abs(w), 1.0))
  if "l2_origin" in want and not math.isnan(want["l2_origin"]):
    out["l2_origin"] = err("l2_origin", lambda w: w)
  return out


def cases():
  return [Case(n, k, d, attack, 1000 * n + 10 * k + a) for (n, k, d) in SHAPES for a, attack in enumerate(ATTACKS)]


def case_id(case):
  return f"n{case.n}-k{case.k}-{case.attack}"


def make_rows(case):
  """(rows float32 (n, d): n - k honest rows mu + N(0, 1), then k copies of ONE Byzantine row; start float32 (d): a
  vector near mu).  empire 1.1 / little 1.5: attacks/identical.py:129-141 on the honest rows."""
  rng = np.random.default_rng(case.seed)
  h = case.n - case.k
  mu = rng.normal(size=case.d)
  honest = (mu + rng.normal(size=(h, case.d))).astype(np.float32)
  avg = honest.astype(np.float64).mean(axis=0)
  if case.attack == "empire":
    byz = avg + 1.1 * (-avg)
  elif case.attack == "little":
    byz = avg + 1.5 * honest.astype(np.float64).std(axis=0, ddof=1)
  elif case.attack == "far":
    byz = avg + 30.0 * rng.normal(size=case.d)
  else:
    byz = honest[0].astype(np.float64)
  rows = np.concatenate([honest, np.repeat(byz.astype(np.float32)[None, :], case.k, axis=0)])
  start = (mu + 0.1 * rng.normal(size=case.d)).astype(np.float32)
  return rows, start


def params(case, mode):
  """(param, iters) of the issue's cases: geomed nu = 1e-6 sqrt(d), 32 iterations; cclip tau = sqrt(d), 3 iterations."""
  if mode == "geomed":
    return 1e-6 * math.sqrt(case.d), GEOMED_ITERS
  return math.sqrt(case.d), CCLIP_ITERS


def exact_sqdist(points):
  """N x N squared distances of float32 points, differences and sums in float64."""
  p = np.asarray(points, dtype=np.float64)
  n = p.shape[0]
  sq = np.zeros((n, n))
  for i in range(n):
    diff = p - p[i]
    sq[i] = np.einsum("ij,ij->i", diff, diff)
  return sq


def vector_iteration(rows, mode, param, iters, tol=0.0, start=None):
  """The rule ON THE VECTORS in float64: (v, iterations run)."""
  x = np.asarray(rows, dtype=np.float64)
  n = x.shape[0]
  v = x.mean(axis=0) if start is None else np.asarray(start, dtype=np.float64)
  done = 0
  for _ in range(iters):
    r = np.sqrt(np.einsum("ij,ij->i", x - v, x - v))
    if mode == "geomed":
      w = 1.0 / np.maximum(param, r)
      nxt = (w[:, None] * x).sum(axis=0) / w.sum()
    else:
      with np.errstate(divide="ignore"):
        s = np.where(r <= param, 1.0, param / r)
      nxt = v + (s[:, None] * (x - v)).sum(axis=0) / n
    move = math.sqrt(float(np.dot(nxt - v, nxt - v)))
    v = nxt
    done += 1
    if tol > 0 and move <= tol:
      break
  return v, done


def host_weights(lib, sq, n, mode, param, iters, tol=0.0, has_start=False):
  """bm_center_weights on a float64 numpy matrix: (code, weights (64,), info (3,))."""
  sq = np.ascontiguousarray(sq, dtype=np.float64)
  weights = np.full(64, -7.0)
  info = np.full(3, -7.0)
  code = lib.bm_center_weights(sq.ctypes.data_as(ctypes.c_void_p), n, 1 if has_start else 0,
                               {"geomed": 0, "cclip": 1}[mode], float(param), int(iters), float(tol),
                               weights.ctypes.data_as(ctypes.c_void_p), info.ctypes.data_as(ctypes.c_void_p))
  return code, weights, info


def combine(weights, points):
  """sum_i weights[i] points[i] in float64."""
  p = np.asarray(points, dtype=np.float64)
  return (np.asarray(weights, dtype=np.float64)[:p.shape[0], None] * p).sum(axis=0)


def relative_error(v, ref):
  return float(np.linalg.norm(v - ref) / np.linalg.norm(ref))


def weighted_sum_reference(points, weights):
  """What bm_weighted_sum is measured against: (float64 sum_i w_i x_i, bound per coordinate) with w_i = float32 of
  the fp64 weights, rows that are the same object merged (weights added in index order in float64, then rounded) and
  groups of fp32 weight 0 dropped.  bound = (N + 1) 2^-24 sum_i |w_i x_i|: N fused steps plus the rounding of each
  weight.  `points`: a list of numpy rows, aliased entries being the same object."""
  groups = collections.OrderedDict()
  for p, c in zip(points, weights):
    groups.setdefault(id(p), [p, 0.0])
    groups[id(p)][1] += float(c)
  total = np.zeros(points[0].shape[0])
  mass = np.zeros(points[0].shape[0])
  for p, c in groups.values():
    w = np.float32(c)
    if w == 0:
      continue
    term = float(w) * p.astype(np.float64)
    total += term
    mass += np.abs(term)
  return total, (len(points) + 1) * 2.0 ** -24 * mass


# The bit-for-bit cases of bm_weighted_sum (tests/test_gpu_weighted_sum.py): (rows, d, floats behind a 256-byte boundary,
# seed).  "aliased": the stack of test_aliased_rows_are_one_group, 7 rows of which the last is referenced 5 times.
WsumCase = collections.namedtuple("WsumCase", "name n d offset seed")
WSUM_EXACT_CASES = (WsumCase("n11-align16", 11, 4099, 0, 11), WsumCase("n11-align8", 11, 4099, 2, 12),
                    WsumCase("n11-align4", 11, 4099, 1, 13), WsumCase("n64", 64, 1027, 0, 64),
                    WsumCase("aliased", 7, 4099, 0, 7), WsumCase("tail-only", 11, 3, 0, 3))


def wsum_exact_inputs(case):
  """(distinct float32 rows, stack: the index of the row behind each entry, float64 weights, one per entry)."""
  rng = np.random.default_rng(case.seed)
  rows = [rng.normal(size=case.d).astype(np.float32) for _ in range(case.n)]
  stack = list(range(6)) + [6] * 5 if case.name == "aliased" else list(range(case.n))
  weights = rng.uniform(0.01, 0.2, size=len(stack)) if case.name == "aliased" else rng.normal(size=len(stack))
  return rows, stack, [float(w) for w in weights]


def weighted_sum_exact(points, weights):
  """The definition of bm_weighted_sum evaluated on the CPU: (float32 result, number of fused steps whose emulation met
  a midpoint).  Weights of entries that are the same object are added in float64 in index order and rounded once to
  fp32, groups of fp32 weight 0 are dropped, then acc = 0; acc = fma(w_k, x_k, acc) over the groups in index order.  The
  fma is tests/first_pass_matrix.fma_emulated — exact except where its float64 sum is an fp32 midpoint, which the
  second number counts: a case is usable bit for bit only when it is 0."""
  import torch
  from tests.first_pass_matrix import fma_emulated
  groups = collections.OrderedDict()
  for p, c in zip(points, weights):
    groups.setdefault(id(p), [p, 0.0])
    groups[id(p)][1] += float(c)
  acc = torch.zeros(points[0].shape[0], dtype=torch.float32)
  midpoints = 0
  for p, c in groups.values():
    w = np.float32(c)
    if w == 0:
      continue
    acc, mid = fma_emulated(float(w), torch.from_numpy(p), 1.0, acc)
    midpoints += int(mid.sum())
  return acc.numpy(), midpoints
