"""Float64 numpy reference of the Min-Max / Min-Sum attacks (Shejwalkar & Houmansadr, NDSS 2021) for the tests: the
closed form of include/bm_gar.h and the paper's halving search on the vectors.  Both know rows, differences and sums
only — no kernel, no library call.  TEST INFRASTRUCTURE."""

import math

import numpy as np

PERTURBATIONS = ("unit", "std", "sign")
MODES = ("minmax", "minsum")
SLOTS = 66  # BM_PERTURB_SLOTS: b_0 .. b_63 | P | N
STRUCTURES = ("iid", "common", "scaled")


def stack(h, d, structure, seed):
  """h seeded rows of d coordinates (float64): iid normal; a common component of 5 sigma; half the rows scaled by 0.05."""
  rng = np.random.default_rng(1000003 * seed + 1009 * h + d)
  rows = rng.standard_normal((h, d))
  if structure == "common":
    rows = rows + 5.0 * rng.standard_normal(d)
  elif structure == "scaled":
    rows[: h // 2] *= 0.05
  elif structure != "iid":
    raise ValueError(structure)
  return rows


def seq_mean32(rows32):
  """The sequential fp32 mean bm_stack_stats writes: ((x_0 + x_1) + ...) / h, every operation rounded to fp32."""
  s = rows32[0].astype(np.float32).copy()
  for r in rows32[1:]:
    s = (s + r.astype(np.float32)).astype(np.float32)
  return (s / np.float32(len(rows32))).astype(np.float32)


def direction(rows, avg, perturbation):
  """p of the definition, in the precision of its arguments."""
  if perturbation == "unit":
    return -avg
  if perturbation == "std":
    q = ((rows - avg) ** 2).sum(axis=0)
    return -np.sqrt(q / (len(rows) - 1))
  if perturbation == "sign":
    return -np.sign(avg)
  raise ValueError(perturbation)


def distances(rows):
  """D_ij = |g_i - g_j|^2 from the differences."""
  h = len(rows)
  D = np.zeros((h, h))
  for i in range(h):
    diff = rows - rows[i]
    D[i] = (diff * diff).sum(axis=1)
  return D


def scalars(rows, avg, p):
  """[b_0 .. b_{h-1}, zeros, P, N]: b_i = <p, avg - g_i> from the differences."""
  scal = np.zeros(SLOTS)
  for i in range(len(rows)):
    scal[i] = (p * (avg - rows[i])).sum()
  scal[64], scal[65] = (p * p).sum(), (avg * avg).sum()
  return scal


def closed_form(D, scal, h, mode):
  """{gamma, bound, binding, P, N, degenerate, gammas} by the definition of include/bm_gar.h, in float64."""
  D = np.asarray(D, dtype=np.float64).reshape(h, h)
  b, P, N = np.asarray(scal[:h], dtype=np.float64), float(scal[64]), float(scal[65])
  rowsum = D.sum(axis=1)
  with np.errstate(all="ignore"):
    a = rowsum / h - rowsum.sum() / (2.0 * h * h)
    a = np.where(a <= 0.0, 0.0, a)
    out = dict(gamma=0.0, binding=-1, P=P, N=N, degenerate=True, gammas=None)
    ok = P > 0.0 and math.isfinite(P)
    if mode == "minmax":
      upper = D[np.triu_indices(h, 1)]
      bound = math.nan if np.isnan(upper).any() else float(upper.max())
      out["bound"] = bound
      if not (ok and math.isfinite(bound) and np.isfinite(a).all() and np.isfinite(b).all()):
        return out
      disc = b * b + P * (bound - a)
      if (disc < 0.0).any():
        return out
      gammas = (-b + np.sqrt(disc)) / P
      arg = int(np.argmin(gammas))  # the first of equal minima: the lower index
      if not math.isfinite(gammas[arg]):
        return out
      out.update(gamma=float(gammas[arg]), binding=arg, degenerate=False, gammas=gammas)
      return out
    bound = float(rowsum.max()) if not np.isnan(rowsum).any() else math.nan
    out["bound"] = bound
    A, B = float(a.sum()), float(b.sum())
    disc = B * B + h * P * (bound - A)
    if not (ok and math.isfinite(bound) and math.isfinite(A) and math.isfinite(B) and disc >= 0.0):
      return out
    g = (-B + math.sqrt(disc)) / (h * P)
    if math.isfinite(g):
      out.update(gamma=g, degenerate=False)
    return out


def attack(rows, perturbation, mode, avg=None, p=None):
  """The closed form on float64 rows (avg and p may be given: the device's own fp32 vectors, upcast)."""
  rows = np.asarray(rows, dtype=np.float64)
  avg = rows.mean(axis=0) if avg is None else np.asarray(avg, dtype=np.float64)
  p = direction(rows, avg, perturbation) if p is None else np.asarray(p, dtype=np.float64)
  res = closed_form(distances(rows), scalars(rows, avg, p), len(rows), mode)
  res["avg"], res["p"] = avg, p
  res["vector"] = avg + res["gamma"] * p
  return res


def objective(rows, m, mode):
  """(value, bound) of the attack's constraint for a Byzantine vector m: Min-Max max_i |m - g_i|^2 against
  R = max_{i<j} D_ij; Min-Sum sum_i |m - g_i|^2 against S = max_i sum_j D_ij."""
  rows = np.asarray(rows, dtype=np.float64)
  d2 = ((rows - m) ** 2).sum(axis=1)
  D = distances(rows)
  if mode == "minmax":
    return float(d2.max()), float(D.max())
  return float(d2.sum()), float(D.sum(axis=1).max())


def paper_search(rows, avg, p, mode, init, tau=1e-9):
  """The oscillating halving search of the paper's code on the vectors: from the factor `init`, a factor that keeps the
  constraint is remembered and the step (half the previous one) is added, else subtracted, until the remembered and
  the current factor are within tau."""
  rows = np.asarray(rows, dtype=np.float64)
  D = distances(rows)
  bound = float(D.max()) if mode == "minmax" else float(D.sum(axis=1).max())
  lam, lam_fail, lam_succ = float(init), float(init), 0.0
  while abs(lam_succ - lam) > tau:
    d2 = ((rows - (avg + lam * p)) ** 2).sum(axis=1)
    value = float(d2.max()) if mode == "minmax" else float(d2.sum())
    if value <= bound:
      lam_succ = lam
      lam = lam + lam_fail / 2
    else:
      lam = lam - lam_fail / 2
    lam_fail = lam_fail / 2
  return lam_succ
