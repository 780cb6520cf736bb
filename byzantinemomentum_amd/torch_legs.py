"""The optional compute legs of sharded.ShardedAggregator in plain torch and Python floats, for a backend that does not
declare the capability (the oracle backend of the CPU tests): the arithmetic of the kernels they stand in for, bit for
bit where a test says so.  `Legs` resolves, once per aggregator, each optional leg to the backend's method or to its
stand-in here."""

import functools
import math

import torch

from . import _lib


def _anticge_sum_torch(backend, local, f_decl, sq):
  """bm_anticge_sum in plain torch for a backend without the kernel: (S, order, [sum S^2 here, |g_(maxpos)|^2])."""
  h = len(local)
  maxpos = h - f_decl
  keys = torch.where(torch.isfinite(sq[:h]), sq[:h], torch.full_like(sq[:h], math.inf))
  order = backend.argsort(keys, h)
  ranked = order[:h].tolist()
  attack = local[ranked[0]].clone()
  for i in ranked[:maxpos]:  # (the smallest row a second time first: anticge.py:70-72)
    attack.add_(local[i])
  return attack, order, torch.stack([attack.double().pow(2).sum(), keys[ranked[maxpos]]])


def _anticge_scale_torch(vec, scal):
  """bm_anticge_scale in plain torch: the norms as fp32 numbers, nextafter and quotient in double (anticge.py:68,74-76)."""
  attnorm, byznorm = scal.sqrt().float().tolist()
  if attnorm > 0:
    vec.mul_(-math.nextafter(byznorm, 0) / attnorm)
  return vec


def _perturb_stats_torch(backend, local, perturbation):
  """bm_perturb_stats in plain torch for a backend without the kernel: the backend's sequential fp32 average, the
  direction in fp32, the scalars as fp64 sums of the fp32 vectors."""
  h = len(local)
  avg = backend.stack_stats(local)[0]
  if perturbation == "unit":
    direction = avg.neg()
  elif perturbation == "std":
    direction = torch.stack(list(local)).var(dim=0).sqrt_().neg_() if avg.numel() else avg.clone()
  else:
    direction = torch.sign(avg).neg_()
  p64, a64 = direction.double(), avg.double()
  scal = torch.zeros(_lib.PERTURB_SLOTS, dtype=torch.float64, device=avg.device)
  for i in range(h):
    scal[i] = torch.dot(p64, a64 - local[i].double())
  scal[_lib.PERTURB_P], scal[_lib.PERTURB_N] = torch.dot(p64, p64), torch.dot(a64, a64)
  return avg, direction, scal


def _minmax_factor_torch(sq, scal, h, mode):
  """bm_minmax_factor in Python floats (fp64, plain index order: the host form's arithmetic): fp64[6]."""
  D = sq.reshape(-1)[:h * h].reshape(h, h).tolist()
  sc = scal.tolist()
  b, P, N = sc[:h], sc[_lib.PERTURB_P], sc[_lib.PERTURB_N]
  rowsum = []
  for i in range(h):
    t = 0.0
    for j in range(h):
      t = t + D[i][j]
    rowsum.append(t)
  total = 0.0
  for t in rowsum:
    total = total + t
  a = [max(rowsum[i] / h - total / (2.0 * h * h), 0.0) if not math.isnan(rowsum[i]) else math.nan for i in range(h)]
  gamma, binding, ok = 0.0, -1.0, P > 0.0 and math.isfinite(P)
  if mode == "minmax":
    pairs = [D[i][j] for i in range(h) for j in range(i + 1, h)]
    bound = math.nan if any(math.isnan(v) for v in pairs) else max(pairs)
    ok = ok and math.isfinite(bound) and all(math.isfinite(v) for v in a + b)
    if ok:
      disc = [b[i] * b[i] + P * (bound - a[i]) for i in range(h)]
      ok = all(v >= 0.0 for v in disc)
    if ok:
      cands = [(-b[i] + math.sqrt(disc[i])) / P for i in range(h)]
      best = min(range(h), key=lambda i: (cands[i], i))
      ok = math.isfinite(cands[best])
      if ok:
        gamma, binding = cands[best], float(best)
  else:
    bound = math.nan if any(math.isnan(v) for v in rowsum) else max(rowsum)
    A = B = 0.0
    for i in range(h):
      A, B = A + a[i], B + b[i]
    disc = B * B + h * P * (bound - A)
    ok = ok and math.isfinite(bound) and math.isfinite(A) and math.isfinite(B) and disc >= 0.0
    if ok:
      g = (-B + math.sqrt(disc)) / (h * P)
      ok = math.isfinite(g)
      gamma = g if ok else 0.0
  return torch.tensor([gamma, bound, binding, P, N, 0.0 if ok else 1.0], dtype=torch.float64, device=sq.device)


def _attack_vector_torch(kind, avg, factor, target, want_direction):
  """bm_attack_vector in plain torch for a backend without the kernel: the same fp32 expression at every coordinate,
  avg + factor * dir with dir in {0, 1} (never a copy of avg), the factor rounded to fp32 first."""
  if kind == "nan":
    return torch.full_like(avg, math.nan)
  if isinstance(factor, torch.Tensor):  # (a device search's float64[1]: rounded as the kernel rounds it)
    factor = factor.reshape(-1)[0].to(avg.device, torch.float32)
  else:
    factor = torch.tensor(float(factor), dtype=torch.float32, device=avg.device)
  if kind == "scale":
    return avg * factor
  direction = torch.ones_like(avg) if kind == "shift_all" else torch.zeros_like(avg)
  if kind == "shift_one" and target is not None and target >= 0:
    direction[target] = 1
  out = avg + factor * direction
  return (out, direction) if want_direction else out


def _center_weights_torch(sq, n, mode, param, iters, tol, has_start):
  """bm_center_weights in plain torch (fp64, where `sq` lives) for a backend without the kernel: the iteration of
  include/bm_gar.h on the weights — (weights fp64[MAX_ROWS], info fp64[3])."""
  N = n + (1 if has_start else 0)
  D = sq[:N, :N].to(torch.float64)
  weights = torch.zeros(_lib.MAX_ROWS, dtype=torch.float64, device=sq.device)
  off = ~torch.eye(N, dtype=torch.bool, device=sq.device)
  bad = (~torch.isfinite(D) & off).sum(dim=1)
  usable = ~((bad > 0) & (2 * bad >= N - 1))
  rows = usable.clone()
  rows[n:] = False
  U = int(rows.sum())
  if U == 0:
    weights[:N] = math.nan
    return weights, torch.tensor([0.0, math.nan, 0.0], dtype=torch.float64, device=sq.device)
  Dz = torch.where(torch.isfinite(D), D, torch.zeros_like(D))  # (a term of weight 0 is skipped, whatever D holds)
  blind = ~torch.isfinite(D)
  c = torch.zeros(N, dtype=torch.float64, device=sq.device)
  if has_start and bool(usable[n]):
    c[n] = 1.0
  else:
    c[rows] = 1.0 / U

  def dot_rows(w):  # sum_j w_j D_ij with the terms of weight 0 skipped; NaN where a term that counts is not finite
    t = Dz @ w
    return torch.where((blind & (w != 0)[None, :]).any(dim=1), torch.full_like(t, math.nan), t)

  done, move2 = 0, 0.0
  for _ in range(iters):
    t = dot_rows(c)
    q = (c * torch.where(c != 0, t, torch.zeros_like(t))).sum()
    r2 = t - 0.5 * q
    r = torch.where(torch.isfinite(r2), r2.clamp_min(0.0).sqrt(), torch.full_like(r2, math.inf))
    if mode == "geomed":
      w = torch.where(rows, 1.0 / r.clamp_min(param), torch.zeros_like(r))
      nxt = w / w.sum()
    else:
      s = torch.where(rows, torch.where(r <= param, torch.ones_like(r), param / r), torch.zeros_like(r))
      nxt = c * (1.0 - s.sum() / U) + s / U
    e = nxt - c
    c = nxt
    u = dot_rows(e)
    move2 = max(0.0, -0.5 * float((e * torch.where(e != 0, u, torch.zeros_like(u))).sum()))
    done += 1
    if tol > 0 and math.sqrt(move2) <= tol:
      break
  weights[:N] = c
  return weights, torch.tensor([float(done), move2, float(U)], dtype=torch.float64, device=sq.device)


def _spectral_weights_torch(sq, n, mode, count, power_iters):
  """bm_spectral_weights in plain torch (fp64, where `sq` lives) for a backend without the kernel: the filter of
  include/bm_gar.h on the squared distances — (weights fp64[MAX_ROWS], info fp64[4])."""
  D = sq.reshape(-1)[:n * n].reshape(n, n).to(torch.float64)
  weights = torch.zeros(_lib.MAX_ROWS, dtype=torch.float64, device=sq.device)
  off = ~torch.eye(n, dtype=torch.bool, device=sq.device)
  bad = (~torch.isfinite(D) & off).sum(dim=1)
  usable = ~((bad > 0) & (2 * bad >= n - 1))
  U = int(usable.sum())

  def info(rounds, lam, kept):
    return torch.tensor([float(rounds), lam, float(U), float(kept)], dtype=torch.float64, device=sq.device)

  if U == 0:
    weights[:n] = math.nan
    return weights, info(0, math.inf, -1)
  Dz = torch.where(usable[:, None] & usable[None, :], D, torch.zeros_like(D))  # (rows without weight take no part)

  def evaluate(c):  # (tau, lambda) of E(c), None when degenerate
    C = c.sum()
    live = c > 0
    r = torch.where(live, (Dz @ c) / C, torch.zeros_like(c))
    s = (c * r).sum() / C
    key = torch.where(live, c * (r - 0.5 * s), torch.zeros_like(c)).clamp_min(0.0)
    top = key.max()
    if not float(top) > 0:
      return None
    first = int((key == top).nonzero()[0])
    sc = c.sqrt()
    z = torch.zeros_like(c)
    z[first] = sc[first]

    def kz(z):
      Z = z.sum()
      return torch.where(live, -0.5 * (Dz @ z - r * Z - (r * z).sum() + s * Z), torch.zeros_like(c))

    for _ in range(power_iters):
      w = sc * kz(z) / C
      norm = float((w * w).sum().sqrt())
      if not (0 < norm < math.inf):
        break
      z = sc * (w / norm)
    q = kz(z)
    zq = float((z * q).sum())
    if not zq > 0:
      return None
    tau = torch.where(live, q * q, torch.zeros_like(q))
    return torch.where(torch.isnan(tau), torch.full_like(tau, math.inf), tau), float((c * q * q).sum() / (C * zq))

  c = usable.to(torch.float64)
  best, lam_best, kept, rounds = c / U, math.inf, -1, 0
  if mode == "caf":
    for rnd in range(n):
      C = float(c.sum())
      if not C > n - 2 * count:
        break
      ev = evaluate(c)
      if ev is None:
        break
      tau, lam = ev
      rounds = rnd + 1
      if lam < lam_best:
        best, lam_best, kept = c / C, lam, rnd
      tmax = float(tau.max())
      if not tmax > 0:
        break
      ratio = torch.where(tau == tmax, torch.ones_like(tau), tau / tmax)
      c = torch.where(c > 0, c * (1.0 - ratio), torch.zeros_like(c))
  else:
    ev = evaluate(c)
    tau = torch.zeros_like(c)
    if ev is not None:
      tau, lam_best, kept, rounds = ev[0], ev[1], 0, 1
    drop = max(0, count - (n - U))
    idx = torch.arange(n, device=sq.device)
    ahead = usable[None, :] & ((tau[None, :] > tau[:, None]) | ((tau[None, :] == tau[:, None]) & (idx[None, :] > idx[:, None])))
    keep = usable & (ahead.sum(dim=1) >= drop)
    best = keep.to(torch.float64) / (U - drop)
  weights[:n] = best
  return weights, info(rounds, lam_best, kept)


def _weighted_sum_torch(points, weights):
  """bm_weighted_sum in plain torch, accumulated in fp64: rows that are one tensor once, with their weights added; rows
  of weight 0 are not read; a NaN weight gives NaN everywhere."""
  w = weights[:len(points)].tolist()
  if any(math.isnan(x) for x in w):
    return torch.full_like(points[0], math.nan)
  groups = {}
  for p, x in zip(points, w):
    groups.setdefault(id(p), [p, 0.0])[1] += x
  acc = torch.zeros(points[0].shape, dtype=torch.float64, device=points[0].device)
  for p, x in groups.values():
    if x != 0.0:
      acc.add_(p.double(), alpha=x)
  return acc.to(points[0].dtype)


def _nnm_masks_torch(sq, n, f):
  """bm_nnm_masks in plain torch (fp64 ranking, where `sq` lives) for a backend without the kernel: row i and the
  n - f - 1 other rows of smallest distance, ties to the lower index, NaN last (a stable sort) — int64[MAX_ROWS]."""
  D = sq[:n, :n].to(torch.float64)
  words = []
  for i in range(n):
    others = [j for j in range(n) if j != i]
    order = torch.sort(D[i, others], stable=True).indices.tolist()  # NaN sorts last, equal keys keep their order
    word = 1 << i
    for t in order[:n - f - 1]:
      word |= 1 << others[t]
    words.append(word - (1 << 64) if word >= (1 << 63) else word)
  return torch.tensor(words + [0] * (_lib.MAX_ROWS - n), dtype=torch.int64, device=sq.device)


def _mix_rows_torch(rows, masks, n_out):
  """bm_mix_rows in plain torch: per output row the sequential fp32 sum, in index order, of the rows in its mask, then
  one division by their count.  A row outside the mask is not touched; an empty mask gives NaN."""
  n = len(rows)
  outs = []
  for word in masks[:n_out].tolist():
    members = [j for j in range(n) if (word >> j) & 1]
    acc = torch.zeros_like(rows[0])
    for j in members:
      acc = acc + rows[j]
    outs.append(acc / torch.tensor(float(len(members)), dtype=rows[0].dtype, device=rows[0].device))
  return outs


def _bucket_masks_torch(n, s, seed, counter, like):
  """bm_bucket_masks for a backend without the leg: the counter-based permutation in Python integers
  (gars.bucket_permutation) cut into buckets of s — int64[MAX_ROWS] where `like` lives, zeros beyond ceil(n / s).
  `counter`: a Python integer (a host counter: whoever calls advances it)."""
  from . import gars
  words = gars.bucket_masks(n, s, gars.bucket_permutation(n, seed, counter))
  words = [w - (1 << 64) if w >= (1 << 63) else w for w in words]
  return torch.tensor(words + [0] * (_lib.MAX_ROWS - len(words)), dtype=torch.int64, device=like.device)


def _mask_words(masks, count):
  return [int(w) & ((1 << 64) - 1) for w in masks[:count].tolist()]


def _mixed_sqdist_torch(sq, n_in, masks, n_out):
  """bm_mixed_sqdist for a backend without the kernel: the definition of include/bm_gar.h walked in Python floats (IEEE
  doubles, the sums in the stated order), so the host form's bits — fp64 (n_out, n_out) where `sq` lives.  Reads the
  matrix and the masks on the host."""
  D = sq.reshape(-1)[:n_in * n_in].view(n_in, n_in).tolist()
  words = _mask_words(masks, n_out)
  if any(w >> n_in for w in words):
    raise ValueError(f"mixed_sqdist: a mask has a bit at or above n_in = {n_in}")
  members = [[j for j in range(n_in) if (w >> j) & 1] for w in words]
  Q = [[0.0] * n_out for _ in range(n_in)]
  for i in range(n_in):
    for b in range(n_out):
      s = 0.0
      for j in members[b]:
        if j != i:
          s = s + D[min(i, j)][max(i, j)]
      Q[i][b] = s

  def P(a, b):
    s = 0.0
    for i in members[a]:
      s = s + Q[i][b]
    return s

  diag = [P(a, a) for a in range(n_out)]
  out = [[0.0] * n_out for _ in range(n_out)]
  for a in range(n_out):
    out[a][a] = 0.0 if words[a] else math.nan
    for b in range(a + 1, n_out):
      if not words[a] or not words[b]:
        v = math.nan
      elif words[a] == words[b]:
        v = 0.0
      else:
        x, y = (a, b) if words[a] < words[b] else (b, a)  # the smaller mask word walks the outer sum
        p, cx, cy = P(x, y), float(len(members[x])), float(len(members[y]))
        if not (math.isfinite(p) and math.isfinite(diag[x]) and math.isfinite(diag[y])):
          v = math.nan
        else:
          v = p / (cx * cy) - 0.5 * diag[x] / (cx * cx) - 0.5 * diag[y] / (cy * cy)
          v = 0.0 if v <= 0.0 else v
      out[a][b] = out[b][a] = v
  return torch.tensor(out, dtype=torch.float64, device=sq.device)


def _mix_weights_torch(masks, n_in, n_out, weights=None, selection=None, m=None):
  """bm_mix_weights for a backend without the kernel, in Python floats: the host form's bits — fp64[MAX_ROWS] where the
  weights / the selection live."""
  given = weights if weights is not None else selection
  words = _mask_words(masks, n_out)
  if any(w >> n_in for w in words):
    raise ValueError(f"mix_weights: a mask has a bit at or above n_in = {n_in}")
  ok = True
  if selection is not None:
    sel = [int(t) for t in selection[:m].tolist()]
    ok = all(0 <= t < n_out for t in sel)
    w = [0.0] * n_out
    if ok:
      for t in sel:
        w[t] = w[t] + 1.0 / float(m)
  else:
    w = weights[:n_out].tolist()
  ok = ok and all(w[r] == 0.0 or words[r] for r in range(n_out))
  out = [0.0] * _lib.MAX_ROWS
  for j in range(n_in):
    s = 0.0
    for r in range(n_out):
      if w[r] != 0.0 and (words[r] >> j) & 1:
        s = s + w[r] / float(bin(words[r]).count("1"))
    out[j] = s if ok else math.nan
  return torch.tensor(out, dtype=torch.float64, device=given.device)


def _anticge_torch(backend, local, f_decl, reduce):
  """HipBackend.anticge over a backend's `row_sqnorms` and `argsort` legs: the same steps, the same two reductions."""
  byz, _, scal = _anticge_sum_torch(backend, local, f_decl, reduce(backend.row_sqnorms(local)))
  reduce(scal[:1])
  return _anticge_scale_torch(byz, scal)


def _declared_only(name):
  def leg(*args, **kwargs):
    raise AttributeError(f"the backend declares the capability {name!r} and has no method of that name")
  return leg


class Legs:
  """The compute legs of one backend as ShardedAggregator and pipelines call them, resolved ONCE: each optional leg is
  the backend's method where the backend declares the capability, else its stand-in above (`native` names the former).
  `colwise_mixed` / `colwise_bucketed` (fusions, not steps) and `brute_select_device` (absent on the oracle backend) have
  no stand-in: None."""

  STAND_INS = {"center_weights": _center_weights_torch, "spectral_weights": _spectral_weights_torch,
               "weighted_sum": _weighted_sum_torch, "nnm_masks": _nnm_masks_torch, "mix_rows": _mix_rows_torch,
               "colwise_mixed": None, "colwise_bucketed": None, "bucket_masks": _bucket_masks_torch,
               "mixed_sqdist": _mixed_sqdist_torch, "mix_weights": _mix_weights_torch,
               "attack_vector": _attack_vector_torch, "perturb_stats": _perturb_stats_torch,
               "minmax_factor": _minmax_factor_torch, "anticge": _anticge_torch}
  TAKE_THE_BACKEND = ("perturb_stats", "anticge")

  def __init__(self, backend):
    self.backend = backend
    self.native = frozenset(getattr(backend, "capabilities", ())) & frozenset(self.STAND_INS)
    for name, stand_in in self.STAND_INS.items():
      if name in self.native:
        leg = getattr(backend, name, None) or _declared_only(name)  # (an error when called, as it was)
      elif name in self.TAKE_THE_BACKEND:
        leg = functools.partial(stand_in, backend)
      else:
        leg = stand_in
      setattr(self, name, leg)
    self.brute_select_device = getattr(backend, "brute_select_device", None)

  def rank(self, sq, n, f, m, mode):
    return self.backend.rank(sq, n, f, m, mode)

  def host_selection(self, sq, n, f, like):
    """The host Brute search on the squared distances `sq`, as an index tensor where `like` lives."""
    return self.backend.index_tensor(self.backend.brute_select(sq.sqrt().cpu().contiguous(), n, f), like)
