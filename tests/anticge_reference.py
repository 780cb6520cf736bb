"""Restatements of the reference's `anticge` attack (attacks/anticge.py:49-78) for the tests — TEST INFRASTRUCTURE.

  anticge_f32  the reference's own fp32 torch-CPU operations in its order: bit-identical to it (pinned by the fixtures
               tests/golden/anticge/*.npz and, where a reference checkout is staged, by the live attack)
  anticge_f64  the same steps with every norm, sum and product in float64: what the arithmetic outputs of the device
               path are compared with

Both return an `Anticge` record: the norm order of the honest rows, the unscaled sum S (None on the NaN path) and the
attack vector.  `AnticgeLoop` is the simulation step of oracle/step_oracle.py with this attack in the place of the
"identical" ones.
"""

import collections
import math
import os
import sys

import torch

from oracle import gar_oracle as O
from oracle import reference_loader
from oracle.step_oracle import RULES

Anticge = collections.namedtuple("Anticge", "order sum vector")

MIN_NORM_GAP = 1e-4  # relative gap between consecutive sorted norms above which an fp64 and an fp32 ordering agree


def multiplier_of(vector, total):
  """The fp32 number m with `total * m` bit-identical to `vector` (None if there is none): how a vector whose norms
  came from another source than the restatement's fp32 `norm()` is compared with it — the sum must be the same bits,
  the multiplier may differ in its last places."""
  import numpy as np
  j = int(total.abs().argmax())
  m = np.float32(vector[j].item()) / np.float32(total[j].item())
  for cand in [m] + [step(m, k) for k in range(1, 9) for step in (_ulps_up, _ulps_down)]:
    if torch.equal(total * float(cand), vector):
      return float(cand)
  return None


def _ulps_up(m, k):
  import numpy as np
  for _ in range(k):
    m = np.nextafter(m, np.float32(np.inf))
  return m


def _ulps_down(m, k):
  import numpy as np
  for _ in range(k):
    m = np.nextafter(m, np.float32(-np.inf))
  return m


def _order(norms):
  keys = [v if math.isfinite(v) else math.inf for v in norms]
  return sorted(range(len(keys)), key=lambda i: keys[i]), keys


def check_arguments(h, f_decl):
  if not 1 <= f_decl <= h:
    raise ValueError(f"anticge indexes the sorted norms at h - f_decl: 1 <= f_decl <= {h} needed, got {f_decl}")


def norm_gap(honests):
  """Smallest relative gap between consecutive sorted (float64) norms of the rows; inf for a single row."""
  norms = sorted(math.sqrt(g.double().pow(2).sum().item()) for g in honests)
  return min(((b - a) / b for a, b in zip(norms, norms[1:]) if b > 0), default=math.inf)


def _anticge(rows, f_decl, f_real, norm):
  """attacks/anticge.py:59-78 on `rows` in their own dtype, `norm(row)` giving each norm as a Python float."""
  if f_real > f_decl:
    return Anticge(None, None, torch.full_like(rows[0], math.nan))
  check_arguments(len(rows), f_decl)
  order, keys = _order([norm(g) for g in rows])
  maxpos = len(rows) - f_decl
  maxnorm = math.nextafter(keys[order[maxpos]], 0)
  total = rows[order[0]].clone()
  for i in order[:maxpos]:
    total.add_(rows[i])
  vector = total.clone()
  attnorm = norm(vector)
  if attnorm > 0:
    vector.mul_(-maxnorm / attnorm)
  return Anticge(order, total, vector)


def anticge_f32(honests, f_decl, f_real):
  return _anticge(list(honests), f_decl, f_real, lambda g: g.norm().item())


def anticge_f64(honests, f_decl, f_real):
  rows = [g.detach().to("cpu", torch.float64) for g in honests]
  return _anticge(rows, f_decl, f_real, lambda g: math.sqrt(g.pow(2).sum().item()))


def reference_attack():
  """The unmodified `attacks.attacks["anticge"]` of the staged reference checkout (reference_loader.available())."""
  reference_loader.load(with_native=False)  # its `tools` package, which `attacks` imports
  saved = (sys.stdout, sys.stderr, sys.excepthook)
  saved_path = list(sys.path)
  try:
    sys.path.insert(0, reference_loader.REFERENCE_DIR)
    import attacks
  finally:
    sys.stdout, sys.stderr, sys.excepthook = saved
    sys.path[:] = saved_path
  return attacks.attacks["anticge"].unchecked


def reference_order(honests):
  """The order the reference's `_compute_normed` puts the rows in (indices; rows are identified by object)."""
  reference_attack()
  normed = sys.modules["attacks.anticge"]._compute_normed(honests)
  where = {id(g): i for i, g in enumerate(honests)}
  return [where[id(g)] for _, g in normed]


# ---------------------------------------------------------------------------- #
# The committed fixtures (scripts/make_golden_anticge.py)

# (a directory of their own: tests/golden_io.py takes every tests/golden/*.npz for a fixture of the aggregation rules)
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anticge")
# name -> (kind, n, f, d): O.make_stack(kind, n, f, d, seed=3), attacked with f_decl = f_real = f
STACKS = {f"{kind}_n{n}_f{f}": (kind, n, f, d)
          for kind in ("hetero", "momentum")
          for n, f, d in ((7, 1, 130), (11, 2, 1031), (25, 5, 1031), (25, 11, 1031), (51, 12, 257))}
# name -> (kind, n, f, d, f_decl, f_real): f_decl = h (S is the smallest row alone) and f_real > f_decl (all NaN)
EXTRAS = {"hetero_n7_fdecl6": ("hetero", 7, 1, 130, 6, 1),
          "hetero_n7_freal2": ("hetero", 7, 1, 130, 1, 2)}
CASES = sorted(STACKS) + sorted(EXTRAS)


class Fixture:
  def __init__(self, name):
    import numpy as np
    data = np.load(os.path.join(GOLDEN_DIR, f"{name}.npz"))
    self.name = name
    self.honests = [torch.from_numpy(row.copy()) for row in data["in_honest"]]
    self.f_decl, self.f_real = (int(v) for v in data["meta"])
    self.vector = torch.from_numpy(data["vector"].copy())
    self.order = [int(v) for v in data["order"]] if "order" in data.files else None


# ---------------------------------------------------------------------------- #
# The simulation step with this attack (oracle/step_oracle.py's loop, attack.py:757-878)

class AnticgeLoop:
  def __init__(self, n, f_decl, f_real, gar, momentum_at="worker", mu=0.9, damp=0.9, clip=None, nb_past=3):
    self.n, self.f_decl, self.f_real, self.gar, self.h = n, f_decl, f_real, gar, n - f_real
    self.momentum_at, self.mu, self.damp, self.clip, self.nb_past = momentum_at, mu, damp, clip, nb_past
    self.workers, self.server = None, None
    self.pasts = collections.deque(maxlen=max(nb_past, 1))

  def rule(self, grads):
    if self.gar == "median":
      return O.median(grads)
    if self.gar == "average":
      return O.average(grads)
    if self.gar == "cge":
      return self.cge(grads)[0]
    return RULES[self.gar](grads, self.f_decl)

  def cge(self, grads, byz_scale=1.0):
    """CGE ranked by float64 norms (what the library ranks by), then the reference's sequential fp32 mean (cge.py:50-57);
    `byz_scale` multiplies the norms of the Byzantine rows in the ranking only.  -> (mean, the rows kept)"""
    keep = len(grads) - self.f_decl
    norms = [math.sqrt(g.double().pow(2).sum().item()) * (byz_scale if i >= self.h else 1.0) for i, g in enumerate(grads)]
    order = sorted(range(len(grads)), key=lambda i: norms[i] if math.isfinite(norms[i]) else math.inf)
    acc = grads[order[0]].clone()
    for i in order[1:keep]:
      acc.add_(grads[i])
    return acc.div_(keep), sorted(order[:keep])

  def begin(self, sampled):
    """Clipping and momentum placement of one step on fp32 CPU tensors -> (honests, Anticge of them)."""
    h = self.h
    sampled = [g.clone() for g in sampled]
    if self.clip is not None:
      for g in sampled:
        norm = math.sqrt(g.double().pow(2).sum().item())
        if norm > self.clip:
          g.mul_(self.clip / norm)
    if self.workers is None:
      self.workers = [torch.zeros_like(g) for g in sampled[:h]]
      self.server = torch.zeros_like(sampled[0])
    if self.momentum_at == "worker":
      honests = O.worker_momentum(self.workers, sampled[:h], self.mu, self.damp)
    elif self.momentum_at == "server":
      honests = [g.mul(1. - self.damp).add_(self.server, alpha=self.mu) for g in sampled[:h]]
    else:
      honests = sampled[:h]
    attack = anticge_f32(honests, self.f_decl, self.f_real)
    self._now = (sampled, honests, attack)
    return [g.clone() for g in honests], attack

  def finish(self, vector, observed=None):
    """The rest of the step with `vector` as the Byzantine gradient (the one under test, once it has been compared with
    the restatement: the rule then ranks the same bits on both sides) -> (defense, update, study floats).
    observed: the defense of a path whose honest rows differ from these in their last bits (the device's momentum is
    fused multiply-adds).  The attack puts its vector within an fp32 rounding of the norm of a row CGE may keep
    (anticge.py:66-68) — the reference's own `norm()` does not resolve which of the two is smaller — so against CGE the
    ranking of the Byzantine rows is taken with their norm moved by 1e-6 either way as well (ten fp32 roundings), and
    the admissible defense closest to `observed` is the expectation.  An admissible selection may differ from the
    unmoved one only in Byzantine copies exchanged with g_(maxpos), the one row the attack aims at (asserted);
    `self.cge_choice` says which ranking was taken (1.0: the unmoved one)."""
    sampled, honests, attack = self._now
    attacks = [vector] * self.f_real
    grads = list(honests) + attacks
    defense = self.rule(grads)
    self.cge_choice = 1.0
    if observed is not None and self.gar == "cge" and 0 < self.f_real <= self.f_decl:
      kept = self.cge(grads)[1]
      exchangeable = set(range(self.h, len(grads))) | {attack.order[self.h - self.f_decl]}
      for scale in (1 - 1e-6, 1 + 1e-6):
        other, other_kept = self.cge(grads, scale)
        assert set(kept) ^ set(other_kept) <= exchangeable, (scale, kept, other_kept)
        if float((other - observed).abs().max()) < float((defense - observed).abs().max()):
          defense, self.cge_choice = other, scale
    if self.momentum_at == "server":
      self.server = defense
      update = defense
    elif self.momentum_at == "update":
      self.server.mul_(self.mu).add_(defense, alpha=(1. - self.damp))
      update = self.server
    else:
      update = defense
    res = O.study_block(sampled, honests, attacks, defense, list(self.pasts) if self.nb_past > 0 else [], self.mu, "f64")
    if self.nb_past > 0:
      self.pasts.appendleft((res["sampled_grad_avg"], res["sampled_norm_avg"]))
    return defense, update, res


def sampled_for_step(it, count, d):
  """Seeded sampled gradients of step `it`: a common drift and worker noises of distinct scales (distinct norms)."""
  gen = torch.Generator().manual_seed(1000 + it)
  base = 0.2 * torch.randn(d, generator=gen)
  return [base + (0.5 + 0.1 * i) * torch.randn(d, generator=gen) for i in range(count)]
