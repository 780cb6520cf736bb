"""Restatements of the reference's `nan`, `bulyan` and `empire-strict` attacks (attacks/nan.py:24-40,
attacks/identical.py:45-86,114-127, attacks/empire.py:29-64) for the tests — TEST INFRASTRUCTURE.

  restate(..., precision="f32")  the reference's own fp32 torch-CPU operations in its order: bit-identical to it (pinned
                                 by the fixtures tests/golden/attacks/*.npz and, where a reference checkout is staged,
                                 by the live attacks)
  restate(..., precision="f64")  the same vectors, the OBJECTIVE of the factor search taken in float64: what the
                                 project's search forms compute (as oracle.gar_oracle.identical_attack(precision="f64"))
  vector_from(...)               the fp32 expression of the Byzantine vector on a given average and factor

`Loop` is the simulation step of oracle/step_oracle.py with the Byzantine vector handed in from outside.
"""

import collections
import json
import math
import os
import sys

import torch

from oracle import gar_oracle as O
from oracle import reference_loader
from oracle.step_oracle import RULES

Restated = collections.namedtuple("Restated", "vector factor trace")

ATTACKS = ("nan", "bulyan", "empire-strict")


def direction_of(avg, target_idx):
  """attacks/identical.py:114-127."""
  if target_idx == "all":
    return torch.ones_like(avg)
  assert isinstance(target_idx, int)
  att = torch.zeros_like(avg)
  att[target_idx] = 1
  return att


def seq_mean(rows):
  """attacks/empire.py:46-49 (and the sequential mean of the step's first pass)."""
  avg = rows[0].clone()
  for g in rows[1:]:
    avg.add_(g)
  return avg.div_(len(rows))


def vector_from(attack, avg, factor=None, target_idx=-1):
  """The Byzantine vector from the average: identical.py:82-84 with the signed factor, empire.py:61-62 with epsilon."""
  if attack == "nan":
    return torch.full_like(avg, math.nan)
  if attack == "bulyan":
    att = direction_of(avg, target_idx)
    att.mul_(factor)
    return avg.add(att)
  return avg.mul(-factor)


def oracle_rule(gar):
  """defense(gradients, f) of the CPU oracle."""
  if gar == "median":
    return lambda grads, f: O.median(grads)
  if gar == "average":
    return lambda grads, f: O.average(grads)
  return lambda grads, f: RULES[gar](grads, f)


def restate(attack, honests, f_real, f_decl=None, defense=None, arg=None, negative=False, target_idx=-1, precision="f32",
            avg=None):
  """`arg`: the attack's `factor` (bulyan) or `epsilon` (empire-strict): positive = fixed, negative = -evaluations.
  defense(gradients, f) -> vector.  avg: the honest average to use instead of the attack's own (the step's).
  -> Restated(vector, the factor / epsilon applied, [(x, y)] of the search or None)."""
  honests = list(honests)
  if f_real == 0:
    return Restated(None, None, None)
  if attack == "nan":
    return Restated(vector_from("nan", honests[0]), None, None)

  def objective(cand):
    out = defense(honests + [cand] * f_real, f_decl)
    if precision == "f32":
      out = out.sub(avg)
      return out.dot(out).item()
    diff = out.double() - avg.double()
    return diff.dot(diff).item()

  trace = None
  if attack == "bulyan":
    if avg is None:
      avg = torch.stack(honests).mean(dim=0)
    att = direction_of(avg, target_idx)
    factor = arg
    if factor < 0:
      factor, trace = O.line_maximize(lambda x: objective(avg + (-x if negative else x) * att), evals=math.ceil(-factor))
    elif negative:
      factor = -factor
    return Restated(vector_from("bulyan", avg, factor, target_idx), factor, trace)
  assert attack == "empire-strict" and not negative
  if avg is None:
    avg = seq_mean(honests)
  epsilon = arg
  if epsilon < 0:
    epsilon, trace = O.line_maximize(lambda x: objective(avg.mul(-x)), evals=math.ceil(-epsilon))
  return Restated(vector_from("empire-strict", avg, epsilon), epsilon, trace)


def reference_attack(name):
  """The unmodified `attacks.attacks[name].unchecked` of the staged reference checkout (reference_loader.available())."""
  reference_loader.load(with_native=False)  # its `tools` package, which `attacks` imports
  saved = (sys.stdout, sys.stderr, sys.excepthook)
  saved_path = list(sys.path)
  try:
    sys.path.insert(0, reference_loader.REFERENCE_DIR)
    import attacks
  finally:
    sys.stdout, sys.stderr, sys.excepthook = saved
    sys.path[:] = saved_path
  return attacks.attacks[name].unchecked


def reference_rule(gar):
  """The reference's own rule, as the `defense` its attacks call: defense(gradients=..., f=..., model=...)."""
  return reference_loader.load(with_native=False)[0].gars[gar].unchecked


def reference_kwargs(case):
  """The keyword arguments the reference's attack takes for a case (besides grad_honests, f_real, f_decl, defense, model)."""
  if case["attack"] == "bulyan":
    return dict(factor=case["arg"], negative=case["negative"], target_idx=case["target_idx"])
  if case["attack"] == "empire-strict":
    return dict(epsilon=case["arg"])
  return {}


# ---------------------------------------------------------------------------- #
# The committed fixtures (scripts/make_golden_attacks.py)

# (a directory of their own: tests/golden_io.py takes every tests/golden/*.npz for a fixture of the aggregation rules)
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attacks")
D = 203
EVALS = 8
FIRST_SEED = 3


def _case(attack, n, f, arg=None, negative=False, target_idx=-1, gar=None):
  return dict(attack=attack, n=n, f=f, arg=arg, negative=negative, target_idx=target_idx, gar=gar)


def _name(c):
  parts = [c["attack"].replace("-", ""), f"n{c['n']}", f"f{c['f']}"]
  if c["attack"] == "bulyan":
    parts.append("all" if c["target_idx"] == "all" else f"t{c['target_idx']}".replace("-", "m"))
  if c["arg"] is not None:
    parts.append(f"search{-c['arg']}" if c["arg"] < 0 else f"x{c['arg']}")
  if c["negative"]:
    parts.append("neg")
  if c["gar"]:
    parts.append(c["gar"])
  return "_".join(parts)


_LIST = []
for _n, _f in ((7, 1), (11, 2)):
  _LIST += [_case("nan", _n, _f),
            _case("bulyan", _n, _f, 1.5), _case("bulyan", _n, _f, 2.0, True, 17), _case("bulyan", _n, _f, 0.75, False, "all"),
            _case("empire-strict", _n, _f, 1 if _n == 7 else 3),
            _case("bulyan", _n, _f, -EVALS, gar="krum"), _case("empire-strict", _n, _f, -EVALS, gar="krum")]
_LIST += [_case("bulyan", 11, 2, -EVALS, gar=g) for g in ("median", "trmean", "bulyan", "cge")]
_LIST += [_case("bulyan", 11, 2, -EVALS, True, gar="median"), _case("bulyan", 11, 2, -EVALS, False, "all", gar="trmean"),
          _case("bulyan", 11, 2, -EVALS, True, "all", gar="krum")]
_LIST += [_case("empire-strict", 11, 2, -EVALS, gar=g) for g in ("median", "trmean", "cge")]
_LIST += [_case("bulyan", 25, 5, 1.25, False, "all"), _case("bulyan", 25, 5, -EVALS, False, "all", gar="krum")]
CASES = {_name(c): c for c in _LIST}
assert len(CASES) == len(_LIST)
FIXED = sorted(k for k, c in CASES.items() if c["arg"] is None or c["arg"] > 0)
SEARCHED = sorted(k for k, c in CASES.items() if c["arg"] is not None and c["arg"] < 0)


class Fixture:
  def __init__(self, name):
    import numpy as np
    data = np.load(os.path.join(GOLDEN_DIR, f"{name}.npz"))
    self.name = name
    self.case = json.loads(str(data["case"]))
    self.seed = int(data["seed"])
    self.honests = [torch.from_numpy(row.copy()) for row in data["in_honest"]]
    self.vector = torch.from_numpy(data["vector"].copy())
    self.factor = float(data["factor"]) if "factor" in data.files else None
    self.f = self.case["f"]


# ---------------------------------------------------------------------------- #
# The simulation step around a Byzantine vector handed in (oracle/step_oracle.py's loop, attack.py:757-878)

def same_values(a, b):
  """torch.equal with NaN equal to NaN."""
  return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0))


class Loop:
  def __init__(self, n, f_decl, f_real, gar, momentum_at="worker", mu=0.9, damp=0.9, clip=None, nb_past=3):
    self.n, self.f_decl, self.f_real, self.gar, self.h = n, f_decl, f_real, gar, n - f_real
    self.momentum_at, self.mu, self.damp, self.clip, self.nb_past = momentum_at, mu, damp, clip, nb_past
    self.workers, self.server = None, None
    self.pasts = collections.deque(maxlen=max(nb_past, 1))

  def cge_order(self, grads):
    """CGE's ranking by float64 norms (what the library ranks by)."""
    norms = [math.sqrt(g.double().pow(2).sum().item()) for g in grads]
    return sorted(range(len(grads)), key=lambda i: norms[i] if math.isfinite(norms[i]) else math.inf)

  def rule(self, grads):
    if self.gar == "cge":  # the reference's sequential fp32 mean (cge.py:50-57) over that ranking
      keep = len(grads) - self.f_decl
      order = self.cge_order(grads)
      acc = grads[order[0]].clone()
      for i in order[1:keep]:
        acc.add_(grads[i])
      return acc.div_(keep)
    return oracle_rule(self.gar)(grads, self.f_decl)

  def accept_ratio(self, grads):
    """attack.py:822 with the rules' own `influence`: Byzantine rows among those averaged; math.nan without one."""
    if self.gar == "krum":
      m = self.n - self.f_decl - 2
      return sum(1 for i in O.krum_order(grads, self.f_decl)[0][:m] if i >= self.h) / m
    if self.gar == "cge":
      keep = self.n - self.f_decl
      return sum(1 for i in self.cge_order(grads)[:keep] if i >= self.h) / keep
    return math.nan

  def begin(self, sampled, clip_f32=False):
    """Clipping and momentum placement of one step on fp32 CPU tensors -> (honests, their sequential mean)."""
    h = self.h
    sampled = [g.clone() for g in sampled]
    if self.clip is not None:
      for i, g in enumerate(sampled):
        norm = math.sqrt(g.double().pow(2).sum().item())
        if norm > self.clip:
          # (the step's clipping factor is an fp32 number: clip_f32 rounds it the same way)
          g.mul_(torch.tensor(self.clip / norm, dtype=torch.float64).float() if clip_f32 else self.clip / norm)
    if self.workers is None:
      self.workers = [torch.zeros_like(g) for g in sampled[:h]]
      self.server = torch.zeros_like(sampled[0])
    if self.momentum_at == "worker":
      honests = O.worker_momentum(self.workers, sampled[:h], self.mu, self.damp)
    elif self.momentum_at == "server":
      honests = [g.mul(1. - self.damp).add_(self.server, alpha=self.mu) for g in sampled[:h]]
    else:
      honests = sampled[:h]
    self._now = (sampled, honests)
    return [g.clone() for g in honests], seq_mean(honests)

  def finish(self, vector):
    """The rest of the step with `vector` as the Byzantine gradient -> (defense, update, study floats)."""
    sampled, honests = self._now
    attacks = [vector] * self.f_real
    grads = list(honests) + attacks
    defense = self.rule(grads)
    accept = self.accept_ratio(grads)
    if self.momentum_at == "server":
      self.server = defense
      update = defense
    elif self.momentum_at == "update":
      self.server.mul_(self.mu).add_(defense, alpha=(1. - self.damp))
      update = self.server
    else:
      update = defense
    res = O.study_block(sampled, honests, attacks, defense, list(self.pasts) if self.nb_past > 0 else [], self.mu, "f64")
    res["accept_ratio"] = accept
    if self.nb_past > 0:
      self.pasts.appendleft((res["sampled_grad_avg"], res["sampled_norm_avg"]))
    return defense, update, res


def assert_floats_close_nan(got, want, tag="", tol=1e-5):
  """tests.step_reference.assert_floats_close with the NaN entries compared as NaN: where the expectation is NaN (the
  statistics of an all-NaN attack, of a defense that holds a NaN) the step's must be NaN too; the rest go through the
  usual bounds."""
  from tests.step_reference import assert_floats_close
  got, want = dict(got), dict(want)
  for key, value in list(want.items()):
    if isinstance(value, float) and math.isnan(value) and key in got and key != "accept_ratio":
      assert math.isnan(got[key]), (tag, key, got[key])
      got[key] = want[key] = 1.0
  for key, value in got.items():
    if isinstance(value, float) and key in want and key != "accept_ratio":
      assert not math.isnan(value), (tag, key, value, want[key])
  assert_floats_close(got, want, tag=tag, tol=tol)


def sampled_for_step(it, count, d):
  """Seeded sampled gradients of step `it`: a common drift and worker noises of distinct scales."""
  gen = torch.Generator().manual_seed(2000 + it)
  base = 0.2 * torch.randn(d, generator=gen)
  return [base + (0.5 + 0.1 * i) * torch.randn(d, generator=gen) for i in range(count)]
