"""The graphed step: every configuration of AggregationStep.run() that graphs.GraphedCall records, replayed THREE times
on new gradients and held bit for bit against an eager twin.  TEST INFRASTRUCTURE (a helper module, not a conftest), shared
by tests/test_graph_matrix_cpu.py (case lists, plans, refusals and the twin itself against step_matrix.MatrixLoop on
tests/sharded_backend.OracleBackend, no GPU) and tests/test_gpu_graph_matrix.py (the HIP backend, the replays).

A replay runs the recorded kernels and none of run()'s Python, so whatever the step carries from one step to the next
must live where those kernels read and write it, and whatever the host cached of an earlier step must be forgotten.  One
replay on unchanged gradients shows neither; two show a frozen state, the third that it keeps moving.

Universe: tests/step_matrix.py's — RULES, ATTACKS, PLACEMENTS, GAR_ARGS, FF, D = 1027 — at nb_past = 0 (a step with a past
is refused: AggregationStep.graph_refusal) and world 1.  STEPS = 5: two warm-up steps of GraphedCall, three replays.
  product    14 rules x 12 attack forms x 3 placements at fixed factors, the secondary arguments laid over it by the
             step matrix's own formulas (clipping, (n, f_decl, f_real), a negative factor, m, params / origin,
             single_call) plus `extra`: one sampled gradient more than h, at EVERY step of the case (a recording holds
             one count)
  plan       the step matrix's PLAN cases: the six rules of the single call x {empire, little}, worker placement,
             f_real = 2 / 0, single_call on / off — with them every plan of the universe at nb_past = 0 is reached
  searched   every rule but Brute x {empire, little}, attack_evals = 8, line_search "auto", placements rotating
  pre        nnm and bucketing (s = 2), form "rows" and — krum, cclip — "scalars", x {median, krum, cclip} x placements
Every step of a case draws new gradients (step_matrix.sampled_rows at the step's index).
"""

import collections
import itertools
import math

import torch

from tests import step_matrix as SM

WARMUP, REPLAYS = 2, 3
STEPS = WARMUP + REPLAYS
EVALS = 8
SEARCHED_ATTACKS = ("empire", "little")
PRE_RULES = ("median", "krum", "cclip")
SCALAR_RULES = ("krum", "cclip")   # of PRE_RULES: what pre_args form="scalars" serves (pipelines.SCALAR_RULES)
BUCKET = 2
PRE_SEED = 5

Case = collections.namedtuple("Case", SM.Case._fields + ("nb_past", "extra", "evals", "pre", "pre_args"))


def _norm64(t):
  return math.sqrt(t.double().pow(2).sum().item())


def clip_value(count, seed, d=SM.D):
  """step_matrix.clip_value over this module's STEPS and `count` sampled rows: a norm that separates the same few
  largest rows from the others at every step."""
  steps = [sorted((_norm64(g) for g in SM.sampled_rows(seed, it, count, d)), reverse=True) for it in range(STEPS)]
  for k in range(1, count):
    lo, hi = max(norms[k] for norms in steps), min(norms[k - 1] for norms in steps)
    if hi - lo > 0.01 * hi:
      return round(0.5 * (lo + hi), 1)
  raise AssertionError("no clipping norm separates the same rows at every step")


# Seeds of the cases whose default draw puts a decision of the float64 loop under its threshold at one of the five steps
# (tests/test_graph_matrix_cpu.py asserts the margins): chosen once, then fixed.
SEEDS = {"bulyan-minmax-sign-update": 1,   # (seed 0: step 3, Bulyan's ranking at 6.4e-5 of its 1e-4)
         "dnc-hidden-last-update": 1,      # (seed 0: step 2, DnC's last removal under spectral_cases.MIN_MARGIN,
         "dnc-hidden-all-update": 1}       #  as in step_matrix.SEEDS)


def _make(name, rule, att, placement, ff, clip, negative, m, with_l2, single_call, group, extra=0, evals=None, pre=None,
          pre_args=None):
  n, f_decl, f_real = ff
  seed = SEEDS.get(name, 0)
  factor = att.negative if negative and att.negative is not None else att.factor
  return Case(name, rule, att.key, placement, n, f_decl, f_real,
              clip_value(n - f_real + extra, seed) if clip else None, m if rule in SM.DISTANCE else None, with_l2,
              single_call, factor, SM.D, seed, group, 0, extra, evals, pre, pre_args)


_CASES = None


def cases():
  global _CASES
  if _CASES is not None:
    return _CASES
  out = []
  # (the step matrix's own assignment of the secondary values: tests/step_matrix.cases)
  for (i, rule), (j, att), (k, placement) in itertools.product(enumerate(SM.RULES), enumerate(SM.ATTACKS),
                                                               enumerate(SM.PLACEMENTS)):
    ff = SM.FF[(i + 2 * j + k) % 4]
    if rule == "brute":
      ff = SM.FF[3] if (j, k) == (0, 2) else SM.FF[(i + j + k) % 3]
    out.append(_make(f"{rule}-{att.key}-{placement}", rule, att, placement, ff, clip=(i + j + k) % 2 == 1,
                     negative=(i + k) % 2 == 1, m=SM.M_ARG if (j + k) % 2 == 1 else None, with_l2=(j + k) % 2 == 0,
                     single_call=(i + j) % 2 == 0, group="product", extra=1 if (2 * i + j + k) % 3 == 0 else 0))
  # the single call both ways where the plan can take it (worker placement, the six rules, empire / little), with and
  # without somebody to attack: the step matrix's PLAN cases
  for rule, key in itertools.product(SM.DISTANCE + SM.COLWISE, SM.FIRST_PASS_ATTACKS):
    for ff, single in itertools.product((SM.FF[0], SM.FF[2]), (True, False)):
      out.append(_make(f"{rule}-{key}-worker-plan-f{ff[2]}-{'single' if single else 'sequence'}", rule, SM.ATTACK[key],
                       "worker", ff, clip=False, negative=False, m=None, with_l2=True, single_call=single, group="plan"))
  for i, rule in enumerate(r for r in SM.RULES if r != "brute"):
    for j, key in enumerate(SEARCHED_ATTACKS):
      placement = SM.PLACEMENTS[(i + j) % 3]
      out.append(_make(f"{rule}-{key}-{placement}-searched", rule, SM.ATTACK[key], placement, SM.FF[0], clip=False,
                       negative=False, m=None, with_l2=(i + j) % 2 == 0, single_call=False, group="searched",
                       evals=EVALS))
  for pre, rule, placement in itertools.product(("nnm", "bucketing"), PRE_RULES, SM.PLACEMENTS):
    for form in ("rows", "scalars") if rule in SCALAR_RULES else ("rows",):
      args = dict(form=form, **(dict(s=BUCKET, seed=PRE_SEED) if pre == "bucketing" else {}))
      out.append(_make(f"{rule}-empire-{placement}-{pre}-{form}", rule, SM.ATTACK["empire"], placement, SM.FF[0],
                       clip=False, negative=False, m=None, with_l2=False, single_call=False, group="pre", pre=pre,
                       pre_args=args))
  assert len({c.name for c in out}) == len(out)
  _CASES = out
  return out


def constructor_kwargs(case):
  """The keyword arguments of AggregationStep for a case (all but the aggregator)."""
  kwargs = SM.constructor_kwargs(case)
  assert kwargs["nb_past"] == 0
  kwargs.update(attack_evals=case.evals, line_search="auto", pre=case.pre, pre_args=case.pre_args)
  return kwargs


def inputs(case):
  """[(sampled rows, params or None, origin or None)] of the case's STEPS steps: new rows at every step, h + extra of
  them; the parameters move by a seeded vector per step."""
  count = case.n - case.f_real + case.extra
  gen = torch.Generator().manual_seed(50 + case.seed)
  origin = torch.randn(case.d, generator=gen)
  out = []
  for it in range(STEPS):
    params = origin + 0.05 * it * torch.randn(case.d, generator=gen)
    rows = SM.sampled_rows(case.seed, it, count, case.d)
    out.append((rows, params if case.with_l2 else None, origin if case.with_l2 else None))
  return out


def plain(value):
  """A value of floats() / last_search as something `==` compares the way the matrix means it: NaN equal to NaN."""
  if isinstance(value, float) and math.isnan(value):
    return None
  if isinstance(value, (list, tuple)):
    return [plain(v) for v in value]
  return value


def snapshot(step, defense):
  """Everything the matrix compares after a step, read through the step's getters and copied to the host."""
  def cpu(t):
    return None if t is None else t.detach().cpu().clone()

  factor, byz = step.last_factor, step.last_byzantine
  return dict(
    defense=cpu(defense), update=cpu(step.update_gradient()), byzantine=cpu(byz),
    buffers=None if step.buffers is None else [cpu(b) for b in step.buffers], server_momentum=cpu(step.server_momentum),
    cclip_start=cpu(step.cclip_start), last_masks=cpu(step.last_masks),
    last_factor=cpu(factor) if isinstance(factor, torch.Tensor) else plain(factor), last_search=plain(step.last_search),
    attack_info=cpu(getattr(byz, "attack_info", None)),
    floats={key: plain(value) for key, value in step.floats().items()})


def same(a, b):
  if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
    return isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and SM.same_bits(a, b)
  if isinstance(a, list) and a and isinstance(a[0], torch.Tensor):
    return isinstance(b, list) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
  return a == b


def differences(got, want):
  """The keys of two snapshots that are not the same, bit for bit (floats: key by key)."""
  bad = [key for key in want if key != "floats" and not same(got[key], want[key])]
  assert set(got["floats"]) == set(want["floats"])
  bad += ["floats." + key for key in want["floats"] if got["floats"][key] != want["floats"][key]]
  return bad


def moved(before, after):
  """Whether the twin's outputs changed between two consecutive steps: the defense vector, or — where it is non-finite
  at every coordinate on both steps (the nan attack against a rule that does not filter it: NaN equals NaN) — the norm
  of the sampled average, which moves with the new gradients whatever the rule returns."""
  if not SM.same_bits(before["defense"], after["defense"]):
    return True
  if not bool(torch.isfinite(before["defense"]).any()):
    return before["floats"]["sampled_norm_avg"] != after["floats"]["sampled_norm_avg"]
  return False
