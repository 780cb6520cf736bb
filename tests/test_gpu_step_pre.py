"""AggregationStep with a pre-aggregation on the HIP backend: the comparison of tests/test_step_pre_cpu.py at d = 4099 —
the defense of every step against ShardedAggregator.nnm / .bucketing on the very stack the step aggregated, bit for bit,
the masks of consecutive steps from the device counter — then the "sqdist" plan against the same step on a backend without
the two fused distance legs (at d = 4099, and at h = 20 with the burst knob, where the fused first pass runs), and one
bucketing step recorded into a HIP graph.  Needs an MI355X: `pytest -m gpu`."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = 4099
RULES = {"median": {}, "trmean": {}, "krum": {}, "bulyan": {}, "average": {}, "geomed": dict(nu=1e-4, iters=3),
         "cclip": dict(tau=2.0, iters=2)}
SCALAR = ("krum", "average", "geomed", "cclip")
COMBOS = [(rule, pre, form) for rule in RULES for pre in ("nnm", "bucketing")
          for form in (("rows", "scalars") if rule in SCALAR else ("rows",))]
# the searched attack of this file is `little` (avg + x * std), not `empire`: the empire search proposes x = 0, 1, 3, 1.4
# with four evaluations, and at x = 1 its candidate is avg - avg = 0 — where the search lands there (it does on some of
# these stacks, and `negative` does not help: the factor is applied with its positive sign) the Byzantine vector is zero
# and floats() cannot form its cosines (a division by its norm, with or without a pre-aggregation).  avg + x * std is never
# the zero vector, so every step's study row is read.  The empire search through a pre-aggregation is what
# tests/test_step_pre_cpu.py runs
ATTACKS = {"empire": dict(attack="empire", attack_factor=1.1),
           "little-search": dict(attack="little", attack_evals=4),
           "anticge": dict(attack="anticge"), "minmax": dict(attack="minmax")}
PLACEMENTS = ("worker", "server", "update")
SEED = 7
# the fused distances differ from the stand-alone pass by its rounding, which DESIGN bounds at 1e-5 of fp64: a neighbour
# margin ten times above that keeps the masks of the two forms equal
MIN_MARGIN = 1e-4


def bucket_size(rule, n, f):
  # bulyan needs 4 f + 3 rows: buckets of one; the coordinate-wise rules 2 f + 1 means: buckets of two
  return 1 if rule == "bulyan" else 2


def pre_args_of(rule, pre, form, n, f):
  args = {"form": form}
  if pre == "bucketing":
    args.update(s=bucket_size(rule, n, f), seed=SEED)
  return args


def honest_rows(it, h, d=D, seed=0):
  """base + r_i * N(0, 1/16), r_i = 1 + 0.25 i: every row at its own distance from the others."""
  gen = torch.Generator().manual_seed(5000 + 100 * seed + it)
  base = torch.randn(d, generator=gen)
  return [(base + (1 + 0.25 * i) * 0.25 * torch.randn(d, generator=gen)).to(DEV) for i in range(h)]


def no_fused_distances():
  """A HipBackend without the two *_sqdist legs: the step then plans the plain first pass."""
  from byzantinemomentum_amd.sharded import HipBackend

  class Plain(HipBackend):
    capabilities = HipBackend.capabilities - {"momentum_stats_sqdist", "stack_stats_sqdist"}
  return Plain()


def aggregator(backend=None):
  from byzantinemomentum_amd.sharded import ShardedAggregator
  return ShardedAggregator(backend=backend, local_only=True)


def make_step(rule, pre, form, placement, attack, n, f, backend=None, **more):
  from byzantinemomentum_amd.step import AggregationStep
  return AggregationStep(n, f, f, gar=rule, gar_args=RULES[rule], momentum=0.9, dampening=0.9, momentum_at=placement,
                         nb_past=2, aggregator=aggregator(backend), pre=pre, pre_args=pre_args_of(rule, pre, form, n, f),
                         **dict(ATTACKS[attack], **more))


class Spy:
  """Keeps the stack the step's defense ran on."""

  def __init__(self, step):
    self.stack, self.first = None, None
    inner = step._defense

    def defense(first, attacks):
      self.first, self.stack = first, list(first.honests) + list(attacks)
      return inner(first, attacks)

    step._defense = defense


def expected_defense(rule, pre, form, stack, masks, start, n, f):
  from byzantinemomentum_amd.pipelines import NNM_RULES
  agg = aggregator()
  args = dict(RULES[rule])
  if rule == "cclip":
    args["start"] = start
  if pre == "nnm":
    return agg.nnm(stack, f, rule=rule, form=form, **args)
  if NNM_RULES[rule]:
    args["f"] = f
  return agg.bucketing(stack, bucket_size(rule, n, f), rule, masks=masks, form=form, **args)


def host_masks(rule, n, f, counter):
  from byzantinemomentum_amd import gars
  return gars.bucket_masks_host(n, bucket_size(rule, n, f), SEED, counter)


def same_bits(a, b):
  return torch.equal(a.view(torch.int32), b.view(torch.int32))


def neighbour_margin(stack, h, f):
  """min over rows of (D_(k+1) - D_(k)) / D_(k+1) at the boundary of nearest-neighbour mixing (k - 1 = n - f - 1 other rows
  are taken), in float64, with pairs of aliased copies left out (rows h .. n-1 are one tensor: their distances are equal
  bit for bit in either form, the index decides)."""
  x = torch.stack([t.double() for t in stack]).cpu()
  n = x.shape[0]
  sq = torch.cdist(x, x).pow(2)
  worst = math.inf
  for i in range(n):
    others = sorted((float(sq[i, j]), j) for j in range(n) if j != i)
    (d_in, j_in), (d_out, j_out) = others[n - f - 2], others[n - f - 1]
    if j_in >= h and j_out >= h:
      continue
    worst = min(worst, (d_out - d_in) / d_out)
  return worst


def run_and_check(step, spy, rule, pre, form, n, f, steps=3, seed=0):
  start = None
  for it in range(steps):
    defense = step.run(honest_rows(it, n - f, seed=seed))
    byz = step.last_byzantine
    assert len(spy.stack) == n and all(t is byz for t in spy.stack[n - f:])
    if pre == "bucketing":
      assert step.last_masks.is_cuda and torch.equal(step.last_masks.cpu(), host_masks(rule, n, f, it)), it
    want = expected_defense(rule, pre, form, spy.stack, step.last_masks, start, n, f)
    print(rule, pre, form, it, "max |defense - expected| =", float((defense - want).abs().max()))
    assert same_bits(defense, want), it
    assert bool(torch.isfinite(defense).all())
    if rule == "cclip":
      start = defense
    floats = step.floats()
    d64 = defense.double()
    # (2e-6 of float64: the bar tests/test_step_cpu.py holds every float of the study row to)
    assert abs(floats["defense_norm_avg"] - math.sqrt(float(torch.dot(d64, d64)))) <= 2e-6 * floats["defense_norm_avg"]
    assert abs(floats["defense_norm_max"] - float(defense.abs().max())) <= 2e-6 * floats["defense_norm_max"]
    assert math.isnan(floats["accept_ratio"])


CASES_11 = [(combo, PLACEMENTS[(i + j) % 3], list(ATTACKS)[(i + 2 * j) % 4]) for i, combo in enumerate(COMBOS) for j in range(3)]


@pytest.mark.parametrize("combo,placement,attack", CASES_11, ids=lambda v: str(v))
def test_defense_is_the_pre_aggregated_rule_on_the_steps_stack(combo, placement, attack):
  rule, pre, form = combo
  n, f = 11, 2
  step = make_step(rule, pre, form, placement, attack, n, f)
  from byzantinemomentum_amd.sharded import HipBackend
  assert isinstance(step.ops, HipBackend) and step.plan.pre == pre and not step.single_call
  run_and_check(step, Spy(step), rule, pre, form, n, f)


@pytest.mark.parametrize("rule,pre,form,placement,attack", [
  ("trmean", "nnm", "rows", "worker", "empire"), ("trmean", "bucketing", "rows", "update", "little-search"),
  ("median", "bucketing", "rows", "server", "minmax"), ("krum", "nnm", "scalars", "worker", "empire"),
  ("krum", "bucketing", "scalars", "update", "anticge"), ("bulyan", "nnm", "rows", "worker", "empire"),
  ("geomed", "nnm", "scalars", "update", "empire"), ("cclip", "bucketing", "scalars", "worker", "empire")])
def test_twenty_five_workers(rule, pre, form, placement, attack):
  n, f = 25, 5
  step = make_step(rule, pre, form, placement, attack, n, f)
  run_and_check(step, Spy(step), rule, pre, form, n, f)


# ---------------------------------------------------------------------------- #
# The "sqdist" plan: the distance matrix of the first pass goes in as local_sq

SQDIST = [("trmean", "nnm", "rows"), ("krum", "nnm", "rows"), ("krum", "nnm", "scalars"), ("geomed", "nnm", "scalars"),
          ("krum", "bucketing", "scalars"), ("cclip", "bucketing", "scalars"), ("median", "nnm", "rows")]


def against_the_plain_partner(rule, pre, form, placement, n, f, d, steps=3, seed=0, fused_kernel=False):
  """fused_kernel: the first pass's own Gram kernel must have made the matrix that went in as local_sq — it then differs
  from the stand-alone pass over the same stack in some bits, and by no more than that pass's bound (1e-5)."""
  from byzantinemomentum_amd import gars
  fused = make_step(rule, pre, form, placement, "empire", n, f)
  plain = make_step(rule, pre, form, placement, "empire", n, f, backend=no_fused_distances())
  assert fused.plan.first_pass == "sqdist" and plain.plan.first_pass == "plain"
  spy = Spy(fused)
  handed = []
  inner = fused._aggregate
  fused._aggregate = lambda gradients, local_sq=None: (handed.append(None if local_sq is None else local_sq.clone()),
                                                       inner(gradients, local_sq))[1]
  for it in range(steps):
    rows = honest_rows(it, n - f, d=d, seed=seed)
    handed.clear()
    got = fused.run([r.clone() for r in rows])
    assert len(handed) == 1 and handed[0] is not None and tuple(handed[0].shape) == (n, n)   # the matrix went in
    alone = gars.pairwise_sqdist(spy.stack)
    apart = float(((handed[0] - alone).abs() / alone.clamp_min(1e-300)).max())
    print(rule, pre, form, placement, it, "fused matrix against the stand-alone pass: worst relative difference", apart)
    if fused_kernel:
      assert not torch.equal(handed[0], alone), "the fused first pass was not reached: the stand-alone pass made the matrix"
      assert apart <= 1e-5, apart
    else:
      assert torch.equal(handed[0], alone)   # below the burst length the first pass IS the stand-alone pass
    # first the margin of this very stack: the two forms may differ by the rounding of the distances alone
    margin = neighbour_margin(spy.stack, n - f, f)
    print(rule, pre, form, placement, it, "neighbour margin", margin)
    assert margin >= MIN_MARGIN, margin
    want = plain.run([r.clone() for r in rows])
    if pre == "nnm":
      assert torch.equal(fused.agg.last_masks, plain.agg.last_masks), it
    else:
      assert torch.equal(fused.last_masks, plain.last_masks), it
    print("max |fused - plain| =", float((got - want).abs().max()))
    assert same_bits(got, want), it


@pytest.mark.parametrize("placement", ["worker", "update"])
@pytest.mark.parametrize("rule,pre,form", SQDIST, ids=lambda v: str(v))
@pytest.mark.parametrize("n,f", [(11, 2), (25, 5)])
def test_sqdist_plan_equals_the_plain_partner(rule, pre, form, placement, n, f):
  """At d = 4099 neither *_sqdist entry point is burst-ready: the matrix the first pass hands in is made by the very
  kernels of the stand-alone pass (asserted: the same bits), so this test checks the PLUMBING of local_sq — that the
  matrix goes in, once, and that everything behind it is unchanged — not robustness to the fused kernel's rounding; the
  margin assertion cannot bite here.  Behind the fused kernel (a longer d, h = 20 or 14) bit-equality would NOT hold for
  the rules whose output depends on the distances continuously (geomed, cclip, the scalars forms): only the test below,
  on rules that read the matrix through the neighbour masks alone, runs there.  Do not raise d here."""
  against_the_plain_partner(rule, pre, form, placement, n, f, D)


@pytest.mark.parametrize("placement", ["worker", "update"])
@pytest.mark.parametrize("rule,form", [("trmean", "rows"), ("krum", "rows")])
def test_fused_first_pass_at_twenty_honest_rows(rule, form, placement):
  """h = 20, f = 5 and a gradient long enough for the burst form under BM_STEP_BURST = 1, at the lengths of the
  knob_burst_sqdist group of tests/first_pass_matrix.py: the ragged length for bm_stack_stats_sqdist (update placement),
  which fuses at d % 4 == 0 only, and three columns more for bm_momentum_stats_sqdist (worker placement: its tail
  launches run too).  The mirror says the call is fused, and the matrix handed to nnm is held NOT to be the stand-alone
  pass's: the distances come out of the first pass's own kernel, with its rounding.  Behind equal neighbour masks — the
  margin is asserted — every bit of nnm in front of a rule on written rows is the same."""
  import os
  from byzantinemomentum_amd import _lib
  from tests import first_pass_matrix as F
  lib = _lib.load()
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  ragged = cus * 4 * F.K_STEP_BURST_BLOCK + 2048 * 3 + 256 + 132
  d = ragged if placement == "update" else ragged + 3
  h, nb = 20, 5
  knobs = dict(F.DEFAULT_KNOBS, BM_STEP_BURST=1)
  assert F.burst_ready(d // 4, cus, knobs) and d <= F.K_MAX_COLS_PER_LAUNCH
  assert (F.nomom_shape(h, nb) and d % 4 == 0) if placement == "update" else F.sqdist_shape(h, h, nb)
  before = int(os.environ.get("BM_STEP_BURST") or F.DEFAULT_KNOBS["BM_STEP_BURST"])   # what the library read at its start
  assert lib.bm_tuning_set(b"BM_STEP_BURST", 1) == 0
  try:
    against_the_plain_partner(rule, "nnm", form, placement, h + nb, nb, d, steps=2, fused_kernel=True)
  finally:
    assert lib.bm_tuning_set(b"BM_STEP_BURST", before) == 0


# ---------------------------------------------------------------------------- #
# A graphed bucketing step

def test_graphed_bucketing_step_draws_new_masks_at_every_replay():
  from byzantinemomentum_amd.graphs import GraphedCall
  from byzantinemomentum_amd.step import AggregationStep
  n, f, warmup = 11, 2, 2

  def new_step():
    return AggregationStep(n, f, f, gar="trmean", momentum=0.9, dampening=0.9, momentum_at="worker", nb_past=0,
                           aggregator=aggregator(), pre="bucketing", pre_args=dict(s=2, seed=SEED))

  rows = honest_rows(0, n - f)
  graphed, eager = new_step(), new_step()
  call = GraphedCall(lambda: graphed.run(rows), warmup=warmup)
  torch.cuda.synchronize()
  eager_out = []
  for it in range(warmup + 3):
    out = eager.run(rows)
    eager_out.append((out.clone(), eager.last_masks.clone()))
  seen = []
  for it in range(3):
    out = call()
    torch.cuda.synchronize()
    seen.append(graphed.last_masks.cpu().clone())
    want_out, want_masks = eager_out[warmup + it]
    assert torch.equal(graphed.last_masks, want_masks), it
    assert torch.equal(graphed.last_masks.cpu(), host_masks("trmean", n, f, warmup + it)), it
    assert same_bits(out, want_out), it
  assert len({tuple(m.tolist()) for m in seen}) == 3
