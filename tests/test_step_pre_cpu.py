"""AggregationStep with a pre-aggregation (pre="nnm" / "bucketing") on the oracle backend, no GPU: the defense of every
step against ShardedAggregator.nnm / .bucketing called on the very stack the step aggregated, bit for bit; the study row
from that defense; the masks of consecutive steps; the plan table; the constructor's refusals; two gloo ranks against
one."""

import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

N, F, D = 11, 2, 96
S, SEED = 2, 7
RULES = {"median": {}, "trmean": {}, "krum": {}, "bulyan": {}, "average": {}, "geomed": dict(nu=1e-4, iters=3),
         "cclip": dict(tau=2.0, iters=2)}
SCALAR = ("krum", "average", "geomed", "cclip")
# (rule, pre, form): the form where it exists.  bulyan behind bucketing needs n_out >= 4 f + 3 = 11 means: s = 1 only
COMBOS = [(rule, pre, form) for rule in RULES for pre in ("nnm", "bucketing")
          for form in (("rows", "scalars") if rule in SCALAR else ("rows",))]
ATTACKS = {"empire": dict(attack="empire", attack_factor=1.1), "empire-search": dict(attack="empire", attack_evals=4),
           "anticge": dict(attack="anticge"), "minmax": dict(attack="minmax")}
PLACEMENTS = ("worker", "server", "update")


def bucket_size(rule, pre):
  return 1 if rule == "bulyan" else S


def pre_args_of(rule, pre, form):
  args = {"form": form}
  if pre == "bucketing":
    args.update(s=bucket_size(rule, pre), seed=SEED)
  return args


def aggregator(**kwargs):
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from tests.sharded_backend import OracleBackend
  return ShardedAggregator(backend=OracleBackend(), **kwargs)


def make_step(rule, pre, form, placement, attack, agg=None, clip=None):
  from byzantinemomentum_amd.step import AggregationStep
  return AggregationStep(N, F, F, gar=rule, gar_args=RULES[rule], momentum=0.9, dampening=0.9, momentum_at=placement,
                         nb_past=2, gradient_clip=clip, aggregator=agg or aggregator(), pre=pre,
                         pre_args=pre_args_of(rule, pre, form), **ATTACKS[attack])


def sampled_for_step(it, h, d=D):
  gen = torch.Generator().manual_seed(2000 + it)
  base = 0.2 * torch.randn(d, generator=gen)
  return [base + (0.5 + 0.1 * i) * torch.randn(d, generator=gen) for i in range(h)]


def expected_masks(rule, pre, counter, seed=SEED):
  from byzantinemomentum_amd.torch_legs import _bucket_masks_torch
  return _bucket_masks_torch(N, bucket_size(rule, pre), seed, counter, torch.zeros(1))


class Spy:
  """Wraps step._defense and step._aggregate: keeps the stack the defense ran on and the masks every aggregation of the
  step read."""

  def __init__(self, step):
    self.step, self.stack, self.first, self.masks_read = step, None, None, []
    inner_defense, inner_aggregate = step._defense, step._aggregate

    def defense(first, attacks):
      self.first, self.stack = first, list(first.honests) + list(attacks)
      return inner_defense(first, attacks)

    def aggregate(gradients, local_sq=None):
      self.masks_read.append(step.last_masks)
      return inner_aggregate(gradients, local_sq)

    step._defense, step._aggregate = defense, aggregate


def expected_defense(rule, pre, form, stack, masks, start):
  agg = aggregator()
  args = dict(RULES[rule])
  if rule == "cclip":
    args["start"] = start
  if pre == "nnm":
    return agg.nnm(stack, F, rule=rule, form=form, **args)
  from byzantinemomentum_amd.pipelines import NNM_RULES
  if NNM_RULES[rule]:
    args["f"] = F
  return agg.bucketing(stack, bucket_size(rule, pre), rule, masks=masks, form=form, **args)


def check_study_row(floats, spy, defense, byz):
  """The fields of the study row that read the defense, from the defense in float64."""
  d64, s64, h64, b64 = (t.double() for t in (defense, spy.first.s_avg, spy.first.h_avg, byz))

  def close(got, want):
    assert abs(got - want) <= 1e-12 * max(abs(want), 1e-30), (got, want)

  def cos(a, b):
    return float(torch.dot(a, b)) / math.sqrt(float(torch.dot(a, a))) / math.sqrt(float(torch.dot(b, b)))

  close(floats["defense_norm_avg"], math.sqrt(float(torch.dot(d64, d64))))
  close(floats["defense_norm_max"], float(defense.abs().max()))
  close(floats["cosin_spldef"], cos(s64, d64))
  close(floats["cosin_hondef"], cos(h64, d64))
  close(floats["cosin_attdef"], cos(b64, d64))
  assert math.isnan(floats["accept_ratio"])


@pytest.mark.parametrize("attack", list(ATTACKS))
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("rule,pre,form", COMBOS, ids=lambda v: str(v))
def test_defense_is_the_pre_aggregated_rule_on_the_steps_stack(rule, pre, form, placement, attack):
  assert not dist.is_initialized()
  step = make_step(rule, pre, form, placement, attack)
  spy = Spy(step)
  assert step.plan.pre == pre and not step.single_call
  start = None
  for it in range(3):
    spy.masks_read.clear()
    defense = step.run([g.clone() for g in sampled_for_step(it, N - F)])
    byz = step.last_byzantine
    assert len(spy.stack) == N and all(t is byz for t in spy.stack[N - F:])
    if pre == "bucketing":
      # one set of masks per run(), those of counter `it`; every evaluation of a search and the defense read them
      assert torch.equal(step.last_masks, expected_masks(rule, pre, it)), it
      assert len(spy.masks_read) == (5 if attack == "empire-search" else 1)
      assert all(m is step.last_masks for m in spy.masks_read)
    else:
      assert step.last_masks is None
    want = expected_defense(rule, pre, form, spy.stack, step.last_masks, start)
    assert torch.equal(defense, want), (it, float((defense - want).abs().max()))
    assert torch.isfinite(defense).all()
    check_study_row(step.floats(), spy, defense, byz)
    if rule == "cclip":
      assert step.cclip_start is defense
      start = defense


def test_the_pre_aggregation_changes_the_defense():
  """The comparison above is not vacuous: with and without `pre` the same inputs give different vectors."""
  for pre in ("nnm", "bucketing"):
    with_pre, without = make_step("trmean", pre, "rows", "worker", "empire"), None
    from byzantinemomentum_amd.step import AggregationStep
    without = AggregationStep(N, F, F, gar="trmean", momentum=0.9, dampening=0.9, nb_past=2, aggregator=aggregator())
    a = with_pre.run([g.clone() for g in sampled_for_step(0, N - F)])
    b = without.run([g.clone() for g in sampled_for_step(0, N - F)])
    assert not torch.equal(a, b)


def test_clipping_goes_with_a_pre_aggregation():
  step = make_step("krum", "bucketing", "scalars", "worker", "empire", clip=4.0)
  spy = Spy(step)
  for it in range(2):
    defense = step.run([g.clone() for g in sampled_for_step(it, N - F)])
    assert torch.equal(defense, expected_defense("krum", "bucketing", "scalars", spy.stack, step.last_masks, None))


def test_seed_and_counter_of_the_masks():
  a = make_step("median", "bucketing", "rows", "worker", "empire")
  from byzantinemomentum_amd.step import AggregationStep
  b = AggregationStep(N, F, F, gar="average", aggregator=aggregator(), pre="bucketing", pre_args=dict(s=3))  # seed 0
  for it in range(3):
    a.run(sampled_for_step(it, N - F))
    b.run(sampled_for_step(it, N - F))
    assert torch.equal(a.last_masks, expected_masks("median", "bucketing", it))
    from byzantinemomentum_amd.torch_legs import _bucket_masks_torch
    assert torch.equal(b.last_masks, _bucket_masks_torch(N, 3, 0, it, torch.zeros(1)))
    assert int((b.last_masks != 0).sum()) == 4


# ---------------------------------------------------------------------------- #
# The plan table

class _Caps:  # the plan reads the capabilities alone: the HIP backend's, without a GPU
  device_search_rules = ("krum", "average")

  def __init__(self, drop=()):
    from byzantinemomentum_amd.sharded import HipBackend
    self.capabilities = HipBackend.capabilities - frozenset(drop)


def _plan(rule, pre, form, placement, attack, backend, f_real=F, **more):
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from byzantinemomentum_amd.step import AggregationStep
  agg = ShardedAggregator(backend=backend) if backend is not None else aggregator()
  step = AggregationStep(N, F, f_real, gar=rule, gar_args=RULES[rule], momentum_at=placement, aggregator=agg,
                         single_call=True, pre=pre, pre_args=pre_args_of(rule, pre, form), **ATTACKS[attack], **more)
  return step.plan


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("rule,pre,form", COMBOS, ids=lambda v: str(v))
def test_plan_table(rule, pre, form, placement):
  from_sq = pre == "nnm" or (form == "scalars" and rule != "average")
  rides = from_sq and placement in ("worker", "update")
  for attack, evals in (("empire", False), ("empire-search", True), ("anticge", False), ("minmax", False)):
    plan = _plan(rule, pre, form, placement, attack, _Caps())
    want = "direction" if evals else ("sqdist" if rides and attack == "empire" else "plain")
    assert plan.first_pass == want, (attack, plan.first_pass, want)
    assert plan.search == ("generic" if evals else None)
    assert plan.device_cursor == (evals and rule != "brute")
    assert plan.single_call is False and plan.accept is None and plan.pre == pre
    # a backend without the fused distance legs, and one without any capability: the plain first pass
    for backend in (_Caps(drop=("momentum_stats_sqdist", "stack_stats_sqdist")), None):
      plan = _plan(rule, pre, form, placement, attack, backend)
      assert plan.first_pass == ("direction" if evals else "plain")
      assert plan.search == ("generic" if evals else None) and not plan.single_call and plan.accept is None
  # nobody to attack: no distance pass rides along
  assert _plan(rule, pre, form, placement, "empire", _Caps(), f_real=0).first_pass == "plain"
  # the host's cursor where it was asked for
  for mode in ("host", "generic"):
    plan = _plan(rule, pre, form, placement, "empire-search", _Caps(), line_search=mode)
    assert plan.search == "generic" and not plan.device_cursor


def test_plan_without_pre_is_what_it_was():
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from byzantinemomentum_amd.step import AggregationStep, StepPlan
  step = AggregationStep(N, F, F, gar="krum", aggregator=ShardedAggregator(backend=_Caps()))
  assert step.plan.pre is None and step.plan.first_pass == "sqdist" and step.plan.accept == "count"
  assert step.pre is None and step.last_masks is None
  assert StepPlan._field_defaults["pre"] is None
  StepPlan(True, True, "plain", None, False, False, frozenset())  # every existing construction still works


# ---------------------------------------------------------------------------- #
# Refusals, in the constructor

@pytest.mark.parametrize("kwargs", [
  dict(pre="mixing"),                                                  # an unknown pre
  dict(pre="nnm", pre_args=dict(form="columns")),                      # an unknown form
  dict(pre="nnm", gar="median", pre_args=dict(form="scalars")),        # a form the rule does not serve
  dict(pre="bucketing", gar="bulyan", pre_args=dict(s=1, form="scalars")),
  dict(pre="nnm", pre_args=dict(s=2)),                                 # foreign keys
  dict(pre="bucketing", pre_args=dict(s=2, perm=[0])),
  dict(pre="bucketing", pre_args=[("s", 2)]),
  dict(pre_args=dict(form="rows")),                                    # pre_args without pre
  dict(pre_args={}),
  dict(pre="bucketing"),                                               # s is required ...
  dict(pre="bucketing", pre_args=dict(seed=3)),
  dict(pre="bucketing", pre_args=dict(s=0)),                           # ... within 1..n ...
  dict(pre="bucketing", pre_args=dict(s=N + 1)),
  dict(pre="bucketing", pre_args=dict(s=2.0)),                         # ... an integer
  dict(pre="bucketing", pre_args=dict(s=True)),
  dict(pre="bucketing", pre_args=dict(s=2, seed="x")),
  dict(pre="bucketing", gar="median", pre_args=dict(s=3)),             # 4 means < 2 f + 1 = 5
  dict(pre="bucketing", gar="trmean", pre_args=dict(s=3)),
  dict(pre="bucketing", gar="phocas", pre_args=dict(s=4)),
  dict(pre="bucketing", gar="meamed", pre_args=dict(s=N)),
])
def test_constructor_refusals(kwargs):
  from byzantinemomentum_amd.step import AggregationStep
  kwargs = dict(dict(gar="krum"), **kwargs)
  with pytest.raises(ValueError):
    AggregationStep(N, F, F, aggregator=aggregator(), **kwargs)


def test_constructor_accepts_the_edges():
  from byzantinemomentum_amd.step import AggregationStep
  for kwargs in (dict(pre="nnm"), dict(pre="nnm", pre_args={}), dict(pre="nnm", pre_args=dict(form="scalars")),
                 dict(pre="bucketing", pre_args=dict(s=1)), dict(pre="bucketing", pre_args=dict(s=N)),
                 dict(pre="bucketing", gar="median", pre_args=dict(s=2)),       # 6 means >= 5
                 dict(pre="bucketing", gar="average", pre_args=dict(s=N, seed=2 ** 64 - 1, form="scalars")),
                 dict(pre="nnm", gar="aksel"), dict(pre="nnm", gar="caf"), dict(pre=None, pre_args=None)):
    AggregationStep(N, F, F, aggregator=aggregator(), **dict(dict(gar="krum"), **kwargs))


# ---------------------------------------------------------------------------- #
# ShardedAggregator.bucketing and nnm(local_sq=) themselves

def test_sharded_bucketing_on_one_rank():
  from byzantinemomentum_amd.torch_legs import _mix_rows_torch
  rows = sampled_for_step(0, N)
  agg = aggregator(local_only=True)
  for s in (1, 2, 3, N):
    n_out = -(-N // s)
    out = agg.bucketing(rows, s, "average", seed=5, counter=9)
    from byzantinemomentum_amd.torch_legs import _bucket_masks_torch
    masks = _bucket_masks_torch(N, s, 5, 9, rows[0])
    assert torch.equal(agg.last_masks, masks)
    means = _mix_rows_torch(rows, masks, n_out)
    assert torch.equal(out, agg.average(means))
    assert torch.equal(agg.bucketing(rows, s, "average", masks=masks), out)
    if n_out >= 2 * F + 1:
      assert torch.equal(agg.bucketing(rows, s, "trmean", masks=masks, f=F), agg.trmean(means, F))
      assert torch.equal(agg.bucketing(rows, s, "median", masks=masks), agg.median(means))
    if n_out >= F + 3:
      assert torch.equal(agg.bucketing(rows, s, "krum", masks=masks, f=F), agg.krum(means, F))
      got = agg.bucketing(rows, s, "krum", masks=masks, f=F, form="scalars")
      assert float((got - agg.krum(means, F)).abs().max()) <= 1e-5
  with pytest.raises(ValueError):
    agg.bucketing(rows, 2, "krum", f=F)                     # neither counter nor masks
  with pytest.raises(ValueError):
    agg.bucketing(rows, 0, "krum", counter=0, f=F)
  with pytest.raises(ValueError):
    agg.bucketing(rows, 2, "median", counter=0, form="scalars")
  with pytest.raises(TypeError):
    agg.bucketing(rows, 2, "krum", counter=0)               # krum needs its f
  with pytest.raises(ValueError):
    agg.bucketing(rows, 2, "median", masks=torch.zeros(3, dtype=torch.int64))


def test_nnm_takes_the_local_distances():
  """local_sq stands in for the distance pass, in both forms: same output, no pass run, the matrix reduced in place."""
  rows = sampled_for_step(1, N)
  for form, rule in (("rows", "trmean"), ("rows", "krum"), ("scalars", "krum"), ("scalars", "geomed")):
    agg = aggregator(local_only=True)
    want = agg.nnm(rows, F, rule=rule, form=form)
    passes = len(agg.backend.totals_seen)
    sq = agg.backend.pairwise_sqdist(rows)
    agg.backend.totals_seen.clear()
    got = agg.nnm(rows, F, rule=rule, form=form, local_sq=sq)
    assert torch.equal(got, want), (form, rule)
    # the pass over the n rows is gone (a distance-based rule on written rows still runs its own on the mixed rows)
    assert len(agg.backend.totals_seen) == passes - 1


# ---------------------------------------------------------------------------- #
# Two gloo ranks against one

SHARDED = [("trmean", "nnm", "rows", "worker", "empire"), ("median", "bucketing", "rows", "update", "empire"),
           ("krum", "nnm", "scalars", "server", "empire"), ("krum", "bucketing", "rows", "worker", "anticge"),
           ("geomed", "bucketing", "scalars", "worker", "minmax"), ("cclip", "nnm", "rows", "update", "empire"),
           ("average", "bucketing", "scalars", "server", "empire"), ("bulyan", "nnm", "rows", "worker", "empire-search")]


def _free_port():
  with socket.socket() as s:
    s.bind(("127.0.0.1", 0))
    return s.getsockname()[1]


def _worker(rank, world, port, d, queue):
  os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
  dist.init_process_group("gloo", rank=rank, world_size=world)
  try:
    from byzantinemomentum_amd.sharded import shard_bounds
    lo, hi = shard_bounds(d, world, rank)
    out = {}
    for ci, cfg in enumerate(SHARDED):
      agg = aggregator()
      assert agg.world_size == world and agg.collective
      step = make_step(*cfg, agg=agg)
      for it in range(3):
        defense = step.run([g[lo:hi].clone() for g in sampled_for_step(it, N - F, d)])
        masks = None if step.last_masks is None else step.last_masks.numpy().copy()
        out[(ci, it)] = (agg.all_gather_output(defense, d).numpy().copy(), step.floats(), masks)
    queue.put((rank, out))
    dist.barrier()
  finally:
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world,d", [(2, 192), (2, 100)])
def test_sharded_step_with_pre_matches_single_rank(world, d):
  """d = 100: the second rank's shard is short (36 coordinates).  Every rank draws the same masks with no collective."""
  ctx = mp.get_context("spawn")
  queue = ctx.Queue()
  port = _free_port()
  procs = [ctx.Process(target=_worker, args=(r, world, port, d, queue)) for r in range(world)]
  for p in procs:
    p.start()
  results = dict(queue.get(timeout=500) for _ in range(world))
  for p in procs:
    p.join(timeout=60)
    assert p.exitcode == 0
  for ci, cfg in enumerate(SHARDED):
    single = make_step(*cfg)
    for it in range(3):
      want_def = single.run([g.clone() for g in sampled_for_step(it, N - F, d)])
      want = single.floats()
      for r in range(world):
        got_def, got, masks = results[r][(ci, it)]
        assert float((torch.from_numpy(got_def) - want_def).abs().max()) <= 1e-6, (cfg, it, r)
        if single.last_masks is None:
          assert masks is None
        else:
          assert torch.equal(torch.from_numpy(masks), single.last_masks), (cfg, it, r)
        for key, val in want.items():
          g = got[key]
          assert (math.isnan(g) and math.isnan(val)) or abs(g - val) <= 1e-9 * max(abs(val), 1e-6), (cfg, it, key, g, val)
      a = results[0][(ci, it)][1]
      for r in range(1, world):
        b = results[r][(ci, it)][1]
        assert all(a[k] == b[k] or (math.isnan(a[k]) and math.isnan(b[k])) for k in a)
