"""tests/graph_matrix.py on the CPU: the case lists reach what they claim (every pair, every value of the secondary
arguments with every rule, attack and placement, every plan of the universe at nb_past = 0, the universe partitioned
into "matrix case" and "refused"), the eager twin the GPU test trusts is itself held against the float64 loop
(step_matrix.MatrixLoop at nb_past = 0, the step matrix's own bars) on tests/sharded_backend.OracleBackend, and the
host-side contracts of a graphed step: the refusals, the caches that follow a replay, the state kept at fixed addresses,
the study row of a zero vector.  No GPU."""

import itertools
import math

import pytest
import torch

from tests import graph_matrix as GM
from tests import step_matrix as SM
from tests.attack_vectors_reference import assert_floats_close_nan
from tests.test_step_matrix_cpu import _hip_like, _plan_key

# ---------------------------------------------------------------------------------------------------------------------
# The case lists


def _group(name):
  return [c for c in GM.cases() if c.group == name]


def test_the_lists_are_what_the_module_says():
  product = _group("product")
  keys = [a.key for a in SM.ATTACKS]
  assert {(c.rule, c.attack, c.placement) for c in product} == set(itertools.product(SM.RULES, keys, SM.PLACEMENTS))
  assert len(product) == 14 * 12 * 3
  assert all(c.d == SM.D and c.nb_past == 0 for c in GM.cases())
  searched = _group("searched")
  assert {(c.rule, c.attack) for c in searched} == set(itertools.product([r for r in SM.RULES if r != "brute"],
                                                                         GM.SEARCHED_ATTACKS))
  assert len(searched) == 26 and all(c.evals == GM.EVALS for c in searched)
  assert {c.placement for c in searched} == set(SM.PLACEMENTS)
  for key in GM.SEARCHED_ATTACKS:
    assert {c.placement for c in searched if c.attack == key} == set(SM.PLACEMENTS)
  pre = _group("pre")
  want = {(p, r, pl, f) for p, r, pl in itertools.product(("nnm", "bucketing"), GM.PRE_RULES, SM.PLACEMENTS)
          for f in (("rows", "scalars") if r in GM.SCALAR_RULES else ("rows",))}
  assert {(c.pre, c.rule, c.placement, c.pre_args["form"]) for c in pre} == want and len(pre) == len(want) == 30
  from byzantinemomentum_amd import pipelines
  assert set(GM.SCALAR_RULES) == set(GM.PRE_RULES) & set(pipelines.SCALAR_RULES)
  assert all(c.pre_args["s"] == GM.BUCKET for c in pre if c.pre == "bucketing")
  # the single call both ways wherever the plan can take it
  plans = _group("plan")
  assert all(SM.can_take_the_single_call(c) for c in plans)
  assert {(c.rule, c.attack, c.f_real, c.single_call) for c in plans} == set(itertools.product(
    SM.DISTANCE + SM.COLWISE, SM.FIRST_PASS_ATTACKS, (2, 0), (True, False))) and len(plans) == 48
  assert len(GM.cases()) == 504 + 48 + 26 + 30


def test_every_pair_and_every_secondary_value_is_reached():
  product = _group("product")
  keys = {a.key for a in SM.ATTACKS}
  axes = {
    "clip": (lambda c: c.clip is not None, (True, False)),
    "ff": (lambda c: (c.n, c.f_decl, c.f_real), SM.FF),
    "l2": (lambda c: c.with_l2, (True, False)),
    "single_call": (lambda c: c.single_call, (True, False)),
    "extra": (lambda c: c.extra, (0, 1)),
  }
  for axis, (of, values) in axes.items():
    for value in values:
      chosen = [c for c in product if of(c) == value]
      assert {c.rule for c in chosen} == set(SM.RULES), (axis, value)
      assert {c.attack for c in chosen} == keys, (axis, value)
      assert {c.placement for c in chosen} == set(SM.PLACEMENTS), (axis, value)
  signed = [a.key for a in SM.ATTACKS if a.negative is not None]
  for value in (True, False):
    chosen = [c for c in product if c.attack in signed and (c.factor < 0) == value]
    assert {c.rule for c in chosen} == set(SM.RULES) and {c.attack for c in chosen} == set(signed)
    assert {c.placement for c in chosen} == set(SM.PLACEMENTS)
  for value in (SM.M_ARG, None):
    chosen = [c for c in product if c.rule in SM.DISTANCE and c.m == value]
    assert {c.rule for c in chosen} == set(SM.DISTANCE) and {c.attack for c in chosen} == keys
    assert {c.placement for c in chosen} == set(SM.PLACEMENTS)
  assert any(c.f_real == 0 for c in product)


# ---------------------------------------------------------------------------------------------------------------------
# Plans, and the partition of the universe into "matrix case" and "refused"


def _step(kwargs, backend=None):
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from byzantinemomentum_amd.step import AggregationStep
  from tests.sharded_backend import OracleBackend
  backend = backend or OracleBackend
  return AggregationStep(aggregator=ShardedAggregator(backend=backend(), local_only=True), **kwargs)


def _universe():
  """Every configuration of the universe as constructor arguments: the fixed-factor product with every secondary value,
  the searches of empire and little against EVERY rule with every line_search, the pre-aggregations — each at nb_past 0
  and at the step matrix's nb_past."""
  base = dict(SM.constructor_kwargs(SM.cases()[0]))
  for nb_past in (0, SM.NB_PAST):
    for rule, att, placement, ff, single, m, negative in itertools.product(
        SM.RULES, SM.ATTACKS, SM.PLACEMENTS, SM.FF, (True, False), (None, SM.M_ARG), (False, True)):
      if m is not None and rule not in SM.DISTANCE:
        continue
      factor = att.negative if negative and att.negative is not None else att.factor
      case = GM.Case("u", rule, att.key, placement, *ff, None, m, False, single, factor, SM.D, 0, "universe", nb_past, 0,
                     None, None, None)
      yield dict(SM.constructor_kwargs(case), line_search="auto")
    for rule, key, placement, line_search in itertools.product(SM.RULES, GM.SEARCHED_ATTACKS, SM.PLACEMENTS,
                                                               ("auto", "host", "generic")):
      case = GM.Case("u", rule, key, placement, *SM.FF[0], None, None, False, False, 1.1, SM.D, 0, "universe", nb_past, 0,
                     GM.EVALS, None, None)
      yield dict(SM.constructor_kwargs(case), attack_evals=GM.EVALS, line_search=line_search)
    for case in _group("pre"):
      yield dict(GM.constructor_kwargs(case), nb_past=nb_past)
  assert base["nb_past"] == SM.NB_PAST


def test_the_universe_is_matrix_case_or_refused():
  """With the HIP backend's capability set: a configuration the step does not refuse has a plan that a matrix case
  runs, with the same line_search; one it refuses is refused for a past, or for a cursor on the host — and exactly
  those are.  Nothing is in neither."""
  hip_like = _hip_like()
  reached = set()
  for case in GM.cases():
    step = _step(GM.constructor_kwargs(case), hip_like)
    assert step.graph_refusal() is None, (case.name, step.graph_refusal())
    reached.add(_plan_key(step.plan))
  accepted, refused = set(), 0
  for kwargs in _universe():
    step = _step(kwargs, hip_like)
    reason, plan = step.graph_refusal(), step.plan
    host_cursor = plan.searches and not plan.device_cursor
    assert (reason is not None) == (kwargs["nb_past"] > 0 or host_cursor), (kwargs, reason)
    if reason is None:
      assert kwargs["line_search"] == "auto" and kwargs["gar"] != "brute" or not plan.searches
      accepted.add(_plan_key(plan))
    else:
      refused += 1
  assert accepted == reached, (len(accepted), len(reached), sorted(accepted - reached)[:3], sorted(reached - accepted)[:3])
  assert refused > 0


def test_searched_cases_keep_the_cursor_on_the_device():
  hip_like = _hip_like()
  for case in _group("searched"):
    plan = _step(GM.constructor_kwargs(case), hip_like).plan
    assert plan.searches and plan.device_cursor and plan.search is not None, case.name
  assert {_step(GM.constructor_kwargs(c), hip_like).plan.search for c in _group("searched")} == {
    "scalar_device", "bulyan", "median", "colwise_eval", "generic"}


# ---------------------------------------------------------------------------------------------------------------------
# The eager twin against the float64 loop

NNM_MARGIN = 1e-4   # relative gap between the last neighbour taken and the first one left out


class PreLoop(SM.MatrixLoop):
  """MatrixLoop with the pre-aggregation of a "pre" case in front of the rule, in float64: nnm — every row replaced by
  the mean of itself and its n - f - 1 nearest, ties to the lower index —, bucketing — the means of the buckets drawn
  with the step's own counter (0, 1, 2 ... by step; the project's masks: test_bucket_masks_cpu.py pins them)."""

  def __init__(self, case):
    super().__init__(case)
    self.counter = 0

  def aggregate(self, grads, f, observed=None):
    case, n = self.case, len(grads)
    margins = {}
    if case.pre == "nnm":
      mixed, worst = [], math.inf
      for i in range(n):
        others = [j for j in range(n) if j != i]
        dist = {j: float((grads[i] - grads[j]).pow(2).sum()) for j in others}
        order = sorted(others, key=lambda j: dist[j])
        keep = n - f - 1
        if grads[order[keep - 1]] is not grads[order[keep]]:
          worst = min(worst, SM._gap(dist[order[keep - 1]], dist[order[keep]]))
        mixed.append(SM._mean64([grads[i]] + [grads[j] for j in order[:keep]]))
      margins["nnm"] = worst
    else:
      from byzantinemomentum_amd.torch_legs import _bucket_masks_torch, _mask_words
      s = case.pre_args["s"]
      words = _mask_words(_bucket_masks_torch(n, s, case.pre_args["seed"], self.counter, torch.zeros(1)), -(-n // s))
      self.counter += 1
      mixed = [SM._mean64([grads[j] for j in range(n) if (w >> j) & 1]) for w in words]
    defense, _, rule_margins = super().aggregate(mixed, f, observed)
    margins.update(rule_margins)
    return defense, math.nan, margins


def eager_against_the_loop(case):
  """{(step, quantity): (error, bar)} of what misses its bar: the case's five eager steps on the oracle backend against
  the loop.  A searched case is held at the factor the step found (the search itself: tests/search_matrix.py)."""
  step = _step(GM.constructor_kwargs(case))
  loop = PreLoop(case) if case.pre is not None else SM.MatrixLoop(case)
  in_step = case.rule == "cge" and case.attack == "anticge" and case.f_real > 0
  bad, defenses = {}, []
  for it, (sampled, params, origin) in enumerate(GM.inputs(case)):
    assert len(sampled) == case.n - case.f_real + case.extra
    got = step.run([g.clone() for g in sampled], params, origin)
    defenses.append(dict(defense=got.clone(), floats=dict(step.floats())))
    if case.evals is not None:
      assert isinstance(step.last_factor, float) and len(step.last_search) == case.evals
      loop.case = case._replace(factor=step.last_factor)
    exp = loop.step(sampled, params, origin, observed=got if in_step else None)
    if case.evals is not None and exp.byzantine is not None and bool(torch.isfinite(exp.byzantine).all()):
      # a searched factor may be large: fp32 rounds a vector relative to ITS largest entry, not to the gradients'
      exp = exp._replace(scale=max(exp.scale, float(exp.byzantine.abs().max())))
    under = SM.below_margin(exp.margins)
    if exp.margins.get("nnm", math.inf) < NNM_MARGIN:
      under["nnm"] = exp.margins["nnm"]
    assert not under, (case.name, it, under)
    if case.clip is not None:
      assert any(exp.clipped) and not all(exp.clipped), (case.name, it, exp.clipped)
    assert_floats_close_nan(step.floats(), exp.floats, tag=(case.name, it), tol=SM.FLOATS_TOL)
    assert math.isnan(step.floats()["cosin_sampled"]) and math.isnan(step.floats()["curv_sampled"])  # nb_past = 0
    errs = SM.errors(case, step, got, exp)
    if case.attack == "empire" and case.evals is None:
      # avg + f * (-avg) in fp32 cancels: one rounding of avg's size, 2^-24 (1 + |f|) |avg|, in a vector of size
      # |1 - f| |avg| — 1.25e-6 of it at f = 1.1, whatever the rule; twice that is the bar of its norm and maximum where
      # the rule's own bar for the study row (center_cases.FLOATS_BAR) is tighter
      cancel = 2.0 ** -23 * (1 + abs(case.factor)) / abs(1 - case.factor)
      for key in ("floats.attack_norm_avg", "floats.attack_norm_max"):
        errs[key] = (errs[key][0], max(errs[key][1], cancel))
    bad.update({(it, key): pair for key, pair in SM.failures(errs).items()})
    # Five steps, two more than the bars of the step matrix were measured over: the loop goes on from the state the step
    # carries (compared above, at its bar, at the step where it arises), so that every step is held on its own and the
    # roundings of the momentum do not add up over the sequence
    if step.server_momentum is not None:
      loop.server64 = step.server_momentum.detach().double().clone()
    if step.cclip_start is not None:
      loop.start = step.cclip_start.detach().double().clone()
  for it in range(1, GM.STEPS):  # what graph_matrix.moved asks of the twin on the device
    assert GM.moved(defenses[it - 1], defenses[it]), (case.name, it)
  return bad


@pytest.mark.parametrize("rule,placement", list(itertools.product(SM.RULES, SM.PLACEMENTS)))
def test_the_eager_twin_is_the_float64_loop(rule, placement):
  todo = [c for c in GM.cases() if (c.rule, c.placement) == (rule, placement)]
  assert len(todo) >= len(SM.ATTACKS)
  for case in todo:
    bad = eager_against_the_loop(case)
    assert not bad, (case.name, bad)


# ---------------------------------------------------------------------------------------------------------------------
# Refusals: decided on the host, before anything runs

D_SMALL = 64


def _rows(seed, count, d=D_SMALL):
  gen = torch.Generator().manual_seed(seed)
  return [torch.randn(d, generator=gen) for _ in range(count)]


def _small(**kwargs):
  args = dict(nb_workers=7, nb_decl_byz=2, nb_real_byz=2, gar="median", momentum=0.9, dampening=0.9, nb_past=0)
  args.update(kwargs)
  return _step(args)


REFUSED = {
  "a-past": (dict(nb_past=2), "nb_past"),
  "line-search-host": (dict(attack_evals=4, line_search="host"), "cursor is on the host"),
  "line-search-generic": (dict(attack_evals=4, line_search="generic"), "cursor is on the host"),
  "brute-searched": (dict(gar="brute", attack_evals=4), "cursor is on the host"),
  "empire-strict-on-a-scalar-rule": (dict(gar="krum", attack="empire-strict", attack_evals=4), "cursor is on the host"),
  "bucketing-on-a-host-counter": (dict(pre="bucketing", pre_args=dict(s=1)), "counter"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_a_step_that_cannot_replay_is_refused_under_capture(name, monkeypatch):
  from byzantinemomentum_amd import graphs
  kwargs, word = REFUSED[name]
  step = _small(**kwargs)
  assert word in step.graph_refusal()
  rows = _rows(1, 5)
  before = [g.clone() for g in rows]
  step.run([g.clone() for g in rows])   # eager: runs
  monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
  fresh = _small(**kwargs)
  calls = []
  monkeypatch.setattr(fresh, "_clip_factors", lambda sampled: calls.append("launched"))
  with pytest.raises(graphs.GraphRefusal, match=word):
    fresh.run(rows)
  assert not calls and fresh._pending is None and fresh.buffers is None
  assert all(torch.equal(a, b) for a, b in zip(rows, before))


def test_graphedcall_reports_a_refusal_during_its_warm_up(monkeypatch):
  """GraphedCall holds graphs.preparing() around warm-up and recording: the step refuses at the first warm-up call, before
  it has advanced anything, and the error names the reason.  (No GPU here: the stand-in below is the part of
  GraphedCall.__init__ around `fn`.)"""
  from byzantinemomentum_amd import graphs
  step = _small(nb_past=2)
  monkeypatch.setattr(graphs, "_preparing", 1)
  with pytest.raises(graphs.GraphRefusal, match="nb_past"):
    step.run(_rows(1, 5))
  assert step._pending is None and len(step.pasts) == 0


def test_a_capturable_step_is_not_refused(monkeypatch):
  monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
  for kwargs in (dict(), dict(gar="krum", momentum_at="server"), dict(gar="cclip", gar_args=dict(tau=2.0), momentum_at="update"),
                 dict(pre="nnm")):
    step = _small(**kwargs)
    assert step.graph_refusal() is None
    step.run(_rows(1, 5))
    assert step.floats()["defense_norm_avg"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# The caches follow a replay, and only a replay


class _CountingFetch:
  def __init__(self, step, monkeypatch):
    self.count = 0
    inner_exchange, inner_fetch = step._exchange, step._fetch

    def exchange(pend):
      self.count += 1
      return inner_exchange(pend)

    def fetch(matrix):
      self.count += 1
      return inner_fetch(matrix)

    monkeypatch.setattr(step, "_exchange", exchange)
    monkeypatch.setattr(step, "_fetch", fetch)


def test_floats_follow_a_replay_and_nothing_else(monkeypatch):
  from byzantinemomentum_amd import graphs
  step = _small(gar="krum")
  reads = _CountingFetch(step, monkeypatch)
  step.run(_rows(1, 5))
  first = step.floats()
  assert step.floats() is first and reads.count == 1
  # what a replay does: the recorded kernels rewrite the scalars where they are, no Python of run() runs
  pend = step._pending
  pend.study.mul_(4.0)
  pend.s.mul_(4.0)
  pend.h.mul_(4.0)
  assert step.floats() is first and reads.count == 1   # without the notification: not touched again
  graphs.notify_replay()
  second = step.floats()
  assert reads.count == 2 and second is not first
  assert second["defense_norm_avg"] == 2.0 * first["defense_norm_avg"]
  assert second["sampled_norm_avg"] == 2.0 * first["sampled_norm_avg"]
  assert second["honest_norm_max"] == 4.0 * first["honest_norm_max"]
  assert step.floats() is second and reads.count == 2  # idempotent between replays


def test_last_factor_and_last_search_follow_a_replay_and_nothing_else(monkeypatch):
  """The result of a device search (stats.DeviceSearch.finish, bm_attack_line_search_device): fp64, [0] the factor, then
  (x, objective) per evaluation.  The oracle backend searches on the host, so the tensor is put where run() puts it."""
  from byzantinemomentum_amd import graphs
  step = _small(gar="krum", attack_evals=2, line_search="host")
  reads = _CountingFetch(step, monkeypatch)
  step.run(_rows(1, 5))
  reads.count = 0   # (the host search of run() has read its distances)
  found = torch.tensor([1.5, 1.0, 10.0, 1.5, 20.0], dtype=torch.float64)
  step.last_search = found
  step.last_factor = found
  assert step._factor_now is found and reads.count == 0   # nobody has read it: it stays where it is
  assert step.last_factor == 1.5 and step.last_search == [(1.0, 10.0), (1.5, 20.0)] and reads.count == 1
  found.copy_(torch.tensor([2.5, 2.0, 30.0, 2.5, 40.0], dtype=torch.float64))   # a replay's search
  assert step.last_factor == 1.5 and step.last_search == [(1.0, 10.0), (1.5, 20.0)] and reads.count == 1
  graphs.notify_replay()
  assert step.last_search == [(2.0, 30.0), (2.5, 40.0)] and step.last_factor == 2.5 and reads.count == 2
  assert step.last_factor == 2.5 and reads.count == 2
  # an eager step after that sets a number and a list: they are what the getters return
  step.run(_rows(2, 5))
  reads.count = 0
  assert isinstance(step.last_factor, float) and len(step.last_search) == 2
  graphs.notify_replay()
  assert isinstance(step.last_factor, float) and len(step.last_search) == 2 and reads.count == 0


@pytest.mark.parametrize("gar,placement", [("krum", "server"), ("cclip", "worker"), ("cclip", "server")])
def test_a_graphed_step_keeps_its_state_at_fixed_addresses(gar, placement, monkeypatch):
  """Under graphs.preparing() (what GraphedCall holds around warm-up and recording) the server momentum and cclip's start
  are buffers of the step's own with the defense's bits — the same addresses from the first warm-up on, so a recorded
  kernel reads what the replay before it wrote — and the defense vectors handed out are never written again.  An eager
  step rebinds, as before, and copies nothing."""
  from byzantinemomentum_amd import graphs
  args = dict(gar=gar, gar_args=dict(tau=2.0) if gar == "cclip" else None, momentum_at=placement)
  eager, graphed = _small(**args), _small(**args)
  handed, kept = [], None
  for it in range(4):
    rows = _rows(10 + it, 5)
    monkeypatch.setattr(graphs, "_preparing", 0)
    want = eager.run([g.clone() for g in rows])
    if placement == "server":
      assert eager.server_momentum is want
    if gar == "cclip":
      assert eager.cclip_start is want
    monkeypatch.setattr(graphs, "_preparing", 1 if it < 3 else 0)   # (kept once the step has been warmed up)
    got = graphed.run([g.clone() for g in rows])
    assert torch.equal(got, want), it
    state = [t for t in (graphed.server_momentum if placement == "server" else None,
                         graphed.cclip_start if gar == "cclip" else None) if t is not None]
    assert state and all(t is not got and torch.equal(t, got) for t in state)
    addresses = [t.data_ptr() for t in state]
    assert kept is None or addresses == kept, it
    kept = addresses
    handed.append((got, got.clone()))
    assert all(torch.equal(t, copy) for t, copy in handed)   # no defense handed out earlier was overwritten
  assert not eager._kept


# ---------------------------------------------------------------------------------------------------------------------
# The study row of a vector of norm zero


def test_floats_with_a_zero_vector_divide_like_the_reference():
  """attack.py:854-859 divides tensors: a Byzantine vector or a defense of norm 0 gives NaN cosines, no exception.
  empire at factor 1 is avg + 1 * (-avg) = 0 exactly; honest rows that cancel give a zero average and a zero defense."""
  step = _small(gar="average", attack="empire", attack_factor=1.0, momentum_at="update")
  step.run(_rows(3, 5))
  assert float(step.last_byzantine.abs().max()) == 0.0
  row = step.floats()
  assert row["attack_norm_avg"] == 0.0
  assert all(math.isnan(row[key]) for key in ("cosin_splatt", "cosin_honatt", "cosin_attdef"))
  assert all(math.isfinite(row[key]) for key in ("cosin_splhon", "cosin_spldef", "cosin_hondef"))
  a, b = _rows(4, 2)
  step = _small(nb_workers=4, nb_decl_byz=0, nb_real_byz=0, gar="average", momentum_at="update")
  step.run([a, -a, b, -b])
  row = step.floats()
  assert row["honest_norm_avg"] == 0.0 and row["defense_norm_avg"] == 0.0
  assert all(math.isnan(row[key]) for key in ("cosin_splhon", "cosin_spldef", "cosin_hondef"))
  from byzantinemomentum_amd.step import _ieee_div
  assert _ieee_div(1.0, 0.0) == math.inf and _ieee_div(-1.0, 0.0) == -math.inf and _ieee_div(1.0, -0.0) == -math.inf
  assert math.isnan(_ieee_div(0.0, 0.0)) and math.isnan(_ieee_div(math.nan, 0.0)) and _ieee_div(1.0, 2.0) == 0.5
