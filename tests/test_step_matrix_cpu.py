"""tests/step_matrix.py on the CPU: the float64 loop pinned on the restatements that exist, every case of the matrix
through AggregationStep on tests/sharded_backend.OracleBackend against the loop, the plans the cases reach, pairwise
coverage of the secondary arguments, no decision under its margin, and one built-in host-logic mistake per defect twin
shown to be caught.  No GPU."""

import itertools
import math

import pytest
import torch

from tests import anticge_reference as A
from tests import attack_vectors_reference as R
from tests import step_matrix as SM

# ---------------------------------------------------------------------------------------------------------------------
# Pinning


def _free_case(rule, attack, placement, clip=None, factor=None, d=SM.D, n=11, f=2):
  att = SM.ATTACK[attack]
  return SM.Case("pin", rule, attack, placement, n, f, f, clip, None, True, False, att.factor if factor is None else factor,
                 d, 0, "pin")


def test_gar_args_are_those_of_the_center_step_test():
  from tests.test_gpu_center_step import GAR_ARGS
  assert {rule: SM.GAR_ARGS[rule] for rule in SM.CENTER} == GAR_ARGS
  assert SM.GAR_ARGS["caf"]["power_iters"] == SM.GAR_ARGS["dnc"]["power_iters"] == SM.sc.T_END_TO_END


def test_loop_equals_the_reference_loop_on_its_configurations():
  """oracle/step_oracle.ReferenceLoop (the reference's fp32 operations, float64 floats) on test_step_cpu.CONFIGS, four
  steps, step 2 with a gradient sampled for the study only: the two statements agree within the fp32 roundings of the
  reference's own arithmetic — 2e-6 of max|sampled| for the vectors, 2e-6 for the study row, as test_step_cpu holds the
  step to that loop.  (The loop's clipping factor is the fp32 number of the step, the reference loop's a double.)"""
  from tests import test_step_cpu as T
  from tests.step_reference import assert_floats_close
  for cfg in T.CONFIGS:
    case = _free_case(cfg["gar"], cfg["attack"], cfg["momentum_at"], cfg["clip"], cfg["factor"], d=T.D)
    loop, ref = SM.MatrixLoop(case), T.reference_for(cfg)
    gen = torch.Generator().manual_seed(5)
    origin = torch.randn(T.D, generator=gen)
    params = origin.clone()
    for it in range(4):
      sampled = T.sampled_for_step(it, T.N - T.F, extra=(1 if it == 2 else 0))
      want_def, want_upd, want = ref.step(sampled, params, origin)
      exp = loop.step(sampled, params, origin)
      scale = float(torch.stack(sampled).abs().max())
      assert float((exp.defense - want_def.double()).abs().max()) <= 2e-6 * scale, (cfg, it)
      assert float((exp.update - want_upd.double()).abs().max()) <= 2e-6 * scale, (cfg, it)
      assert_floats_close(exp.floats, want, tag=(T.config_id(cfg), it), tol=2e-6)
      params = params - 0.05 * want_upd


@pytest.mark.parametrize("placement,gar", list(itertools.product(SM.PLACEMENTS, ("cge", "krum", "median"))))
def test_loop_equals_the_anticge_loop_on_its_step_cases(placement, gar):
  """tests/anticge_reference.AnticgeLoop on the step cases of tests/test_anticge_cpu.py (n = 11, f = 2, d = 257)."""
  from tests.step_reference import assert_floats_close
  n, f, d = 11, 2, 257
  loop, ref = SM.MatrixLoop(_free_case(gar, "anticge", placement, d=d)), A.AnticgeLoop(n, f, f, gar, placement)
  for it in range(2):
    sampled = A.sampled_for_step(it, n - f, d)
    _, want = ref.begin(sampled)
    want_def, want_upd, floats = ref.finish(want.vector)
    exp = loop.step(sampled, observed=want_def)
    scale = float(torch.stack(sampled).abs().max())
    assert float((exp.byzantine - want.vector.double()).abs().max()) <= 1e-6 * float(want.vector.abs().max())
    assert float((exp.defense - want_def.double()).abs().max()) <= 2e-6 * scale, it
    assert float((exp.update - want_upd.double()).abs().max()) <= 2e-6 * scale, it
    assert_floats_close(exp.floats, floats, tag=(placement, gar, it), tol=1e-5)


@pytest.mark.parametrize("name", R.FIXED)
def test_vectors_equal_the_restated_attacks_on_their_fixed_cases(name):
  """tests/attack_vectors_reference.restate at precision f32 — bit-identical to the reference's attacks — on the fixed
  fixtures: the float64 vector is that one within an fp32 rounding of it."""
  fx = R.Fixture(name)
  c = fx.case
  step_name = {"nan": "nan", "bulyan": "hidden", "empire-strict": "empire-strict"}[c["attack"]]
  want = R.restate(c["attack"], fx.honests, fx.f, fx.f, arg=c["arg"], negative=c["negative"], target_idx=c["target_idx"],
                   avg=R.seq_mean(fx.honests)).vector
  factor = -c["arg"] if c["negative"] else c["arg"]
  got = SM.byzantine_vector(step_name, fx.honests, factor, {"target_idx": c["target_idx"]}, fx.f, fx.f)[0]
  if c["attack"] == "nan":
    assert bool(got.isnan().all()) and bool(want.isnan().all())
  else:
    assert float((got - want.double()).abs().max()) <= 2.0 ** -23 * float(want.abs().max()), name


def test_second_pass_of_bulyan_in_step_equals_the_oracle():
  """step_matrix.bulyan_pass2_f64, which the long cases run in step with the device, is oracle.gar_oracle.bulyan at
  float64 where no column is within fp32 resolution of a tie, and an observation far from both windows moves nothing."""
  from oracle import gar_oracle as O
  case = {c.name: c for c in SM.cases()}["bulyan-empire-worker-plan-f2-sequence"]
  rows = [g.double() for g in SM.inputs(case)[0][0]]
  grads = rows + [rows[0] * 0.5] * 2
  want = O.bulyan(grads, 2, None, "f64")
  order = O.bulyan_order(grads, 2, None, "f64")[0]
  got, share = SM.bulyan_pass2_f64(grads, order, 2, 7, want)
  assert share == 1.0 and float((got - want).abs().max()) <= 1e-15 * float(want.abs().max())
  n, f = 15, 2
  gen = torch.Generator().manual_seed(3)
  grads = [torch.randn(64, generator=gen, dtype=torch.float64) for _ in range(n)]
  order = O.bulyan_order(grads, f, None, "f64")[0]
  plain, share = SM.bulyan_pass2_f64(grads, order, f, n - f - 2, O.bulyan(grads, f, None, "f64"))
  assert share == 1.0
  far = plain + 100.0   # an observation far from both windows moves nothing
  assert torch.equal(SM.bulyan_pass2_f64(grads, order, f, n - f - 2, far)[0], plain)


# ---------------------------------------------------------------------------------------------------------------------
# The case list


def test_the_universe_is_the_steps_own():
  from byzantinemomentum_amd import step
  assert SM.RULES == step._RULES and SM.COLWISE == step._COLWISE and SM.DISTANCE == step._DISTANCE
  assert {a.name for a in SM.ATTACKS} == set(step._ATTACK) | set(step._ATTACK_BEYOND)
  assert {a.args["perturbation"] for a in SM.ATTACKS if a.name == "minmax"} == set(step._PERTURBATIONS)
  targets = [a.args["target_idx"] for a in SM.ATTACKS if a.name == "hidden"]
  assert targets == [-1, SM.INTERIOR, "all"] and 0 < SM.INTERIOR < SM.D - 4
  assert SM.D % 4 == 3 and SM.D // 4 >= 256  # a tail of 3 behind a 16-byte body that fills a 256-thread workgroup


def test_the_product_is_full_and_nothing_but_the_refusals_is_left_out():
  product = [c for c in SM.cases() if c.group == "product"]
  assert {(c.rule, c.attack, c.placement) for c in product} == set(itertools.product(
    SM.RULES, [a.key for a in SM.ATTACKS], SM.PLACEMENTS)) and len(product) == 14 * 12 * 3
  assert all(c.d == SM.D for c in SM.cases())
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from byzantinemomentum_amd.step import AggregationStep
  from tests.sharded_backend import OracleBackend
  agg = ShardedAggregator(backend=OracleBackend(), local_only=True)
  for refused in SM.REFUSED:
    for rule, placement in itertools.product(SM.RULES, SM.PLACEMENTS):
      with pytest.raises(ValueError):
        AggregationStep(11, 2, 2, gar=rule, gar_args=SM.GAR_ARGS.get(rule), momentum_at=placement, aggregator=agg, **refused)


def test_secondary_arguments_meet_every_rule_attack_and_placement():
  product = [c for c in SM.cases() if c.group == "product"]
  axes = {
    "clip": lambda c: c.clip is not None,
    "ff": lambda c: (c.n, c.f_decl, c.f_real),
    "l2": lambda c: c.with_l2,
    "single_call": lambda c: c.single_call,
  }
  values = {"clip": (True, False), "ff": SM.FF, "l2": (True, False), "single_call": (True, False)}
  for axis, of in axes.items():
    for value in values[axis]:
      with_value = [c for c in product if of(c) == value]
      assert {c.rule for c in with_value} == set(SM.RULES), (axis, value)
      assert {c.attack for c in with_value} == {a.key for a in SM.ATTACKS}, (axis, value)
      assert {c.placement for c in with_value} == set(SM.PLACEMENTS), (axis, value)
  # a negative factor: the attacks that have a factor and a `negative`
  signed = [a.key for a in SM.ATTACKS if a.negative is not None]
  assert {SM.ATTACK[k].name for k in signed} == {"empire", "little", "hidden"}
  for value in (True, False):
    chosen = [c for c in product if c.attack in signed and (c.factor < 0) == value]
    assert {c.rule for c in chosen} == set(SM.RULES) and {c.attack for c in chosen} == set(signed)
    assert {c.placement for c in chosen} == set(SM.PLACEMENTS)
  # Krum and Bulyan with m
  for value in (SM.M_ARG, None):
    chosen = [c for c in product if c.rule in SM.DISTANCE and c.m == value]
    assert {c.rule for c in chosen} == set(SM.DISTANCE) and {c.attack for c in chosen} == {a.key for a in SM.ATTACKS}
    assert {c.placement for c in chosen} == set(SM.PLACEMENTS)
  assert all(c.m is None for c in product if c.rule not in SM.DISTANCE)


# ---------------------------------------------------------------------------------------------------------------------
# Plans

ACCEPT = {"krum": "count", "brute": "count", "aksel": "count", "cge": "count", "average": "average"}


def expected_plan(case, hip):
  """(first_pass, single_call, accept, forms_vector) of a case, written out here: the first pass forms the vector of
  empire and little alone; with the HIP backend's legs a coordinate-wise rule (without arguments) or the distance pass of
  Krum / Bulyan rides along at worker and update placement when somebody attacks; the single call takes worker placement,
  those six rules and those two attacks."""
  forms = case.attack in SM.FIRST_PASS_ATTACKS
  first_pass = "plain"
  if hip and forms and case.f_real >= 1 and case.placement in ("worker", "update"):
    first_pass = "rule" if case.rule in SM.COLWISE else ("sqdist" if case.rule in SM.DISTANCE else "plain")
  single = bool(hip and case.single_call and forms and case.placement == "worker" and case.rule in SM.DISTANCE + SM.COLWISE)
  return first_pass, single, ACCEPT.get(case.rule), forms


def _hip_like():
  from byzantinemomentum_amd.sharded import HipBackend

  class EveryCapability:
    capabilities = HipBackend.capabilities
    device_search_rules = ("krum", "average")

  return EveryCapability


def _plan(case, backend):
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from byzantinemomentum_amd.step import AggregationStep
  return AggregationStep(aggregator=ShardedAggregator(backend=backend(), local_only=True), **SM.constructor_kwargs(case)).plan


def _plan_key(plan):
  return tuple(plan._replace(capabilities=frozenset()))


def test_every_case_has_the_plan_written_here():
  from tests.sharded_backend import OracleBackend
  hip_like = _hip_like()
  for case in SM.cases() + SM.long_cases():
    for hip, backend in ((True, hip_like), (False, OracleBackend)):
      plan = _plan(case, backend)
      got = (plan.first_pass, plan.single_call, plan.accept, plan.forms_vector)
      assert got == expected_plan(case, hip), (case.name, hip, got)
      assert plan.search is None and not plan.searches and not plan.device_cursor
  assert all(expected_plan(c, True)[0] in ("rule", "sqdist") for c in SM.long_cases())


def test_the_cases_reach_every_plan_of_the_universe():
  """Every combination of the universe's values — the full product, secondary arguments included — through _make_plan
  with the HIP backend's capability set: the distinct plans are exactly those the cases reach."""
  hip_like = _hip_like()
  universe = set()
  for rule, att, placement, ff, single, m, negative in itertools.product(
      SM.RULES, SM.ATTACKS, SM.PLACEMENTS, SM.FF, (True, False), (None, SM.M_ARG), (False, True)):
    if m is not None and rule not in SM.DISTANCE:
      continue
    factor = att.negative if negative and att.negative is not None else att.factor
    case = SM.Case("u", rule, att.key, placement, *ff, None, m, False, single, factor, SM.D, 0, "universe")
    universe.add(_plan_key(_plan(case, hip_like)))
  reached = {_plan_key(_plan(case, hip_like)) for case in SM.cases()}
  assert reached == universe, (len(reached), len(universe))


# ---------------------------------------------------------------------------------------------------------------------
# Every case through the oracle-backed step

expected_of, run_case = SM.expected_of, SM.run_case


@pytest.mark.parametrize("rule,placement", list(itertools.product(SM.RULES, SM.PLACEMENTS)))
def test_every_case_through_the_oracle_backend(rule, placement):
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from tests.sharded_backend import OracleBackend
  todo = [c for c in SM.cases() if (c.rule, c.placement) == (rule, placement)]
  assert len(todo) >= len(SM.ATTACKS)
  for case in todo:
    bad = run_case(case, ShardedAggregator(backend=OracleBackend(), local_only=True))
    assert not bad, (case.name, bad)


def test_no_case_rests_on_a_decision_under_its_margin():
  """Zero cases left out: every step of every case (the long ones are checked where they run) clears every threshold.
  (test_every_case_through_the_oracle_backend asserts it case by case; this is the count.)"""
  under = {}
  for case in SM.cases():
    for it, exp in enumerate(expected_of(case)):
      if SM.below_margin(exp.margins):
        under[(case.name, it)] = SM.below_margin(exp.margins)
  assert len(under) == 0, under


# ---------------------------------------------------------------------------------------------------------------------
# Defect twins


class _AsStep:
  """An Expected presented as the step the comparison reads."""

  def __init__(self, exp):
    self.exp = exp
    self.buffers, self.server_momentum, self.cclip_start = exp.honests, exp.server, exp.cclip_start
    self.last_byzantine = None
    self.last_factor = exp.gamma
    if exp.byzantine is not None:
      self.last_byzantine = exp.byzantine.clone()
      if exp.info is not None:
        i = exp.info
        self.last_byzantine.attack_info = torch.tensor([i["gamma"], i["bound"], float(i["binding"]), i["P"], i["N"],
                                                        1.0 if i["degenerate"] else 0.0], dtype=torch.float64)

  def update_gradient(self):
    return self.exp.update

  def floats(self):
    return self.exp.floats


# twin -> the case that catches it (the first case, in list order, on which
# the twin differs from the loop by ten bars or more in some compared quantity)
CAUGHT_BY = {
  "attack_on_sampled": "krum-empire-worker",
  "rule_f_real": "krum-empire-update",
  "clip_after_momentum": "krum-empire-server",
  "cclip_restart": "cclip-empire-worker",
  "update_no_dampening": "krum-empire-update",
  "study_on_direction": "krum-empire-worker",
  "accept_vs_decl": "krum-empire-server",
  "extra_in_honests": "krum-empire-server",
}


def twin_distance(case, twin):
  """The largest error / bar of the twin against the loop over the case's steps and compared quantities, and where."""
  loop = SM.MatrixLoop(case, twin)
  worst, where = 0.0, None
  for it, (step_inputs, exp) in enumerate(zip(SM.inputs(case), expected_of(case))):
    other = loop.step(*step_inputs)
    for key, (err, bar) in SM.errors(case, _AsStep(other), other.defense, exp).items():
      ratio = math.inf if (bar == 0 and err > 0) or math.isinf(err) else (err / bar if bar > 0 else 0.0)
      if ratio > worst:
        worst, where = ratio, (it, key)
  return worst, where


def test_every_twin_is_named():
  assert set(CAUGHT_BY) == set(SM.TWINS)


@pytest.mark.parametrize("twin", SM.TWINS)
def test_a_defect_twin_is_caught(twin):
  case = {c.name: c for c in SM.cases()}[CAUGHT_BY[twin]]
  worst, where = twin_distance(case, twin)
  print(f"twin {twin}: caught by {case.name} at step {where[0]} in {where[1]}, {worst:.3g} bars")
  assert worst >= 10.0, (twin, case.name, worst, where)
