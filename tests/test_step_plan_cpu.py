"""The plan AggregationStep makes in its constructor (step.StepPlan): which form the first pass, the factor search and
the whole step take, from the constructor's arguments and the capabilities the backend declares.  No library, no GPU:
the backends here declare capabilities and do nothing else."""

import pytest

from byzantinemomentum_amd.sharded import HipBackend, ShardedAggregator
from byzantinemomentum_amd.step import AggregationStep
from tests.sharded_backend import OracleBackend

COLWISE = ("median", "trmean", "phocas", "meamed")
EVERY_RULE = ("krum", "bulyan", "median", "trmean", "phocas", "meamed", "aksel", "brute", "average", "cge")
SINGLE_CALL_RULES = ("krum", "bulyan") + COLWISE


class EveryCapability:
  capabilities = HipBackend.capabilities
  device_search_rules = ("krum", "average")


def plan(backend=EveryCapability, n=25, f=5, f_real=None, **kwargs):
  step = AggregationStep(n, f, f if f_real is None else f_real, aggregator=ShardedAggregator(backend=backend()), **kwargs)
  assert step.single_call is step.plan.single_call
  return step.plan


def test_the_hip_backend_declares_methods_it_has():
  assert HipBackend.capabilities and all(callable(getattr(HipBackend, name)) for name in HipBackend.capabilities)


@pytest.mark.parametrize("placement", ["worker", "update"])
def test_first_pass(placement):
  for gar in COLWISE:
    assert plan(gar=gar, momentum_at=placement).first_pass == "rule"
    assert plan(gar=gar, momentum_at=placement, gar_args={"m": 3}).first_pass == "plain"
  for gar in ("krum", "bulyan"):
    assert plan(gar=gar, momentum_at=placement).first_pass == "sqdist"
    assert plan(gar=gar, momentum_at=placement, gar_args={"m": 17}).first_pass == "sqdist"
    assert plan(gar=gar, momentum_at=placement, gar_args={"m": 17, "other": 1}).first_pass == "plain"
  for gar in EVERY_RULE:
    assert plan(gar=gar, momentum_at=placement, f_real=0).first_pass == "plain"
    assert plan(gar=gar, momentum_at=placement, attack_evals=4).first_pass == "direction"
    assert plan(gar=gar, momentum_at=placement, attack_evals=4, f_real=0).first_pass == "direction"
  for gar in ("aksel", "brute", "average", "cge"):
    assert plan(gar=gar, momentum_at=placement).first_pass == "plain"


def test_first_pass_of_the_server_placement_carries_nothing():
  for gar in EVERY_RULE:
    assert plan(gar=gar, momentum_at="server").first_pass == "plain"
    assert plan(gar=gar, momentum_at="server", attack_evals=4).first_pass == "direction"


def test_search_forms():
  def form(gar, line_search="auto", **kwargs):
    p = plan(gar=gar, attack_evals=4, line_search=line_search, **kwargs)
    return p.search, p.device_cursor

  assert plan(gar="krum").search is None and not plan(gar="krum").device_cursor
  for gar in ("krum", "average"):
    assert form(gar) == ("scalar_device", True)
    assert form(gar, "host") == ("scalar_host", False)
  assert form("krum", gar_args={"m": 3}) == ("scalar_device", True)
  assert form("brute") == form("brute", "host") == ("scalar_host", False)
  assert form("bulyan") == ("bulyan", True) and form("bulyan", "host") == ("bulyan", False)
  assert form("median") == ("median", True) and form("median", "host") == ("median", False)
  for gar in ("trmean", "phocas", "meamed"):
    assert form(gar) == ("colwise_eval", True) and form(gar, "host") == ("colwise_eval", False)
    assert form(gar, gar_args={"x": 1}) == ("generic", True)
  for gar in ("aksel", "cge"):
    assert form(gar) == ("generic", True) and form(gar, "host") == ("generic", False)
  for gar in EVERY_RULE:
    assert form(gar, "generic") == ("generic", False)
  # an argument of the rule other than "m": no special form
  assert form("krum", gar_args={"x": 1}) == ("generic", True)
  assert form("bulyan", gar_args={"x": 1}) == ("generic", True)
  # h + 2 > 64: the matrix of the scalar forms has no room, the rule runs per evaluation
  assert form("krum", n=64, f=1) == ("generic", True) and form("krum", n=63, f=1) == ("scalar_device", True)
  assert form("brute", n=64, f=1) == ("generic", False)
  assert form("bulyan", n=64, f=1) == ("generic", True)


def test_bulyan_moves_cursor_and_ranking_together():
  class NoDeviceRanking(EveryCapability):
    capabilities = HipBackend.capabilities - {"attack_ranking_device"}

  p = plan(NoDeviceRanking, gar="bulyan", attack_evals=4)
  assert (p.search, p.device_cursor) == ("bulyan", False)
  assert plan(NoDeviceRanking, gar="median", attack_evals=4).device_cursor


@pytest.mark.parametrize("gar", EVERY_RULE)
def test_single_call_is_the_expression_it_was(gar):
  for placement in ("worker", "server", "update"):
    for evals in (None, 4):
      for wanted in (True, False):
        for gar_args in ({}, {"m": 3}, {"x": 1}):
          got = plan(gar=gar, momentum_at=placement, attack_evals=evals, single_call=wanted, gar_args=gar_args).single_call
          want = (wanted and evals is None and placement == "worker" and gar in SINGLE_CALL_RULES
                  and not (set(gar_args) - {"m"}))
          assert got is want, (gar, placement, evals, wanted, gar_args)
  assert not plan(OracleBackend, gar=gar).single_call


@pytest.mark.parametrize("gar", EVERY_RULE)
def test_a_backend_without_capabilities(gar):
  """tests/sharded_backend.OracleBackend declares nothing: plain first pass, the host's cursor, no single call — and of
  the search's forms those that need no optional leg, which it has always taken (tests/test_step_cpu.py compares them
  with the generic form): the scalars of one distance pass on the host (krum, brute, average), Bulyan ranked on the
  host, the median as the middle of three rows.  Every other rule runs per evaluation."""
  host_forms = {"krum": "scalar_host", "brute": "scalar_host", "average": "scalar_host", "bulyan": "bulyan",
                "median": "median"}
  for placement in ("worker", "server", "update"):
    fixed = plan(OracleBackend, gar=gar, momentum_at=placement)
    assert (fixed.first_pass, fixed.search, fixed.device_cursor, fixed.single_call) == ("plain", None, False, False)
    for line_search in ("auto", "host", "generic"):
      p = plan(OracleBackend, gar=gar, momentum_at=placement, attack_evals=4, line_search=line_search)
      want = "generic" if line_search == "generic" else host_forms.get(gar, "generic")
      assert (p.first_pass, p.search, p.device_cursor, p.single_call) == ("direction", want, False, False)


def test_a_device_search_hands_back_its_tensor_unread():
  """_search_factor returns the tensor the device search left (multi_fma3 reads the factor there) and sets last_search
  to it; the tensor is taken apart only when last_search / last_factor are read."""
  import torch
  found = torch.tensor([1.5, 1.0, 2.0, 1.5, 3.0], dtype=torch.float64)

  class Searching(EveryCapability):
    def multi_fma3(self, outs, ps, qs, a, b):
      pass

    def pairwise_sqdist(self, rows, d_total=None):
      return torch.zeros(len(rows), len(rows), dtype=torch.float64)

    def attack_search_device(self, sq, h, k, f, rule, evals, negative, m):
      return found

  step = AggregationStep(11, 2, 2, gar="krum", attack_evals=2, aggregator=ShardedAggregator(backend=Searching()))
  rows = [torch.zeros(4) for _ in range(9)]
  assert step._search_factor(rows, rows[0], rows[1]) is found
  assert step._search_now is found
  assert step.last_search == [(1.0, 2.0), (1.5, 3.0)] and step.last_factor == 1.5


# ---- the table of attacks (step._ATTACK) and the plan fields that replaced what run() derived every step ---- #

EVERY_ATTACK = ("empire", "little", "anticge", "nan", "hidden", "empire-strict")


def test_the_table_has_the_attacks_and_no_other():
  from byzantinemomentum_amd import step
  assert set(step._ATTACK) == set(step._ATTACKS) == set(EVERY_ATTACK) and len(step._ATTACK) == len(step._ATTACKS)
  assert all(isinstance(row, step._Attack) for row in step._ATTACK.values())


@pytest.mark.parametrize("backend", [EveryCapability, OracleBackend])
@pytest.mark.parametrize("attack", EVERY_ATTACK)
def test_plan_fields_are_the_expressions_run_computed(attack, backend):
  """What run() derived from `self.attack` and `self.attack_evals` at every step before the plan stated it, written out
  from those lines: `searched`, `with_direction`, `anticge`, `vector`, `strict`, `kind`, `scale is None`, and the
  `behind` / `strict` of _make_plan and the `1 + x` of the two searches."""
  from byzantinemomentum_amd import step
  for evals in (None, 4):
    if evals is not None and attack in ("anticge", "nan"):
      with pytest.raises(ValueError, match="no factor to search"):
        plan(backend, gar="krum", attack=attack, attack_evals=evals)
      continue
    for gar in EVERY_RULE:
      for placement in ("worker", "server", "update"):
        for f_real in (5, 0):
          p = plan(backend, gar=gar, momentum_at=placement, attack=attack, attack_evals=evals, attack_factor=2,
                   f_real=f_real)
          tag = (attack, evals, gar, placement, f_real)
          # run(), as it was
          searched = evals is not None
          with_direction = p.first_pass == "direction"
          anticge = attack == "anticge"
          vector, strict = attack in ("nan", "hidden", "empire-strict"), attack == "empire-strict"
          kind = "empire" if strict else attack
          scale_is_none = anticge or (vector and not with_direction)
          assert p.searches is (searched and f_real > 0), tag              # `if searched and self.f_real > 0:`
          assert (p.search is not None) is searched, tag                   # `1.0 if searched else self.factor`
          assert p.forms_vector is (not scale_is_none), tag
          assert p.attack.first_pass == kind, tag
          assert with_direction is (searched and attack != "hidden"), tag  # _make_plan: `not fixed and attack != "hidden"`
          # _make_plan: `behind`; the stages behind the first pass: `if anticge`, `if vector`, and below it "nan",
          # "hidden", `elif not searched` (empire-strict); `if strict` where the found factor is applied
          row = p.attack
          assert row is step._ATTACK[attack], tag
          assert (row.formed != "first_pass") is (anticge or vector), tag
          assert (row.formed == "chain") is anticge and (row.formed == "kernel") is vector, tag
          assert (row.formed == "kernel" and not row.factor) is (attack == "nan"), tag
          assert (row.direction == "kernel") is (attack == "hidden"), tag
          assert (row.apply == "scale") is strict, tag
          assert row.kind == {"nan": "nan", "hidden": "shift_one", "empire-strict": "scale"}.get(attack), tag
          # _search_factor / _search_scalar: `1.0 if self.attack == "empire-strict" else 0.0`, `1.0 + x`
          assert row.shift == (1.0 if strict else 0.0), tag
          # the constructor: who takes attack_evals, `negative`, attack_args
          assert row.factor is (attack not in ("anticge", "nan")) and row.negative is (not strict), tag
          assert row.args == ({"target_idx"} if attack == "hidden" else set()), tag


UNKNOWN_ATTACK = ("unknown attack {!r} (empire, little, hidden: factor, use a negative one for negative:True; "
                  "empire-strict: epsilon; anticge, nan: no factor)")
ATTACK_ARGS = "attack_args holds {{'target_idx': int | 'all'}} for the hidden attack and nothing else, got {!r} with attack {!r}"
TARGET_IDX = "target_idx must be an integer or \"all\" (attacks/identical.py:121-124), got {!r}"
EPSILON = "the empire-strict attack takes a positive integer epsilon as attack_factor (attacks/empire.py:82), got {!r}"
ANTICGE_DECL = ("the anticge attack needs 1 <= nb_decl_byz <= {} honest workers "
                "(attacks/anticge.py:67-68 indexes the sorted norms at h - f_decl), got {}")
REFUSALS = [
  (dict(gar="nope"), "unknown aggregation rule 'nope'"),
  (dict(momentum_at="client"), "momentum_at must be 'worker', 'server' or 'update', got 'client'"),
  (dict(attack="bulyan"), UNKNOWN_ATTACK.format("bulyan")
   + "; the reference's `bulyan` attack is \"hidden\" here (bulyan names a rule)"),
  (dict(attack="empire_strict"), UNKNOWN_ATTACK.format("empire_strict")),
  (dict(attack_evals=0), "attack_evals must be a positive number of evaluations, got 0"),
  (dict(attack_evals=2.5), "attack_evals must be a positive number of evaluations, got 2.5"),
  (dict(attack="hidden", attack_evals=-1), "attack_evals must be a positive number of evaluations, got -1"),
  (dict(attack="anticge", attack_evals=4), "the anticge attack has no factor to search: attack_evals must be None"),
  (dict(attack="nan", attack_evals=4), "the nan attack has no factor to search: attack_evals must be None"),
  (dict(attack="anticge", f=0), ANTICGE_DECL.format(9, 0)),
  (dict(attack="anticge", f=10), ANTICGE_DECL.format(9, 10)),
  (dict(attack="hidden", attack_args={"target": 3}), ATTACK_ARGS.format({"target": 3}, "hidden")),
  (dict(attack="hidden", attack_args={"target_idx": 3, "more": 1}), ATTACK_ARGS.format({"target_idx": 3, "more": 1}, "hidden")),
  (dict(attack="hidden", attack_args=[3]), ATTACK_ARGS.format([3], "hidden")),
] + [
  (dict(attack=other, attack_factor=2, attack_args=given), ATTACK_ARGS.format(given, other))
  for other in ("empire", "little", "anticge", "nan", "empire-strict") for given in ({"target_idx": 3}, {})
] + [
  (dict(attack="hidden", attack_args={"target_idx": bad}), TARGET_IDX.format(bad)) for bad in (1.5, "last", None, True)
] + [
  (dict(attack="empire-strict", attack_factor=2, attack_negative=True),
   "the empire-strict attack has no `negative` (attacks/empire.py:29): attack_negative must be False"),
] + [
  (dict(attack="empire-strict", attack_factor=bad), EPSILON.format(bad)) for bad in (1.1, 2.0, 0, -3, True, None)
] + [
  (dict(line_search="device"), "line_search must be 'auto', 'host' or 'generic', got 'device'"),
  (dict(nb_past=-1), "nb_past must be within 0..4096"),
  (dict(nb_past=4097), "nb_past must be within 0..4096"),
]


def test_every_refusal_of_the_constructor_keeps_its_type_and_message():
  agg = ShardedAggregator(backend=OracleBackend())
  for kwargs, message in REFUSALS:
    kwargs = dict(kwargs)
    with pytest.raises(ValueError) as info:
      AggregationStep(11, kwargs.pop("f", 2), 2, aggregator=agg, **kwargs)
    assert type(info.value) is ValueError and str(info.value) == message, kwargs
  # what is accepted next to them
  for kwargs in (dict(attack="nan", attack_factor="ignored"), dict(attack="empire-strict", attack_factor=2),
                 dict(attack="empire-strict", attack_evals=4), dict(attack="anticge", attack_negative=True),
                 dict(attack="hidden", attack_args={"target_idx": "all"}, attack_evals=4, attack_negative=True)):
    AggregationStep(11, 2, 2, aggregator=agg, **kwargs)
  AggregationStep(11, 0, 0, aggregator=agg, attack="anticge")  # (nobody attacks: nb_decl_byz is not looked at)
