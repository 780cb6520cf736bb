"""Every case of tests/step_matrix.py — rule x attack x momentum placement with the secondary arguments laid over it,
the plan cases and the long first-pass cases — through AggregationStep on the HIP backend against the float64 loop
(step_matrix.MatrixLoop).  Needs an MI355X: `pytest -m gpu`.

Compared, every step: the defense, update_gradient(), last_byzantine, the buffers or server_momentum, cclip_start,
every key of floats(), and gamma (last_factor and attack_info) for minmax / minsum — step_matrix.errors, at the bars the
project already holds each rule and attack to (step_matrix.rule_bar / floats_bar / BAR_GAMMA).  Where the loop's output
is not finite (the nan attack against the rules that do not filter it) the device's must be non-finite at exactly those
coordinates; nothing is exempt.  The plain constructor runs every case; the center and spectral rules also run on
ShardedAggregator(local_only=True), as their own tests do.  Where the plan can take the single call the case runs in
both forms, which must agree bit for bit and are both held against the loop.

The worst error of every quantity per (rule, attack), measured on an MI355X by scripts/step_matrix_probe.py, is in
profiles/step_matrix_errors.txt.  Every combination keeps the bars above but these, which exceed them while every decision
of the device agrees with the loop's and are held to 4 x their measured worst (step_matrix.MEASURED_BARS):
  geomed x hidden-last  defense, update, server momentum in relative norm: worst 5.963e-07 (bar of the rule 4.080e-07) -> 2.385e-06
  caf x little          the same quantities: worst 4.576e-07 (4.072e-07) -> 1.830e-06
  dnc x anticge         the same quantities: worst 4.321e-07 (3.897e-07) -> 1.728e-06
  geomed, cclip, caf, dnc x every attack
                        floats()["curv_sampled"], a key that involves neither rule nor attack: worst 1.134e-06 (geomed,
                        caf, dnc x six attacks; center_cases.FLOATS_BAR 7.772e-07; the reference's rules hold it to
                        1e-5) -> 4.536e-06, one bar for the four rules
Min-Max / Min-Sum: their allowance holds the Byzantine vector and gamma; the rule's outputs keep the rule's own bar.
Under the nan attack the outputs of the rules that do not filter it (the average, the median, meamed) are non-finite
exactly where the loop's are: no case needed an exemption."""

import itertools

import pytest
import torch

from tests import step_matrix as SM

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def aggregators(case):
  from byzantinemomentum_amd.sharded import ShardedAggregator
  yield "plain", None
  if case.rule in SM.CENTER + SM.SPECTRAL:
    yield "local_only", ShardedAggregator(local_only=True)


def same(a, b):
  if isinstance(a, torch.Tensor):
    return SM.same_bits(a, b)
  if isinstance(a, list):
    return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
  return a == b


def check(case):
  can_single = SM.can_take_the_single_call(case)
  for tag, aggregator in aggregators(case):
    if not can_single:
      bad = SM.run_case(case, aggregator, DEV, expect_single=False)
      assert not bad, (case.name, tag, bad)
      continue
    records, shared = {}, []
    for single in (True, False):
      records[single] = []
      bad = SM.run_case(case._replace(single_call=single), aggregator, DEV, record=records[single], expect_single=single,
                        expectations=shared)
      assert not bad, (case.name, tag, single, bad)
    for it, (one, sequence) in enumerate(zip(records[True], records[False])):
      for key in one:
        assert same(one[key], sequence[key]), (case.name, it, key)


def test_the_capability_set_is_the_one_the_plans_were_made_with():
  """tests/test_step_matrix_cpu.py makes its plans with HipBackend.capabilities, read without a GPU: the live backend
  declares the same set."""
  from byzantinemomentum_amd.sharded import HipBackend, ShardedAggregator
  from byzantinemomentum_amd.step import AggregationStep
  step = AggregationStep(11, 2, 2, aggregator=ShardedAggregator())
  assert isinstance(step.ops, HipBackend) and step.plan.capabilities == frozenset(HipBackend.capabilities)


@pytest.mark.parametrize("rule,placement", list(itertools.product(SM.RULES, SM.PLACEMENTS)))
def test_every_case_on_the_device(rule, placement):
  todo = [c for c in SM.cases() if (c.rule, c.placement) == (rule, placement)]
  assert len(todo) >= len(SM.ATTACKS)
  for case in todo:
    check(case)


@pytest.mark.parametrize("case", SM.long_cases(), ids=lambda c: c.name)
def test_first_pass_riding_along_at_its_fused_and_fallback_lengths(case):
  """step_matrix.long_cases: the mirror of the dispatch (tests/first_pass_matrix.is_fused) says which of them launch the
  fused instance on this device's compute units — the rule riding along at n = 25, d = 1028, the distance pass of Krum
  and Bulyan at n = 25, d = 4 194 304 (the float64 loop takes 10-16 s on such a case: the shortest length the mirror
  allows) — and which fall back (update placement at d = 1027, n = 11 at d = 524 288)."""
  from tests import first_pass_matrix as FP
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  entry, ks, h, nb = SM.first_pass_entry(case)
  probe = FP._case("step", entry, ks, h, nb=nb, d=case.d, clip=case.clip is not None)
  fused = FP.is_fused(probe, cus)
  print(f"{case.name}: {entry} ks = h = {h}, {nb} copies, d = {case.d}: fused = {fused}")
  assert fused == ("fused" in case.name)
  check(case)
