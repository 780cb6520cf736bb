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
