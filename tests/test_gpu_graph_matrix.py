"""Every case of tests/graph_matrix.py on the HIP backend: an AggregationStep recorded by graphs.GraphedCall (two warm-up
steps) and replayed three times, every replay on new gradients copied in place into the recorded buffers, against an
eager twin with the same arguments that runs the same five steps.  Needs an MI355X: `pytest -m gpu`.

After each replay, bit for bit (step_matrix.same_bits, NaN equal to NaN; nothing is measured, so nothing has a
tolerance): the returned defense, update_gradient(), last_byzantine and its attack_info, the buffers, server_momentum,
cclip_start, last_masks, last_factor, last_search, and every key of floats() as equal Python values — all read through
the getters after EVERY replay, so a cache that survives a replay fails.  The twin's own defense must change from step
to step (graph_matrix.moved: where it is NaN at every coordinate, the sampled norm must), so that equal cannot mean
frozen on both sides.  One stream, no environment variable, no knob.  No recording here is expected to fail: what the
step cannot replay faithfully it refuses on the host (tests/test_graph_matrix_cpu.py).

Per-item times and case counts: profiles/graph_matrix.txt."""

import itertools

import pytest
import torch

from tests import graph_matrix as GM
from tests import step_matrix as SM

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def new_step(case):
  from byzantinemomentum_amd.step import AggregationStep
  return AggregationStep(**GM.constructor_kwargs(case))


def check(case):
  from byzantinemomentum_amd.graphs import GraphedCall
  steps = GM.inputs(case)

  def device(t):
    return None if t is None else t.to(DEV)

  # the eager twin: every step on clones of that step's gradients
  eager = new_step(case)
  want = []
  for rows, params, origin in steps:
    out = eager.run([device(g) for g in rows], device(params), device(origin))
    want.append(GM.snapshot(eager, out))
  for it in range(1, GM.STEPS):
    assert GM.moved(want[it - 1], want[it]), (case.name, it, "the twin's defense did not change")

  # the graphed step: fixed buffers, each step's contents copied in place before the step runs
  graphed = new_step(case)
  assert graphed.plan.single_call is (case.single_call and SM.can_take_the_single_call(case)), case.name
  rows = [device(g) for g in steps[0][0]]
  params, origin = device(steps[0][1]), device(steps[0][2])
  warmed = []

  def load(it):
    for buffer, g in zip(rows, steps[it][0]):
      buffer.copy_(g)
    if params is not None:
      params.copy_(steps[it][1])

  def fn():
    if not torch.cuda.is_current_stream_capturing():  # a warm-up call: the recording itself runs nothing
      load(len(warmed))
      warmed.append(True)
    return graphed.run(rows, params, origin)

  call = GraphedCall(fn, warmup=GM.WARMUP)
  assert len(warmed) == GM.WARMUP
  if case.evals is not None:
    assert graphed.plan.searches and graphed.plan.device_cursor, case.name
    found = graphed._factor_now   # (not through the getter: nobody has read it yet)
    assert isinstance(found, torch.Tensor) and found.is_cuda, (case.name, type(found))
  for it in range(GM.WARMUP, GM.STEPS):
    load(it)
    out = call()
    torch.cuda.synchronize()
    got = GM.snapshot(graphed, out)
    bad = GM.differences(got, want[it])
    assert not bad, (case.name, f"replay {it - GM.WARMUP + 1}", bad)
    assert graphed.floats() is graphed.floats()  # idempotent between two replays


def test_the_capability_set_is_the_one_the_plans_were_made_with():
  from byzantinemomentum_amd.sharded import HipBackend
  step = new_step(GM.cases()[0])
  assert isinstance(step.ops, HipBackend) and step.plan.capabilities == frozenset(HipBackend.capabilities)


@pytest.mark.parametrize("rule,placement", list(itertools.product(SM.RULES, SM.PLACEMENTS)))
def test_every_replay_is_the_eager_step(rule, placement):
  todo = [c for c in GM.cases() if (c.rule, c.placement) == (rule, placement)]
  assert len(todo) >= len(SM.ATTACKS)
  for case in todo:
    check(case)
