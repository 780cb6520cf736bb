"""The acceptation count on the device: bm_accept_count against a Python count on hand-made selections, and
`AggregationStep.floats()["accept_ratio"]` against a plain count over the selections gars.py reports for the same rows
(`krum_selection`, `brute_selection`, `aksel_selection`, `cge_selection`: the suite pins those against the reference's
fixtures elsewhere).  The division is Python's `int / int` on both sides, so every comparison is `==`."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = 4099  # odd: the vector kernels of the step end in a ragged tail


# ---------------------------------------------------------------------------- #
# bm_accept_count

def count_on_device(order, count, h):
  from byzantinemomentum_amd import stats
  table = torch.tensor(order, dtype=torch.int32, device=DEV)
  got = stats.accept_count(table, count, h)
  assert got.dtype == torch.float64 and got.shape == (1,) and got.device == table.device
  return got.item()


@pytest.mark.parametrize("n", [1, 7, 25, 51, 64])
def test_accept_count_against_a_python_count(n):
  gen = torch.Generator().manual_seed(n)
  perm = torch.randperm(n, generator=gen).tolist()
  cases = []  # (order, count, h)
  for h in sorted({0, 1, n // 2, n - 1, n}):
    for count in sorted({0, 1, n // 2, n - 1, n}):
      cases.append((perm, count, h))
  cases.append((list(range(n)), n, n))                                # no entry >= h
  cases.append((list(range(n)), n, 0))                                # every entry >= h
  cases.append(([n - 1] * n, n, n - 1))                               # every entry the SAME row >= h (aliased copies)
  if n >= 2:
    last = list(range(n - 1)) + [n - 1]                               # only the last counted entry >= h
    cases.append((last, n, n - 1))
    behind = list(range(n - 2)) + [0, n - 1]                          # an entry >= h just behind the counted prefix
    cases.append((behind, n - 1, n - 1))
    cases.append((behind, n, n - 1))
  cases.append((perm + [63] * (64 - n), n, 0 if n == 1 else n // 2))  # a 64-entry table: what lies behind n is not read as counted
  for order, count, h in cases:
    want = sum(1 for i in order[:count] if i >= h)
    got = count_on_device(order, count, h)
    assert got == want and got == int(got), (n, order, count, h, got, want)
  # the behind-the-prefix pair really differs by that one entry
  if n >= 2:
    assert count_on_device(behind, n, n - 1) == count_on_device(behind, n - 1, n - 1) + 1


def test_accept_count_refuses_what_the_kernel_could_not_read():
  from byzantinemomentum_amd import gars, stats
  table = torch.arange(7, dtype=torch.int32, device=DEV)
  for bad in (lambda: stats.accept_count(table, 8, 3),                 # more than the table holds
              lambda: stats.accept_count(table, -1, 3),
              lambda: stats.accept_count(table, 3, -1),
              lambda: stats.accept_count(table.long(), 3, 3),
              lambda: stats.accept_count(table.cpu(), 3, 3)):
    with pytest.raises(gars.GarInputError):
      bad()


# ---------------------------------------------------------------------------- #
# The step

SIZES = [(11, 2), (25, 5), (51, 12)]  # (25, 5): h = 20, the first pass with the distance pass inside


def sampled_for_step(it, count, seed=0):
  gen = torch.Generator().manual_seed(7300 + 10 * seed + it)
  base = 0.2 * torch.randn(D, generator=gen)
  return [(base + (0.5 + 0.05 * i) * torch.randn(D, generator=gen)).to(DEV) for i in range(count)]


def make_step(gar, n, f, f_real=None, **kwargs):
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from byzantinemomentum_amd.step import AggregationStep
  kwargs.setdefault("nb_past", 2)
  kwargs.setdefault("attack_factor", 1.1)
  return AggregationStep(n, f, f if f_real is None else f_real, gar=gar, momentum=0.9, dampening=0.9,
                         aggregator=ShardedAggregator(local_only=True), **kwargs)


def plain_ratio(selection, h):
  return sum(1 for i in selection if i >= h) / len(selection)


def rows_of(step, honests):
  return list(honests) + [step.last_byzantine] * step.f_real


@pytest.mark.parametrize("attack,factor", [("empire", 1.1), ("little", 1.5)])
@pytest.mark.parametrize("n,f", SIZES)
def test_krum_step_in_both_forms(n, f, attack, factor):
  from byzantinemomentum_amd import gars
  one = make_step("krum", n, f, single_call=True, attack=attack, attack_factor=factor)
  seq = make_step("krum", n, f, single_call=False, attack=attack, attack_factor=factor)
  assert one.single_call and not seq.single_call and one.plan.accept == seq.plan.accept == "count"
  for it in range(2):
    sampled = sampled_for_step(it, n - f)
    one.run([g.clone() for g in sampled])
    seq.run([g.clone() for g in sampled])
    fa, fb = one.floats(), seq.floats()
    assert fa == fb, (n, f, it, {k: (fa[k], fb[k]) for k in fa if fa[k] != fb[k]})
    want = plain_ratio(gars.krum_selection(rows_of(seq, seq.buffers), f), n - f)
    print(f"krum n={n} f={f} {attack} step {it}: {fa['accept_ratio']!r} against {want!r}")
    assert fa["accept_ratio"] == want and isinstance(fa["accept_ratio"], float)


@pytest.mark.parametrize("single_call", [True, False])
def test_krum_step_with_m_and_with_fewer_real_byzantine_workers(single_call):
  from byzantinemomentum_amd import gars
  n, f_decl = 11, 3
  for f_real, m in ((1, None), (3, 4), (0, None)):
    step = make_step("krum", n, f_decl, f_real=f_real, single_call=single_call, gar_args={} if m is None else {"m": m})
    assert step.single_call is single_call
    for it in range(2):
      step.run(sampled_for_step(it, n - f_real, seed=1))
      got = step.floats()["accept_ratio"]
      want = plain_ratio(gars.krum_selection(rows_of(step, step.buffers), f_decl, m), n - f_real)
      assert got == want and isinstance(got, float), (f_real, m, it, got, want)
      assert f_real > 0 or got == 0.0


def test_krum_step_through_the_single_call_rule():
  """Momentum at the update with one more gradient sampled than honest workers: the first pass is the plain one and
  the rule is ShardedAggregator.krum's one C call — the count reads the ranking where that call left it."""
  from byzantinemomentum_amd import gars
  n, f = 25, 5
  step = make_step("krum", n, f, momentum_at="update")
  assert step.agg.single_call and not step.single_call
  for it in range(2):
    sampled = sampled_for_step(it, n - f + 1, seed=2)
    step.run(sampled)
    got = step.floats()["accept_ratio"]
    assert got == plain_ratio(gars.krum_selection(rows_of(step, sampled[:n - f]), f), n - f), (it, got)


@pytest.mark.parametrize("n,f", SIZES)
@pytest.mark.parametrize("gar", ["brute", "aksel", "cge"])
def test_selection_rules_in_the_step(gar, n, f):
  from byzantinemomentum_amd import gars
  step = make_step(gar, n, f)
  assert not step.single_call and step.plan.accept == "count"
  for it in range(2):
    step.run(sampled_for_step(it, n - f, seed=3))
    got = step.floats()["accept_ratio"]
    rows = rows_of(step, step.buffers)
    gars.invalidate_rank_cache()
    if gar == "brute":
      selection = gars.brute_selection(rows, f)
    elif gar == "aksel":
      selection = gars.aksel_selection(rows, f)
    else:
      selection = gars.cge_selection(rows, f)[:n - f].tolist()
    want = plain_ratio(selection, n - f)
    print(f"{gar} n={n} f={f} step {it}: {got!r} against {want!r}")
    assert got == want and isinstance(got, float), (gar, n, f, it, got, want)


def test_aksel_mode_and_rules_without_a_ratio():
  from byzantinemomentum_amd import gars
  n, f = 25, 5
  step = make_step("aksel", n, f, gar_args={"mode": "n-f"})
  step.run(sampled_for_step(0, n - f, seed=4))
  assert step.floats()["accept_ratio"] == plain_ratio(gars.aksel_selection(rows_of(step, step.buffers), f, "n-f"), n - f)
  average = make_step("average", n, f)
  average.run(sampled_for_step(0, n - f, seed=4))
  assert average.floats()["accept_ratio"] == f / n
  for gar in ("bulyan", "median", "trmean"):
    for single_call in (True, False):
      other = make_step(gar, n, f, single_call=single_call)
      other.run(sampled_for_step(0, n - f, seed=4))
      assert other.floats()["accept_ratio"] is math.nan, (gar, single_call)


def test_brute_counts_the_selection_that_was_averaged():
  """The device search gives up (status -2, forced by a budget of one search-tree node): the step repeats the search on
  the host and averages THAT subset — the index table the device left holds -1 everywhere and would count nothing."""
  from byzantinemomentum_amd import _lib, gars
  n, f = 11, 2
  lib = _lib.load()
  usual = make_step("brute", n, f)
  usual.run(sampled_for_step(0, n - f, seed=5))
  want = usual.floats()["accept_ratio"]
  assert want == plain_ratio(gars.brute_selection(rows_of(usual, usual.buffers), f), n - f) and want > 0
  gars.invalidate_rank_cache()
  assert lib.bm_tuning_set(b"BM_BRUTE_BUDGET", 1) == 0
  try:
    step = make_step("brute", n, f)
    defense = step.run(sampled_for_step(0, n - f, seed=5))
    got = step.floats()["accept_ratio"]
  finally:
    lib.bm_tuning_set(b"BM_BRUTE_BUDGET", 0)
    gars.invalidate_rank_cache()
  assert step.agg.brute_status is None  # (the host search answered)
  assert got == want and bool(defense.isfinite().all())


# ---------------------------------------------------------------------------- #
# HIP graph

def test_a_captured_krum_step_reports_the_eager_ratio():
  """One krum step recorded through graphs.GraphedCall and replayed once: the count is part of the recording (the
  statistics vector the replay fills is the one floats() reads).  nb_past = 0: a replay does not run the Python of the
  step again, so the step keeps no state of its own beyond the momentum buffers, which the recorded kernels update in
  place.  Warm-up (2 runs) + one replay = three steps on the same sampled gradients; the eager twin runs three."""
  from byzantinemomentum_amd.graphs import GraphedCall
  n, f = 25, 5
  sampled = sampled_for_step(0, n - f, seed=6)
  graphed = make_step("krum", n, f, nb_past=0)
  eager = make_step("krum", n, f, nb_past=0)
  assert graphed.single_call
  call = GraphedCall(lambda: graphed.run(sampled), warmup=2)
  defense = call()
  got = graphed.floats()
  for _ in range(3):
    want_defense = eager.run(sampled)
  want = eager.floats()
  assert torch.equal(defense, want_defense)
  for x, y in zip(graphed.buffers, eager.buffers):
    assert torch.equal(x, y)
  print(f"graphed krum step: {got['accept_ratio']!r} against {want['accept_ratio']!r}")
  assert got["accept_ratio"] == want["accept_ratio"] and 0.0 < want["accept_ratio"] < 1.0
  assert got == want
