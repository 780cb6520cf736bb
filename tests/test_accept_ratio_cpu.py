"""`AggregationStep.floats()["accept_ratio"]`, the 24th column of the study row ("Attack acceptation ratio",
attack.py:571,822), on the oracle-backed compute legs (tests/sharded_backend.OracleBackend: it declares no capability,
so the count is the plain-torch form of step.AggregationStep._accept_count) against the reference's OWN `influence`
functions, imported unmodified (`reference` marker), then dim-sharded over two gloo ranks, and the argument checks of
bm_accept_count, which need no GPU."""

import ctypes
import functools
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import reference_loader

D = 257
MU, DAMP = 0.9, 0.9


def sampled_for_step(it, h, d=D):
  gen = torch.Generator().manual_seed(4100 + it)
  base = 0.2 * torch.randn(d, generator=gen)
  return [base + (0.5 + 0.1 * i) * torch.randn(d, generator=gen) for i in range(h)]


def make_step(case, aggregator=None):
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from byzantinemomentum_amd.step import AggregationStep
  from tests.sharded_backend import OracleBackend
  agg = aggregator or ShardedAggregator(backend=OracleBackend())
  return AggregationStep(case["n"], case["f_decl"], case["f_real"], gar=case["gar"], gar_args=case.get("gar_args"),
                         momentum=MU, dampening=DAMP, momentum_at=case.get("momentum_at", "worker"),
                         attack=case.get("attack", "empire"), attack_factor=case.get("factor", 1.1), nb_past=2,
                         aggregator=agg, attack_evals=case.get("evals"))


def case(gar, n, f, momentum_at="worker", attack="empire", factor=1.1, f_real=None, **more):
  return dict(gar=gar, n=n, f_decl=f, f_real=f if f_real is None else f_real, momentum_at=momentum_at, attack=attack,
              factor=factor, **more)


# Every rule with a counted ratio at both sizes, every momentum placement, both attacks.  Brute stays at n = 11: at
# n = 25 the reference's own search walks C(25, 20) = 53 130 subsets of 190 pairs in Python, ~10 M iterations per call.
CASES = [case(gar, n, f, placement, attack, factor)
         for gar in ("krum", "aksel", "cge") for n, f in ((11, 2), (25, 5)) for placement in ("worker", "server", "update")
         for attack, factor in (("empire", 1.1), ("little", 1.5))]
CASES += [case("brute", 11, 2, placement, attack, factor) for placement in ("worker", "server", "update")
          for attack, factor in (("empire", 1.1), ("little", 1.5))]
CASES += [
  case("krum", 11, 2, gar_args={"m": 3}), case("krum", 25, 5, "update", "little", 1.5, gar_args={"m": 3}),
  case("aksel", 11, 2, gar_args={"mode": "n-f"}), case("aksel", 25, 5, "server", "little", 1.5, gar_args={"mode": "n-f"}),
  # the factor search (attacks/identical.py:67-77): from scalars for krum, the rule per evaluation for aksel and cge —
  # the selection counted must be the one of the LAST call of the rule, the aggregation itself
  case("krum", 11, 2, evals=5), case("aksel", 11, 2, evals=5), case("cge", 25, 5, "update", evals=5),
  # more Byzantine workers declared than real: h = 10, one copy — a count over index >= n - f_decl would see rows 8, 9
  case("krum", 11, 3, f_real=1), case("aksel", 11, 3, f_real=1), case("cge", 11, 3, f_real=1), case("brute", 11, 3, f_real=1),
  case("cge", 11, 3, "update", "little", 1.5, f_real=1),
  # an attack far from the honest rows (byz = -29 avg): no rule takes a copy
  case("krum", 11, 2, factor=30.0), case("aksel", 25, 5, factor=30.0), case("cge", 11, 2, factor=30.0),
  case("brute", 11, 2, factor=30.0),
]
# The reference's ratios of these cases as found on the CPU, steps 0 / 1 / 2 where they differ
# (test_the_cases_decide_something holds them to deciding something):
#   krum   n = 11  empire 1.1: 2/7 (m = 3: 2/3; factor search: 2/7); little 1.5: 0, at the server and the update 0 0 1/7
#          n = 25  5/18 under both attacks; little 1.5 with m = 3: 0;  f_decl 3 / f_real 1: 1/6;  factor 30: 0
#   aksel  empire 1.1: 1/3 at n = 11 (n-f: 2/9; factor search: 1/3 1/6 1/3), 5/13 at n = 25; little 1.5: 0 (n-f, n = 25:
#          1/4);  f_real 1: 1/6;  factor 30: 0
#   cge    empire 1.1: 2/9 and 1/4 (factor search: 1/4); little 1.5: 0, at n = 25 worker / server 0 0 1/20;  f_real 1: 1/8
#          (little: 0);  factor 30: 0
#   brute  empire 1.1: 2/9; little 1.5: 2/9, at the server and the update 2/9 0 2/9;  f_real 1: 1/8;  factor 30: 0


def case_id(c):
  tag = f"{c['gar']}-n{c['n']}-f{c['f_decl']}r{c['f_real']}-{c['momentum_at']}-{c['attack']}{c['factor']}"
  if c.get("gar_args"):
    tag += "-" + "-".join(f"{k}{v}" for k, v in c["gar_args"].items())
  if c.get("evals"):
    tag += f"-search{c['evals']}"
  return tag


@functools.lru_cache(maxsize=None)
def reference_rules():
  return reference_loader.load(with_native=False)[0].gars


@functools.lru_cache(maxsize=None)
def ratios_of(index):
  """[(the step's ratio, the reference's `influence` on the rows the step aggregated)] over three steps — computed once
  per case, shared by the tests below."""
  c = CASES[index]
  h = c["n"] - c["f_real"]
  step = make_step(c)
  influence = reference_rules()[c["gar"]].influence
  out = []
  for it in range(3):
    rows = sampled_for_step(it, h)
    server = step.server_momentum if step.server_momentum is not None else torch.zeros(D)
    step.run(rows)
    if c["momentum_at"] == "worker":
      honests = list(step.buffers)
    elif c["momentum_at"] == "server":  # (1 - damp) * g + mu * M with the momentum the step started from
      honests = [g.mul(1.0 - DAMP).add_(server, alpha=MU) for g in rows]
    else:
      honests = rows
    attacks = [step.last_byzantine] * c["f_real"]
    want = influence(honests, attacks, f=c["f_decl"], **(c.get("gar_args") or {}))
    out.append((step.floats()["accept_ratio"], want))
  return tuple(out)


@pytest.mark.reference
@pytest.mark.parametrize("index", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_step_reports_the_reference_influence(index):
  for it, (got, want) in enumerate(ratios_of(index)):
    print(f"{case_id(CASES[index])} step {it}: {got!r} against {want!r}")
    assert isinstance(got, float) and got == want, (case_id(CASES[index]), it, got, want)


@pytest.mark.reference
def test_the_cases_decide_something():
  """On the REFERENCE's numbers alone: a test whose every ratio is 0 (or 1) would pass with a constant."""
  wants = {i: [want for _, want in ratios_of(i)] for i in range(len(CASES))}
  flat = [w for ws in wants.values() for w in ws]
  assert any(w == 0.0 for w in flat)
  assert any(0.0 < w < 1.0 for w in flat)
  for gar in ("krum", "aksel", "cge", "brute"):
    mine = [w for i, ws in wants.items() if CASES[i]["gar"] == gar for w in ws]
    assert any(w > 0.0 for w in mine) and any(w == 0.0 for w in mine), gar
  # the declared / real case separates the two counts: exactly the one real copy is taken
  assert ratios_of(CASES.index(case("krum", 11, 3, f_real=1)))[0][1] == 1 / 6


@pytest.mark.parametrize("gar", ["bulyan", "median", "trmean", "phocas", "meamed"])
def test_rules_without_influence_report_the_nan_object(gar):
  step = make_step(case(gar, 11, 2))
  twin = make_step(case(gar, 11, 2))
  for it in range(2):
    step.run(sampled_for_step(it, 9))
    twin.run(sampled_for_step(it, 9))
    assert step.floats()["accept_ratio"] is math.nan
    assert step.floats() == twin.floats()  # (two NaNs compare equal in a dictionary only as ONE object)
  assert step.plan.accept is None


@pytest.mark.parametrize("n,f_decl,f_real", [(11, 2, 2), (25, 5, 5), (11, 3, 1), (11, 2, 0)])
def test_average_reports_the_share_of_byzantine_workers(n, f_decl, f_real):
  step = make_step(case("average", n, f_decl, f_real=f_real))
  step.run(sampled_for_step(0, n - f_real))
  assert step.floats()["accept_ratio"] == f_real / n and step.plan.accept == "average"
  if reference_loader.available():
    rows = sampled_for_step(0, n - f_real)
    assert reference_rules()["average"].influence(rows, [rows[0]] * f_real, f=f_decl) == f_real / n


@pytest.mark.parametrize("gar", ["krum", "brute", "aksel", "cge", "average"])
def test_no_byzantine_worker_gives_zero_not_nan(gar):
  """attack.py:822 calls `influence` whatever f_real: 0 of the selected rows are attacks."""
  step = make_step(case(gar, 11, 2, f_real=0))
  for it in range(2):
    step.run(sampled_for_step(it, 11))
    got = step.floats()["accept_ratio"]
    assert got == 0.0 and isinstance(got, float)


@pytest.mark.parametrize("gar", ["krum", "aksel"])
def test_floats_stays_idempotent_and_the_deque_advances(gar):
  read, lazy = make_step(case(gar, 11, 2)), make_step(case(gar, 11, 2))
  for it in range(3):
    rows = sampled_for_step(it, 9)
    read.run([g.clone() for g in rows])
    lazy.run([g.clone() for g in rows])
    want = read.floats()
    assert read.floats() is want and "accept_ratio" in want
    assert len(lazy.pasts) == len(read.pasts) == min(it + 1, 2)
    if it != 1:  # (skipped once: nothing of the step may depend on somebody reading it)
      assert lazy.floats() == want


# ---------------------------------------------------------------------------- #
# Two gloo ranks, d = 100: shards of 64 and 36 coordinates

SHARDED = [case("krum", 11, 2), case("aksel", 11, 2), case("krum", 11, 2, "update", "little", 1.5), case("cge", 11, 2)]
D_SHARDED = 100


def _free_port():
  with socket.socket() as s:
    s.bind(("127.0.0.1", 0))
    return s.getsockname()[1]


def _worker(rank, world, port, queue):
  os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
  dist.init_process_group("gloo", rank=rank, world_size=world)
  try:
    from byzantinemomentum_amd.sharded import ShardedAggregator, shard_bounds
    from tests.sharded_backend import OracleBackend
    lo, hi = shard_bounds(D_SHARDED, world, rank)
    out = {}
    for ci, c in enumerate(SHARDED):
      agg = ShardedAggregator(backend=OracleBackend())
      assert agg.collective
      step = make_step(c, agg)
      for it in range(3):
        step.run([g[lo:hi].clone() for g in sampled_for_step(it, c["n"] - c["f_real"], D_SHARDED)])
        out[(ci, it)] = step.floats()["accept_ratio"]
    queue.put((rank, out))
    dist.barrier()
  finally:
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_every_rank_reports_the_single_rank_ratio():
  """The count joins the maxima of the packed exchange: a sum over the ranks would report twice the ratio."""
  world = 2
  ctx = mp.get_context("spawn")
  queue = ctx.Queue()
  port = _free_port()
  procs = [ctx.Process(target=_worker, args=(r, world, port, queue)) for r in range(world)]
  for p in procs:
    p.start()
  results = dict(queue.get(timeout=240) for _ in range(world))
  for p in procs:
    p.join(timeout=60)
    assert p.exitcode == 0
  positive = 0
  for ci, c in enumerate(SHARDED):
    single = make_step(c)
    for it in range(3):
      single.run(sampled_for_step(it, c["n"] - c["f_real"], D_SHARDED))
      want = single.floats()["accept_ratio"]
      positive += want > 0
      for r in range(world):
        assert results[r][(ci, it)] == want, (case_id(c), it, r, results[r][(ci, it)], want)
  assert positive >= 3  # (a sum over two ranks of a zero count would go unnoticed)


# ---------------------------------------------------------------------------- #
# The C entry point: refused before any launch, so this runs without a GPU

def test_accept_count_refuses_bad_arguments():
  from byzantinemomentum_amd import _lib, build
  build.build()
  lib = _lib.load()
  order = (ctypes.c_int32 * 64)()
  out = (ctypes.c_double * 1)()
  call = lib.bm_accept_count
  assert call(None, 7, 9, out, None) == _lib.EINVAL        # no selection
  assert call(order, 7, 9, None, None) == _lib.EINVAL      # nowhere to write
  assert call(order, -1, 9, out, None) == _lib.EINVAL      # count < 0
  assert call(order, 65, 9, out, None) == _lib.EINVAL      # count > BM_MAX_ROWS
  assert call(order, 7, -1, out, None) == _lib.EINVAL      # h < 0
  assert lib.bm_abi_version() == 23 == _lib.ABI_VERSION
  assert lib.bm_step_stats_count() == 32 and _lib.STEP_ACCEPT == 30
  assert {"bm_accept_count", "bm_sharded_order_slot"} <= set(_lib.SIGNATURES)
