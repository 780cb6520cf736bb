"""The geometric median and centered clipping through ShardedAggregator and AggregationStep on CPU, with the
oracle-backed compute legs (tests/sharded_backend.OracleBackend declares no capability, so the rules take the plain
torch legs of byzantinemomentum_amd.sharded): against the float64 iteration on the vectors, dim-sharded over two gloo
ranks against one rank, and the step's handling of the centered-clipping start."""

import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import reference_loader
from tests import center_cases as cc

# float32 output of a float64 combination against the float64 vector iteration: the weights agree to ~1e-15
# (test_center_weights_cpu.py), what is left is the rounding of the result to float32, 2^-24 per coordinate
BAR = 2.0 ** -23


def _tensors(rows):
  """One tensor per DISTINCT row: the k copies of the Byzantine row are k references to one tensor."""
  seen, out = {}, []
  for r in rows:
    key = r.tobytes()
    if key not in seen:
      seen[key] = torch.from_numpy(r.copy())
    out.append(seen[key])
  return out


def _aggregator():
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from tests.sharded_backend import OracleBackend
  return ShardedAggregator(backend=OracleBackend())


@pytest.mark.parametrize("mode", ["geomed", "cclip"])
@pytest.mark.parametrize("case", cc.cases(), ids=cc.case_id)
def test_rules_match_the_vector_iteration(case, mode):
  rows, start = cc.make_rows(case)
  param, iters = cc.params(case, mode)
  agg = _aggregator()
  local = _tensors(rows)
  if mode == "geomed":
    out = agg.geomed(local, case.k, nu=param, iters=iters)
    ref, _ = cc.vector_iteration(rows, mode, param, iters)
  else:
    out = agg.cclip(local, case.k, tau=param, iters=iters, start=torch.from_numpy(start))
    ref, _ = cc.vector_iteration(rows, mode, param, iters, start=start)
  assert out.dtype == torch.float32 and out.shape == (case.d,)
  assert cc.relative_error(out.double().numpy(), ref) <= BAR
  weights = agg.last_weights
  assert weights.shape == (64,) and abs(float(weights.sum()) - 1.0) <= 1e-12
  assert agg.last_center_info.tolist()[0] == iters and agg.last_center_info.tolist()[2] == case.n


def test_torch_leg_equals_the_host_form_on_crafted_matrices():
  """The plain torch leg follows the library's definition: same weights as bm_center_weights (to rounding), the same
  exclusions, NaN when no row is usable."""
  from byzantinemomentum_amd import _lib
  from byzantinemomentum_amd.torch_legs import _center_weights_torch
  lib = _lib.load()
  case = cc.cases()[0]
  rows, start = cc.make_rows(case)
  points = np.concatenate([rows, start[None, :]])
  sq = cc.exact_sqdist(points)
  for nan_rows, has_start in (([], True), ([9, 10], True), ([9, 10, 11], True), ([3], False), (list(range(5, 11)), False)):
    bad = sq.copy()
    bad[nan_rows, :] = math.nan
    bad[:, nan_rows] = math.nan
    N = 12 if has_start else 11
    for mode in ("geomed", "cclip"):
      param, iters = cc.params(case, mode)
      code, want, info = cc.host_weights(lib, bad[:N, :N], 11, mode, param, iters, has_start=has_start)
      got, got_info = _center_weights_torch(torch.from_numpy(bad[:N, :N].copy()), 11, mode, param, iters, 0.0, has_start)
      assert code == 0
      np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, atol=0, equal_nan=True)
      # (move^2 is a difference of the weights, at convergence their rounding alone: 1e-29 on distances of 1e4)
      np.testing.assert_allclose(got_info.numpy(), info, rtol=1e-6, atol=1e-24, equal_nan=True)


def test_nan_rows_do_not_reach_the_output():
  case = cc.cases()[4]  # n = 25, k = 5
  rows, _ = cc.make_rows(case)
  local = _tensors(rows)
  nan_row = torch.full_like(local[0], math.nan)
  stack = local[:20] + [nan_row] * 5   # the `nan` attack: five references to one NaN vector
  agg = _aggregator()
  out = agg.geomed(stack, 5, nu=1e-6, iters=8)
  ref, _ = cc.vector_iteration(rows[:20], "geomed", 1e-6, 8)
  assert torch.isfinite(out).all() and cc.relative_error(out.double().numpy(), ref) <= BAR
  assert not agg.last_weights[20:].any()
  out = agg.cclip(stack, 5, tau=math.sqrt(case.d), iters=3)
  ref, _ = cc.vector_iteration(rows[:20], "cclip", math.sqrt(case.d), 3)
  assert torch.isfinite(out).all() and cc.relative_error(out.double().numpy(), ref) <= BAR
  # a majority of NaN rows: NaN everywhere, never the combination of some rows
  out = agg.geomed(local[:10] + [nan_row] * 15, 5)
  assert torch.isnan(out).all()


def test_row_limits_and_required_arguments():
  agg = _aggregator()
  rows = [torch.zeros(8) for _ in range(65)]
  from byzantinemomentum_amd.gars import GarInputError
  with pytest.raises(GarInputError):
    agg.geomed(rows, 0)
  with pytest.raises(GarInputError):
    agg.cclip(rows[:64], 0, tau=1.0, start=torch.zeros(8))
  assert agg.geomed(rows[:64], 0).shape == (8,)
  assert agg.cclip(rows[:63], 0, tau=1.0, start=torch.zeros(8)).shape == (8,)
  with pytest.raises(ValueError):
    agg.cclip(rows[:5], 0)                      # tau is required
  for bad in (dict(nu=0.0), dict(nu=-1.0), dict(iters=0), dict(iters=65), dict(tol=-1.0), dict(iters=2.5)):
    with pytest.raises(ValueError):
      agg.geomed(rows[:5], 0, **bad)
  with pytest.raises(ValueError):
    agg.cclip(rows[:5], 0, tau=0.0)


# ---------------------------------------------------------------------------- #
# two gloo ranks, each holding half of the coordinates

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
    case = cc.cases()[0]
    rows, start = cc.make_rows(case)
    lo, hi = shard_bounds(case.d, world, rank)
    local = _tensors(np.ascontiguousarray(rows[:, lo:hi]))
    agg = ShardedAggregator(backend=OracleBackend())
    assert agg.world_size == world
    res = {}
    nu, giters = cc.params(case, "geomed")
    tau, citers = cc.params(case, "cclip")
    res["geomed"] = agg.all_gather_output(agg.geomed(local, case.k, nu=nu, iters=giters), case.d)
    res["geomed_w"] = agg.last_weights.clone()
    res["cclip"] = agg.all_gather_output(
      agg.cclip(local, case.k, tau=tau, iters=citers, start=torch.from_numpy(start[lo:hi].copy())), case.d)
    res["cclip_w"] = agg.last_weights.clone()
    res["totals_ok"] = all(t == case.d for t in agg.backend.totals_seen)
    queue.put((rank, {k: (v.detach().numpy().copy() if torch.is_tensor(v) else v) for k, v in res.items()}))
    dist.barrier()
  finally:
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_sharded_rules_match_the_unsharded_call():
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
  case = cc.cases()[0]
  rows, start = cc.make_rows(case)
  agg = _aggregator()
  nu, giters = cc.params(case, "geomed")
  tau, citers = cc.params(case, "cclip")
  want = {"geomed": agg.geomed(_tensors(rows), case.k, nu=nu, iters=giters).numpy()}
  want["geomed_w"] = agg.last_weights.numpy().copy()
  want["cclip"] = agg.cclip(_tensors(rows), case.k, tau=tau, iters=citers, start=torch.from_numpy(start)).numpy()
  want["cclip_w"] = agg.last_weights.numpy().copy()
  for r in range(world):
    assert results[r]["totals_ok"]
    for name in ("geomed", "cclip"):
      # the distances of the halves add up to the whole's to rounding (1e-16 relative), so do the weights; the output
      # is the same float32 vector up to one rounding
      np.testing.assert_allclose(results[r][name + "_w"], want[name + "_w"], rtol=1e-10, atol=1e-16)
      assert results[r][name].shape == want[name].shape
      assert cc.relative_error(results[r][name].astype(np.float64), want[name].astype(np.float64)) <= BAR
  for name in ("geomed_w", "cclip_w"):   # every rank computes the same bits from the same all-reduced matrix
    assert np.array_equal(results[0][name], results[1][name])


# ---------------------------------------------------------------------------- #
# the step

N, F, D = 11, 2, 1536


def _sampled(it, h):
  gen = torch.Generator().manual_seed(2000 + it)
  base = 0.2 * torch.randn(D, generator=gen)
  return [base + (0.5 + 0.1 * i) * torch.randn(D, generator=gen) for i in range(h)]


def _step(gar, gar_args, **kw):
  from byzantinemomentum_amd.step import AggregationStep
  return AggregationStep(N, F, F, gar=gar, gar_args=gar_args, momentum=0.9, dampening=0.9, attack="empire",
                         attack_factor=1.1, nb_past=3, aggregator=_aggregator(), **kw)


@pytest.mark.parametrize("placement", ["worker", "update", "server"])
def test_cclip_step_carries_its_start_from_step_to_step(placement):
  tau = 1.0   # well inside the spread of the rows at every placement: every step clips, the start keeps weight
  step = _step("cclip", dict(tau=tau, iters=3), momentum_at=placement)
  assert step.cclip_start is None
  previous = None
  for it in range(3):
    sampled = _sampled(it, N - F)
    defense = step.run([g.clone() for g in sampled])
    # the rule saw honests + [byz] * f: rebuild its answer from the vectors the step kept — the worker buffers, the
    # sampled rows themselves (update), or (1 - damp) g + mu M with M the previous defense vector (server,
    # attack.py:805-808, the backend's own operations) — and from the start it must have used: the PREVIOUS defense
    # vector, with the values it had when it was returned
    if placement == "worker":
      honests = step.buffers
    elif placement == "update":
      honests = sampled
    else:
      mom = torch.zeros(D) if previous is None else previous
      honests = [g.mul(0.1).add_(mom, alpha=0.9) for g in sampled]
    if previous is not None:
      assert torch.equal(previous, previous_values)     # nobody wrote the vector the step holds as its start
    stack = [b.numpy() for b in honests] + [step.last_byzantine.numpy()] * F
    ref, _ = cc.vector_iteration(np.stack(stack), "cclip", tau, 3, start=None if previous is None else previous_values.numpy())
    assert cc.relative_error(defense.double().numpy(), ref) <= BAR
    assert step.cclip_start is defense          # held by the step, advanced by the defense alone
    if previous is not None:
      assert previous is not defense and not torch.equal(previous, defense)
      assert step.agg.last_weights[N] != 0      # the start vector carries weight: it was handed to the rule
    else:
      assert step.agg.last_weights[N] == 0      # first step: no start, the uniform one
    floats = step.floats()
    assert math.isnan(floats["accept_ratio"])
    previous, previous_values = defense, defense.clone()


@pytest.mark.parametrize("gar,gar_args", [("geomed", dict(nu=1e-6, iters=8)), ("cclip", dict(tau=20.0))])
def test_factor_search_runs_the_rule_and_leaves_the_start_alone(gar, gar_args):
  step = _step(gar, gar_args, attack_evals=4)
  assert step.plan.search == "generic"
  step.run(_sampled(0, N - F))
  before = step.cclip_start
  defense = step.run(_sampled(1, N - F))
  assert len(step.last_search) == 4
  if gar == "cclip":
    assert before is not None and step.cclip_start is defense
    # during the search of step 2 the start was step 1's defense vector: replay one evaluation and see it unmoved
    held = step.cclip_start
    step._generic_objective(step.buffers, step.buffers[0], step.buffers[1])(0.5)
    assert step.cclip_start is held
  else:
    assert step.cclip_start is None


@pytest.mark.parametrize("gar,gar_args", [("geomed", {}), ("geomed", dict(nu=1e-3, iters=4, tol=1e-9)),
                                           ("cclip", dict(tau=3.0)), ("cclip", dict(tau=3.0, iters=2, tol=0.0))])
@pytest.mark.parametrize("placement", ["worker", "update", "server"])
@pytest.mark.parametrize("evals", [None, 4])
def test_plan_fields(gar, gar_args, placement, evals):
  from byzantinemomentum_amd.sharded import HipBackend, ShardedAggregator
  from byzantinemomentum_amd.step import AggregationStep

  class Caps:  # the plan reads the capabilities alone: the HIP backend's, without a GPU
    capabilities = HipBackend.capabilities
    device_search_rules = ("krum", "average")

  for backend in (Caps(), None):
    agg = ShardedAggregator(backend=backend) if backend is not None else _aggregator()
    step = AggregationStep(25, 5, 5, gar=gar, gar_args=gar_args, momentum_at=placement, aggregator=agg,
                           attack_evals=evals, single_call=True)
    plan = step.plan
    # (with a search the first pass of EVERY rule forms the direction alone; neither the rule nor a distance pass rides)
    assert plan.first_pass == ("direction" if evals else "plain")
    assert plan.search == ("generic" if evals else None)
    assert plan.accept is None
    assert plan.single_call is False and step.single_call is False


def test_bad_gar_args_raise():
  for gar, bad in (("geomed", dict(tau=1.0)), ("geomed", dict(nu=0.0)), ("geomed", dict(nu=-1.0)),
                   ("geomed", dict(iters=0)), ("geomed", dict(iters=65)), ("geomed", dict(tol=-1.0)),
                   ("geomed", dict(m=3)), ("cclip", {}), ("cclip", dict(iters=3)), ("cclip", dict(tau=0.0)),
                   ("cclip", dict(tau=-2.0)), ("cclip", dict(tau=1.0, nu=1e-6)), ("cclip", dict(tau=1.0, iters=1.5)),
                   ("cclip", dict(tau=1.0, tol=math.nan)), ("cclip", dict(tau=1.0, start=None))):
    with pytest.raises(ValueError):
      _step(gar, bad)
  _step("geomed", {})
  _step("geomed", dict(nu=1e-3, iters=64, tol=1e-6))
  _step("cclip", dict(tau=1.0, iters=1))


def test_package_exports_the_rules():
  import byzantinemomentum_amd as bm
  assert bm.geomed is bm.gars.geomed and bm.cclip is bm.gars.cclip
  with pytest.raises(bm.gars.GarInputError):
    bm.geomed([torch.zeros(4)], 0)             # CPU tensors are refused loudly: there is no fallback
  with pytest.raises(ValueError):
    bm.cclip([torch.zeros(4)], 0)              # tau is required


@pytest.mark.reference
def test_native_registers_both_rules_with_the_reference():
  """With the unmodified reference's registry: `import aggregators` keeps the reference's own set of native rules;
  native.register_center_rules() adds native-geomed and native-cclip, checked like the other extra rules, without an
  influence."""
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  code = ("import aggregators, native\n"
          "assert 'native-geomed' not in aggregators.gars and 'native-cclip' not in aggregators.gars\n"
          "assert native.register_center_rules() == ['native-geomed', 'native-cclip']\n"
          "native.register_center_rules()\n"
          "for name in ('native-geomed', 'native-cclip'):\n"
          "  rule = aggregators.gars[name]\n"
          "  assert rule.influence is None\n"
          "  assert rule.check(gradients=[], f=1) is not None\n"
          "  assert rule.check(gradients=[1, 2, 3], f=1) is None\n"
          "print('ok')\n")
  env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, reference_loader.REFERENCE_DIR]))
  out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd="/tmp")
  assert out.returncode == 0, out.stderr
  assert out.stdout.strip().splitlines()[-1] == "ok"
