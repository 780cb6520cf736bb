"""The geometric median and centered clipping end to end on the GPU (distance pass -> weights -> weighted sum), on the
cases of test_center_weights_cpu.py plus the rows of the `nan` attack:
  (a) composition — the output against a float64 weighted sum of the rows under the weights the HOST form gives on the
      device's own distance matrix, within the bound of the weighted sum: nothing measured in it;
  (b) against the float64 iteration on the vectors — what is left is the error of the distance pass (1e-6 of a
      distance for plain stacks, 1e-5 at worst: tests/distance_matrix.py) carried through the iteration.
  A GraphedCall of either rule records, replays on changed rows and equals the eager call bit for bit.
Needs an MI355X: `pytest -m gpu`.

(b), measured on an MI355X over these cases (profiles/center_errors.txt holds every case): worst relative error
  geomed 1.020e-07, cclip 1.062e-07, both at n51-k12-empire — the rounding of the fp32 output and of the fp32 weights
  more than the error of the distances.  The bars are 4 times these, the margin being for other seeds — the kernels
  themselves are deterministic."""

import math

import numpy as np
import pytest
import torch

from tests import center_cases as cc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR_B = cc.BAR_B  # 4 x the worst measured relative error of each rule (see the module docstring)


@pytest.fixture(scope="module")
def bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


def _stack(case, attack):
  """(device rows: honest tensors + k references to ONE Byzantine tensor, host rows as a list with the same aliasing,
  the honest rows the reference iterates on — all n rows unless the attack is `nan`)."""
  rows, start = cc.make_rows(case)
  h = case.n - case.k
  byz = np.full(case.d, np.nan, dtype=np.float32) if attack == "nan" else rows[-1].copy()
  host = [rows[i].copy() for i in range(h)] + [byz] * case.k
  byz_dev = torch.from_numpy(byz).to(DEV)
  dev = [torch.from_numpy(r).to(DEV) for r in host[:h]] + [byz_dev] * case.k
  ref_rows = rows[:h] if attack == "nan" else rows
  return dev, host, ref_rows, start


CASES = [(case, case.attack) for case in cc.cases()] + [(case, "nan") for case in cc.cases()[::4]]


def _id(item):
  case, attack = item
  return f"n{case.n}-k{case.k}-{attack}"


@pytest.mark.parametrize("mode", ["geomed", "cclip"])
@pytest.mark.parametrize("item", CASES, ids=_id)
def test_rules_end_to_end(bm, item, mode):
  case, attack = item
  lib = bm._lib.load()
  dev, host, ref_rows, start = _stack(case, attack)
  param, iters = cc.params(case, mode)
  start_dev = torch.from_numpy(start).to(DEV)
  if mode == "geomed":
    out = bm.gars.geomed(dev, case.k, nu=param, iters=iters)
    points_dev, points_host = dev, host
  else:
    out = bm.gars.cclip(dev, case.k, tau=param, iters=iters, start=start_dev)
    points_dev, points_host = dev + [start_dev], host + [start]
  got = out.cpu().double().numpy()
  assert out.dtype == torch.float32 and got.shape == (case.d,) and np.isfinite(got).all()
  assert all(out.data_ptr() != t.data_ptr() for t in points_dev)       # never an alias of an input
  # (a) composition: the host form on the device's own matrix gives the device's weights, bit for bit, and the output
  # is their weighted sum within the kernel's bound
  sq_dev = bm.gars.pairwise_sqdist(points_dev)
  weights_dev, info = bm.gars.center_weights(sq_dev, case.n, mode, param, iters, 0.0, mode == "cclip")
  sq = sq_dev.cpu().numpy()
  code, weights, host_info = cc.host_weights(lib, sq, case.n, mode, param, iters, has_start=mode == "cclip")
  assert code == 0 and np.array_equal(weights_dev.cpu().numpy().view(np.uint64), weights.view(np.uint64))
  assert np.array_equal(info.cpu().numpy(), host_info)
  usable = case.n - case.k if attack == "nan" else case.n
  assert host_info[0] == iters and host_info[2] == usable
  if attack == "nan":
    assert not weights[usable:case.n].any()
  clean = [np.zeros(case.d, dtype=np.float32) if (w == 0 and np.isnan(p).any()) else p
           for p, w in zip(points_host, weights)]
  want, bound = cc.weighted_sum_reference(_realias(points_host, clean), list(weights[:len(points_host)]))
  excess = np.abs(got - want) - bound
  assert excess.max() <= 0, (_id(item), mode, float(excess.max()))
  # (b) against the definition on the vectors, in float64
  ref, _ = cc.vector_iteration(ref_rows, mode, param, iters, start=start if mode == "cclip" else None)
  err = cc.relative_error(got, ref)
  print(f"center_error {mode} {_id(item)} {err:.3e}")
  assert err <= BAR_B[mode], (_id(item), mode, err)


def _realias(original, cleaned):
  """`cleaned` with the aliasing of `original`: entries that were one object are one object again."""
  first = {}
  out = []
  for o, c in zip(original, cleaned):
    out.append(first.setdefault(id(o), c))
  return out


@pytest.mark.parametrize("mode", ["geomed", "cclip"])
def test_graphed_call_replays_on_changed_rows(bm, mode):
  from byzantinemomentum_amd.graphs import GraphedCall
  from byzantinemomentum_amd.sharded import ShardedAggregator
  case = cc.cases()[4]  # n = 25, k = 5
  dev, _, _, start = _stack(case, case.attack)
  start_dev = torch.from_numpy(start).to(DEV)
  agg = ShardedAggregator(local_only=True)
  param, iters = cc.params(case, mode)
  if mode == "geomed":
    call = lambda: agg.geomed(dev, case.k, nu=param, iters=iters)  # noqa: E731
  else:
    call = lambda: agg.cclip(dev, case.k, tau=param, iters=iters, start=start_dev)  # noqa: E731
  graphed = GraphedCall(call)
  recorded_weights = agg.last_weights     # the tensor of the recording: every replay writes it again
  assert torch.equal(graphed(), call())
  gen = torch.Generator(device=DEV).manual_seed(9)
  for round_ in range(2):   # new contents at the recorded addresses
    for t in dev[:case.n - case.k]:
      t.add_(0.3 * torch.randn(case.d, device=DEV, generator=gen))
    dev[-1].mul_(-0.5)
    start_dev.add_(0.01)
    replayed = graphed().clone()
    weights = recorded_weights.clone()
    eager = call()
    assert torch.equal(replayed, eager), (mode, round_)
    assert torch.equal(weights, agg.last_weights)


def test_sharded_aggregator_on_the_gpu_equals_the_package_rule(bm):
  from byzantinemomentum_amd.sharded import ShardedAggregator
  case = cc.cases()[0]
  dev, _, _, start = _stack(case, case.attack)
  start_dev = torch.from_numpy(start).to(DEV)
  agg = ShardedAggregator(local_only=True)
  assert torch.equal(agg.geomed(dev, case.k), bm.geomed(dev, case.k))
  assert agg.last_weights.is_cuda and agg.last_weights.shape == (64,)
  tau = math.sqrt(case.d)
  assert torch.equal(agg.cclip(dev, case.k, tau=tau, start=start_dev), bm.cclip(dev, case.k, tau=tau, start=start_dev))
  assert torch.equal(agg.cclip(dev, case.k, tau=tau), bm.cclip(dev, case.k, tau=tau))
  with pytest.raises(ValueError):
    bm.cclip(dev, case.k)
  with pytest.raises(bm.gars.GarInputError):
    bm.geomed(dev * 6, case.k)               # 66 rows
