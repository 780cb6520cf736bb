"""CAF and DnC on the GPU (distance pass -> bm_spectral_weights_device -> weighted sum), on the cases of
tests/spectral_cases.py.  Needs an MI355X: `pytest -m gpu`.
  (a) the device form of the weights against the host form, BIT FOR BIT (weights and info): on the exact matrices of
      every case at T = 1, 16, 32, on the crafted matrices of test_spectral_cpu.py, and on the matrices the device's own
      distance pass produced;
  (b) end to end against the float64 rules on the vectors at T = 16, as |out - ref| / |ref| of the output VECTOR (a tie
      between identical rows does not matter there).  The reference reports how far each of its decisions was from going
      the other way; a case decided by less than spectral_cases.MIN_MARGIN would say nothing — none of the committed
      cases is (smallest margins: 3.1e-4 of n for the mass check, 1.7e-2 between the two smallest lambda, 0.27 of the
      largest tau at the DnC boundary).  The bar is spectral_cases.BAR_B, 4 x the worst error measured on an MI355X
      (profiles/spectral_errors.txt);
  (c) the rows of the `nan` attack get no weight and the output is the rule on the other rows;
  (d) a GraphedCall of either rule records, replays on changed rows and equals the direct call bit for bit;
  (e) nnm(rule="caf") on the rows path is caf(nnm_rows(...)); (f) ShardedAggregator.caf / .dnc equal gars.caf / .dnc;
  (g) three steps of AggregationStep(gar="caf" | "dnc") against the oracle-backed step, within the bar of (b)."""

import functools
import math

import numpy as np
import pytest
import torch

from tests import spectral_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T = sc.T_END_TO_END


@pytest.fixture(scope="module")
def bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


@functools.lru_cache(maxsize=None)
def _reference(case, mode, nan_rows=False):
  rows, _ = sc.make_rows(case)
  if nan_rows:
    rows = rows.copy()
    rows[case.n - case.k:] = np.nan
  return sc.vector_spectral(rows, mode, sc.count_of(case, mode), T)


def _stack(case, nan_rows=False):
  """Device rows: the honest tensors + k references to ONE Byzantine tensor (NaN everywhere for the `nan` attack)."""
  rows, _ = sc.make_rows(case)
  h = case.n - case.k
  byz = np.full(case.d, np.nan, dtype=np.float32) if nan_rows else rows[-1].copy()
  byz_dev = torch.from_numpy(byz).to(DEV)
  return [torch.from_numpy(rows[i].copy()).to(DEV) for i in range(h)] + [byz_dev] * case.k


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(bm, sq, n, mode, count, power_iters, tag):
  """The device form on `sq` (a float64 numpy matrix, uploaded) against the host form: weights and info, bit for bit."""
  lib = bm._lib.load()
  code, want, want_info = sc.host_weights(lib, sq, n, mode, count, power_iters)
  sq_dev = torch.from_numpy(np.ascontiguousarray(sq, dtype=np.float64)).to(DEV)
  got, got_info = bm.gars.spectral_weights(sq_dev, n, mode, count, power_iters)
  assert code == 0 and got.is_cuda and got.shape == (64,) and got_info.shape == (4,)
  assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (tag, got.cpu().numpy()[:n], want[:n])
  assert np.array_equal(_bits(got_info.cpu().numpy()), _bits(want_info)), (tag, got_info.cpu().numpy(), want_info)
  return want, want_info


# ---------------------------------------------------------------------------- #
# (a)

@pytest.mark.parametrize("mode", ["caf", "dnc"])
@pytest.mark.parametrize("case", sc.cases(), ids=sc.case_id)
def test_device_weights_equal_host_weights_on_exact_matrices(bm, case, mode):
  rows, _ = sc.make_rows(case)
  sq = sc.exact_sqdist(rows)
  for power_iters in sc.POWER_ITERS:
    _same_bits(bm, sq, case.n, mode, sc.count_of(case, mode), power_iters, (sc.case_id(case), mode, power_iters))


@pytest.mark.parametrize("item", sc.crafted(), ids=lambda item: item[0])
def test_device_weights_equal_host_weights_on_crafted_matrices(bm, item):
  name, sq, n, mode, count = item
  for power_iters in (1, 16):
    _same_bits(bm, sq, n, mode, count, power_iters, (name, power_iters))


@pytest.mark.parametrize("nan_rows", [False, True], ids=["plain", "nan"])
@pytest.mark.parametrize("case", sc.cases()[::3], ids=sc.case_id)
def test_device_weights_equal_host_weights_on_the_device_s_own_matrix(bm, case, nan_rows):
  sq = bm.gars.pairwise_sqdist(_stack(case, nan_rows)).cpu().numpy().reshape(-1)[:case.n * case.n].reshape(case.n, case.n)
  for mode in ("caf", "dnc"):
    _, info = _same_bits(bm, sq, case.n, mode, sc.count_of(case, mode), T, (sc.case_id(case), mode, nan_rows))
    assert info[2] == (case.n - case.k if nan_rows else case.n)


def test_one_lane_form_on_the_device_equals_its_host_form(bm):
  """BM_SPECTRAL_LANES = 1, the other side of the A/B in profiles/spectral_timings.txt: host and device switch together."""
  lib = bm._lib.load()
  case = sc.cases()[9]
  sq = sc.exact_sqdist(sc.make_rows(case)[0])
  assert lib.bm_tuning_set(b"BM_SPECTRAL_LANES", 1) == 0
  try:
    for mode in ("caf", "dnc"):
      _same_bits(bm, sq, case.n, mode, case.k, T, ("one lane", mode))
  finally:
    assert lib.bm_tuning_set(b"BM_SPECTRAL_LANES", 0) == 0


# ---------------------------------------------------------------------------- #
# (b), (c)

def test_no_committed_case_is_left_out():
  for case in sc.cases():
    for mode in ("caf", "dnc"):
      for nan_rows in (False, True):
        margins = _reference(case, mode, nan_rows).margins
        assert min(margins.values()) >= sc.MIN_MARGIN, (sc.case_id(case), mode, nan_rows, margins)


@pytest.mark.parametrize("mode", ["caf", "dnc"])
@pytest.mark.parametrize("case", sc.cases(), ids=sc.case_id)
def test_rules_end_to_end(bm, case, mode):
  dev = _stack(case)
  ref = _reference(case, mode)
  assert min(ref.margins.values()) >= sc.MIN_MARGIN
  out = bm.caf(dev, case.k, power_iters=T) if mode == "caf" else bm.dnc(dev, case.k, c=1.0, power_iters=T)
  got = out.cpu().double().numpy()
  assert out.dtype == torch.float32 and got.shape == (case.d,) and np.isfinite(got).all()
  assert all(out.data_ptr() != t.data_ptr() for t in dev)       # never an alias of an input
  weights, info = out.spectral_weights.cpu().numpy(), out.spectral_info.cpu().numpy()
  assert out.spectral_weights.is_cuda and weights.shape == (64,) and info.shape == (4,)
  assert info[0] == ref.rounds and info[3] == ref.kept and info[2] == case.n
  assert abs(weights.sum() - 1.0) <= 1e-12 and not weights[case.n:].any()
  err = sc.relative_error(got, ref.out)
  print(f"spectral_error {mode} {sc.case_id(case)} {err:.3e}")
  assert err <= sc.BAR_B[mode], (sc.case_id(case), mode, err)


@pytest.mark.parametrize("mode", ["caf", "dnc"])
@pytest.mark.parametrize("case", sc.cases()[::4], ids=sc.case_id)
def test_nan_rows_get_no_weight(bm, case, mode):
  dev = _stack(case, nan_rows=True)
  h = case.n - case.k
  ref = _reference(case, mode, True)
  out = bm.caf(dev, case.k, power_iters=T) if mode == "caf" else bm.dnc(dev, case.k, power_iters=T)
  got = out.cpu().double().numpy()
  weights, info = out.spectral_weights.cpu().numpy(), out.spectral_info.cpu().numpy()
  assert np.isfinite(got).all() and not weights[h:].any() and info[2] == h
  assert info[0] == ref.rounds and info[3] == ref.kept
  err = sc.relative_error(got, ref.out)
  print(f"spectral_error {mode} {sc.case_id(case)}-nan {err:.3e}")
  assert err <= sc.BAR_B[mode], (sc.case_id(case), mode, err)
  if mode == "dnc":   # k' = k - (n - U) = 0: the mean of the other rows
    mean = sc.make_rows(case)[0][:h].astype(np.float64).mean(axis=0)
    assert np.array_equal(weights[:h], np.full(h, 1.0 / h)) and sc.relative_error(got, mean) <= sc.BAR_B[mode]


# ---------------------------------------------------------------------------- #
# (d), (e), (f)

@pytest.mark.parametrize("mode", ["caf", "dnc"])
def test_graphed_call_replays_on_changed_rows(bm, mode):
  from byzantinemomentum_amd.graphs import GraphedCall
  from byzantinemomentum_amd.sharded import ShardedAggregator
  case = sc.cases()[4]  # n = 25, k = 5
  dev = _stack(case)
  agg = ShardedAggregator(local_only=True)
  call = lambda: getattr(agg, mode)(dev, case.k, power_iters=T)  # noqa: E731
  graphed = GraphedCall(call)
  recorded_weights = agg.last_weights     # the tensor of the recording: every replay writes it again
  assert torch.equal(graphed(), call())
  gen = torch.Generator(device=DEV).manual_seed(9)
  for round_ in range(2):   # new contents at the recorded addresses
    for t in dev[:case.n - case.k]:
      t.add_(0.3 * torch.randn(case.d, device=DEV, generator=gen))
    dev[-1].mul_(-0.5)
    replayed = graphed().clone()
    weights = recorded_weights.clone()
    eager = call()
    assert torch.equal(replayed, eager), (mode, round_)
    assert torch.equal(weights, agg.last_weights)


def test_nnm_on_the_rows_path_runs_the_rule_on_the_mixed_rows(bm):
  case = sc.cases()[4]
  dev = _stack(case)
  for mode, args in (("caf", dict(power_iters=T)), ("dnc", dict(c=1.0, power_iters=T))):
    direct = getattr(bm, mode)(bm.gars.nnm_rows(dev, case.k), case.k, **args)
    assert torch.equal(bm.nnm(dev, case.k, rule=mode, **args), direct)
  means = bm.bucketing(dev, 2, "caf", perm=list(range(case.n)), f=3)
  masks = bm.gars._masks_tensor(bm.gars.bucket_masks(case.n, 2, list(range(case.n))), torch.device(DEV))
  assert torch.equal(means, bm.caf(bm.gars.mix_rows(dev, masks, 13), 3))


def test_sharded_aggregator_on_the_gpu_equals_the_package_rule(bm):
  from byzantinemomentum_amd.sharded import ShardedAggregator
  case = sc.cases()[0]
  dev = _stack(case)
  agg = ShardedAggregator(local_only=True)
  want = bm.caf(dev, case.k)
  assert torch.equal(agg.caf(dev, case.k), want)
  assert agg.last_weights.is_cuda and torch.equal(agg.last_weights, want.spectral_weights)
  assert torch.equal(agg.last_spectral_info, want.spectral_info)
  assert torch.equal(agg.dnc(dev, case.k, c=1.5), bm.dnc(dev, case.k, c=1.5))
  assert int((agg.last_weights[:case.n] == 0).sum()) == 3
  with pytest.raises(ValueError):
    bm.caf(dev, 6)                            # 2 f >= n
  with pytest.raises(bm.gars.GarInputError):
    bm.caf(dev * 6, 1)                        # 66 rows


# ---------------------------------------------------------------------------- #
# (g)

D = 4099


def _norm_error(got, want):
  return float((got.cpu().double() - want.double()).norm() / want.double().norm())


@pytest.mark.parametrize("attack", ["empire", "nan"])
@pytest.mark.parametrize("gar,gar_args", [("caf", dict(power_iters=T)), ("dnc", dict(c=1.0, power_iters=T))])
def test_step_matches_the_oracle_backed_step(gar, gar_args, attack):
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from byzantinemomentum_amd.step import AggregationStep
  from tests.attack_vectors_reference import sampled_for_step
  from tests.sharded_backend import OracleBackend
  n, f = 11, 2
  common = dict(gar=gar, gar_args=gar_args, momentum=0.9, dampening=0.9, momentum_at="worker", attack=attack,
                attack_factor=1.1, nb_past=3)
  hip = AggregationStep(n, f, f, aggregator=ShardedAggregator(local_only=True), **common)
  oracle = AggregationStep(n, f, f, aggregator=ShardedAggregator(backend=OracleBackend(), local_only=True), **common)
  assert hip.plan.first_pass == "plain" and hip.plan.search is None and hip.plan.accept is None
  assert not hip.single_call
  gen = torch.Generator().manual_seed(5)
  origin = torch.randn(D, generator=gen)
  params = origin.clone()
  for it in range(3):
    tag = f"{gar} {attack} step{it}"
    sampled = sampled_for_step(it, n - f, D)
    want = oracle.run([g.clone() for g in sampled], params, origin)
    got = hip.run([g.to(DEV) for g in sampled], params.to(DEV), origin.to(DEV))
    assert torch.isfinite(got).all()   # the NaN rows of the `nan` attack never reach the output
    # the two steps made the same decisions: the comparison of the vectors says something
    assert hip.agg.last_spectral_info.cpu().tolist()[0::3] == oracle.agg.last_spectral_info.tolist()[0::3], tag
    err = _norm_error(got, want)
    upd_want = oracle.update_gradient()
    upd_err = _norm_error(hip.update_gradient(), upd_want)
    print(f"spectral_step_error {tag} defense {err:.3e} update {upd_err:.3e}")
    assert err <= sc.BAR_B[gar], (tag, err)
    assert upd_err <= sc.BAR_B[gar], (tag, upd_err)
    assert math.isnan(hip.floats()["accept_ratio"])
    params = params - 0.05 * upd_want
