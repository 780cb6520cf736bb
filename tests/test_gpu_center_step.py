"""AggregationStep(gar="geomed" | "cclip") with the HIP backend against the same step on the oracle-backed legs
(tests/sharded_backend.OracleBackend: the rules in plain float64 torch), three steps, worker and update placements,
the `empire` and `nan` attacks, n = 11 / f = 2 and n = 25 / f = 5 at d = 4099.  Needs an MI355X: `pytest -m gpu`.

The defense vector and the update are held to the bar of tests/test_gpu_center_rules.py (b), center_cases.BAR_B, by
the same measure (relative error in norm); measured here 1.8e-7 at worst.  The study row `floats()` is held to
center_cases.FLOATS_BAR, 4 x the worst error measured over every quantity, step and case
(profiles/center_errors.txt lists the worst of each quantity)."""

import math

import pytest
import torch

from tests import center_cases as cc
from tests.attack_vectors_reference import sampled_for_step

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = 4099
GAR_ARGS = {"geomed": dict(nu=1e-6 * math.sqrt(D), iters=8), "cclip": dict(tau=2.0, iters=3)}


def _steps(gar, n, f, placement, attack, evals=None):
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from byzantinemomentum_amd.step import AggregationStep
  from tests.sharded_backend import OracleBackend
  common = dict(gar=gar, gar_args=GAR_ARGS[gar], momentum=0.9, dampening=0.9, momentum_at=placement, attack=attack,
                attack_factor=1.1, nb_past=3, attack_evals=evals)
  hip = AggregationStep(n, f, f, aggregator=ShardedAggregator(local_only=True), **common)
  oracle = AggregationStep(n, f, f, aggregator=ShardedAggregator(backend=OracleBackend(), local_only=True), **common)
  return hip, oracle


def _norm_error(got, want):
  return float((got.cpu().double() - want.double()).norm() / want.double().norm())


@pytest.mark.parametrize("attack", ["empire", "nan"])
@pytest.mark.parametrize("placement", ["worker", "update"])
@pytest.mark.parametrize("n,f", [(11, 2), (25, 5)])
@pytest.mark.parametrize("gar", ["geomed", "cclip"])
def test_step_matches_the_oracle_backed_step(gar, n, f, placement, attack):
  hip, oracle = _steps(gar, n, f, placement, attack)
  assert hip.plan.first_pass == "plain" and hip.plan.search is None and hip.plan.accept is None
  assert not hip.single_call
  gen = torch.Generator().manual_seed(5)
  origin = torch.randn(D, generator=gen)
  params = origin.clone()
  previous = None
  worst = {}
  for it in range(3):
    tag = f"{gar} n{n} {placement} {attack} step{it}"
    sampled = sampled_for_step(it, n - f, D)
    want = oracle.run([g.clone() for g in sampled], params, origin)
    got = hip.run([g.to(DEV) for g in sampled], params.to(DEV), origin.to(DEV))
    assert torch.isfinite(got).all()   # the NaN rows of the `nan` attack never reach the output
    err = _norm_error(got, want)
    upd_want = oracle.update_gradient()
    upd_err = _norm_error(hip.update_gradient(), upd_want)
    print(f"center_step_error {tag} defense {err:.3e} update {upd_err:.3e}")
    assert err <= cc.BAR_B[gar], (tag, err)
    assert upd_err <= cc.BAR_B[gar], (tag, upd_err)
    floats, floats_want = hip.floats(), oracle.floats()
    for key, value in cc.float_errors(floats, floats_want).items():
      worst[key] = max(worst.get(key, 0.0), value)
    assert math.isnan(floats["accept_ratio"])
    if gar == "cclip":
      assert hip.cclip_start is got and (previous is None or hip.cclip_start is not previous)
      # the start carried weight from the second step on: it was handed to the rule
      assert (float(hip.agg.last_weights[n]) != 0.0) == (it > 0)
    else:
      assert hip.cclip_start is None
    previous = got
    params = params - 0.05 * upd_want
  for key, value in sorted(worst.items()):
    print(f"center_floats_error {gar} n{n} {placement} {attack} {key} {value:.3e}")
  over = {key: value for key, value in worst.items() if not value <= cc.FLOATS_BAR}
  assert not over, (gar, n, placement, attack, over)


@pytest.mark.parametrize("gar", ["geomed", "cclip"])
def test_factor_search_against_the_rules_runs_the_generic_form(gar):
  hip, _ = _steps(gar, 11, 2, "worker", "empire", evals=4)
  assert hip.plan.search == "generic"
  for it in range(2):
    before = hip.cclip_start
    out = hip.run([g.to(DEV) for g in sampled_for_step(it, 9, D)])
    assert len(hip.last_search) == 4 and torch.isfinite(out).all()
    if gar == "cclip":
      assert hip.cclip_start is out and hip.cclip_start is not before
