"""The Min-Max / Min-Sum attacks without a GPU: the closed form of include/bm_gar.h against the paper's halving search on
the vectors (float64 numpy, tests/minmax_reference.py), the HOST form bm_minmax_factor on exact scalars, tightness of the
returned factor, the degenerate inputs, every refused argument, the plain-torch legs of ShardedAggregator.minmax and
AggregationStep(attack="minmax" | "minsum") on the oracle-backed backend, and the new exports.  (Two gloo ranks:
tests/test_minmax_gloo.py.)"""

import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import gar_oracle as O
from tests import minmax_reference as R

HS = (2, 5, 11, 20, 39, 64)
DS = (7, 67, 259, 1027)


def host_factor(D, scal, h, mode):
  from byzantinemomentum_amd import stats
  out = stats.minmax_factor(torch.from_numpy(np.ascontiguousarray(D, dtype=np.float64)),
                            torch.from_numpy(np.ascontiguousarray(scal, dtype=np.float64)), h, mode)
  return out.tolist()


# ---------------------------------------------------------------------------- #
# 1. the closed form is the limit of the paper's search

@pytest.mark.parametrize("h", HS)
@pytest.mark.parametrize("d", DS)
def test_closed_form_equals_the_papers_search(h, d):
  worst = 0.0
  for structure in R.STRUCTURES:
    rows = R.stack(h, d, structure, seed=1)
    for perturbation in R.PERTURBATIONS:
      for mode in R.MODES:
        res = R.attack(rows, perturbation, mode)
        assert not res["degenerate"] and res["gamma"] > 0.0, (structure, perturbation, mode)
        found = R.paper_search(rows, res["avg"], res["p"], mode, init=max(10.0, 4.0 * res["gamma"]), tau=1e-9)
        err = abs(found - res["gamma"]) / res["gamma"]
        worst = max(worst, err)
        assert err <= 1e-8, (structure, perturbation, mode, found, res["gamma"])
  print(f"h = {h}, d = {d}: search against closed form, worst relative difference {worst:.2e}")


# ---------------------------------------------------------------------------- #
# 2. / 3. the host form on exact float64 scalars, and tightness of what it returns

def _separated(h, d, structure, perturbation):
  """The first seed whose two smallest gamma_i differ by more than 1e-3 relative: (rows, reference result)."""
  for seed in range(64):
    rows = R.stack(h, d, structure, seed)
    res = R.attack(rows, perturbation, "minmax")
    two = np.sort(res["gammas"])[:2]
    if two[1] - two[0] > 1e-3 * two[1]:
      return rows, res
  raise AssertionError("no seed separates the two smallest factors")


@pytest.mark.parametrize("h", HS)
@pytest.mark.parametrize("perturbation", R.PERTURBATIONS)
def test_host_form_on_exact_scalars(h, perturbation):
  for d in (7, 259):
    for structure in R.STRUCTURES:
      rows, ref = _separated(h, d, structure, perturbation)
      two = np.sort(ref["gammas"])[:2]
      assert two[1] - two[0] > 1e-3 * two[1]
      D, scal = R.distances(rows), R.scalars(rows, ref["avg"], ref["p"])
      for mode in R.MODES:
        want = R.closed_form(D, scal, h, mode)
        gamma, bound, binding, P, N, degenerate = host_factor(D, scal, h, mode)
        assert degenerate == 0.0 and gamma > 0.0
        assert abs(gamma - want["gamma"]) <= 1e-12 * want["gamma"], (d, structure, mode, gamma, want["gamma"])
        assert abs(bound - want["bound"]) <= 1e-12 * want["bound"]
        assert binding == want["binding"] and P == scal[64] and N == scal[65]
        # tightness, in float64 on the vectors, from the factor the library returned
        value, limit = R.objective(rows, ref["avg"] + gamma * ref["p"], mode)
        assert value <= limit * (1 + 1e-9), (d, structure, mode, value, limit)
        beyond, _ = R.objective(rows, ref["avg"] + gamma * (1 + 1e-6) * ref["p"], mode)
        assert beyond > limit, (d, structure, mode, beyond, limit)


# ---------------------------------------------------------------------------- #
# 4. degenerate inputs and refused arguments

def _degenerate_cases():
  rng = np.random.default_rng(7)
  base = rng.standard_normal((5, 16))
  equal = np.repeat(base[:1], 5, axis=0)
  nan_row = base.copy()
  nan_row[2, 3] = math.nan
  return {"equal_unit": (equal, "unit"), "equal_std": (equal, "std"), "nan_row": (nan_row, "std"),
          "two_rows": (base[:2], "std"), "two_equal_rows": (equal[:2], "sign")}


@pytest.mark.parametrize("name", ["equal_unit", "equal_std", "nan_row", "two_rows", "two_equal_rows"])
@pytest.mark.parametrize("mode", R.MODES)
def test_degenerate_inputs_follow_the_definition(name, mode):
  rows, perturbation = _degenerate_cases()[name]
  h = len(rows)
  # (equal rows: their average is the row itself — numpy's mean of five equal numbers need not be, by a rounding)
  ref = R.attack(rows, perturbation, mode, avg=rows[0] if "equal" in name else None)
  got = host_factor(R.distances(rows), R.scalars(rows, ref["avg"], ref["p"]), h, mode)
  assert bool(got[5]) is ref["degenerate"], (name, got)
  expected = {"equal_unit": False, "equal_std": True, "nan_row": True, "two_rows": False, "two_equal_rows": False}[name]
  assert ref["degenerate"] is expected
  if ref["degenerate"]:
    assert got[0] == 0.0 and math.copysign(1.0, got[0]) == 1.0 and got[2] == -1.0
  else:
    assert abs(got[0] - ref["gamma"]) <= 1e-12 * max(ref["gamma"], 1e-300)
  if name.startswith("equal") or name == "two_equal_rows":
    assert got[0] == 0.0  # all rows equal: the largest admissible factor is 0 whether or not the flag is set


@pytest.mark.parametrize("mode", R.MODES)
def test_degenerate_scalars(mode):
  rows = R.stack(6, 19, "iid", 3)
  avg = rows.mean(axis=0)
  D = R.distances(rows)
  good = R.scalars(rows, avg, -avg)
  assert host_factor(D, good, 6, mode)[5] == 0.0
  # avg = 0 with "unit", a zero-variance stack with "std": P = 0
  zero_p = good.copy()
  zero_p[:6], zero_p[64] = 0.0, 0.0
  # an infinite entry of D; a NaN scalar; a negative discriminant cannot come from real rows: P > 0 with a bound below a_i
  inf_D = D.copy()
  inf_D[1, 4] = inf_D[4, 1] = math.inf
  nan_b = good.copy()
  nan_b[2] = math.nan
  inf_P = good.copy()
  inf_P[64] = math.inf
  neg_P = good.copy()
  neg_P[64] = -1.0
  for D_, scal in ((D, zero_p), (inf_D, good), (D, nan_b), (D, inf_P), (D, neg_P)):
    got = host_factor(D_, scal, 6, mode)
    assert got[5] == 1.0 and got[0] == 0.0 and math.copysign(1.0, got[0]) == 1.0 and got[2] == -1.0, got
    assert R.closed_form(D_, scal, 6, mode)["degenerate"]
  shrunk = D * 1e-6  # distances too small for these b_i: b^2 + P (R - a) stays >= 0 (b^2 dominates): not degenerate
  assert host_factor(shrunk, good, 6, mode)[5] == 0.0


def test_every_refused_argument_is_refused_before_any_launch():
  from byzantinemomentum_amd import _lib, gars, stats
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from byzantinemomentum_amd.step import AggregationStep
  from tests.sharded_backend import OracleBackend
  lib = _lib.load()
  buf = (ctypes.c_double * (64 * 64))()
  scal = (ctypes.c_double * _lib.PERTURB_SLOTS)()
  out = (ctypes.c_double * 6)()
  for fn, tail in ((lib.bm_minmax_factor, ()), (lib.bm_minmax_factor_device, (None,))):
    assert fn(None, scal, 5, 0, out, *tail) == _lib.EINVAL
    assert fn(buf, None, 5, 0, out, *tail) == _lib.EINVAL
    assert fn(buf, scal, 5, 0, None, *tail) == _lib.EINVAL
    assert fn(buf, scal, 1, 0, out, *tail) == _lib.EINVAL
    assert fn(buf, scal, 65, 0, out, *tail) == _lib.EINVAL
    assert fn(buf, scal, 5, 2, out, *tail) == _lib.EINVAL
    assert fn(buf, scal, 5, -1, out, *tail) == _lib.EINVAL
  assert lib.bm_minmax_factor(buf, scal, 2, 1, out) == 0
  # bm_perturb_stats: host arrays stand in for device memory, every call below returns before a launch
  d = 32
  data = (ctypes.c_float * (8 * d))()
  at = lambda i: ctypes.cast(ctypes.byref(data, 4 * d * i), ctypes.c_void_p)  # noqa: E731
  rows = (ctypes.c_void_p * 64)()
  for i in range(4):
    rows[i] = at(i).value
  avg, dirv, ws = at(5), at(6), buf
  ok = (rows, 4, d, 1, avg, dirv, scal, ws, None)

  def call(**change):
    names = ("rows", "h", "d", "kind", "avg", "dir", "scal", "ws", "stream")
    args = dict(zip(names, ok))
    args.update(change)
    return lib.bm_perturb_stats(*[args[k] for k in names])
  assert call(rows=None) == _lib.EINVAL and call(scal=None) == _lib.EINVAL and call(ws=None) == _lib.EINVAL
  assert call(avg=None) == _lib.EINVAL and call(dir=None) == _lib.EINVAL
  assert call(h=1) == _lib.EINVAL and call(h=65) == _lib.EINVAL and call(h=5) == _lib.EINVAL  # (h = 5: a null row)
  assert call(kind=3) == _lib.EINVAL and call(kind=-1) == _lib.EINVAL and call(d=-1) == _lib.EINVAL
  assert call(dir=avg) == _lib.EINVAL                                           # the outputs are one buffer
  assert call(dir=ctypes.cast(ctypes.byref(data, 4 * d * 5 + 4), ctypes.c_void_p)) == _lib.EINVAL   # ... or overlap
  assert call(avg=at(2)) == _lib.EINVAL and call(dir=at(0)) == _lib.EINVAL       # an output is a row
  assert call(avg=ctypes.cast(ctypes.byref(data, 4 * d * 3 + 4 * (d - 1)), ctypes.c_void_p), dir=at(7)) == _lib.EINVAL
  assert lib.bm_perturb_workspace_bytes(-1) == _lib.EINVAL
  assert lib.bm_perturb_workspace_bytes(0) == lib.bm_perturb_workspace_bytes(1 << 29) > 0
  assert lib.bm_perturb_workspace_bytes((1 << 29) + 1) == 2 * lib.bm_perturb_workspace_bytes(1)
  assert lib.bm_tuning_set(b"BM_PERTURB_GRID", 0) == 0
  # Python: by name, before a tensor is looked at
  one = [torch.zeros(8)]
  for fn in (stats.minmax_attack, stats.minsum_attack):
    with pytest.raises(ValueError, match="perturbation"):
      fn(one * 3, 1, perturbation="l2")
    with pytest.raises(gars.GarInputError, match="2 <= h"):
      fn(one, 1)
  with pytest.raises(ValueError, match="perturbation"):
    stats.perturb_stats(one * 3, "variance")
  with pytest.raises(gars.GarInputError, match="2 <= h"):
    stats.perturb_stats(one, "std")
  sq, sc = torch.zeros(4, 4, dtype=torch.float64), torch.zeros(_lib.PERTURB_SLOTS, dtype=torch.float64)
  with pytest.raises(ValueError, match="mode"):
    stats.minmax_factor(sq, sc, 4, "maxmin")
  with pytest.raises(gars.GarInputError):
    stats.minmax_factor(sq, sc, 1, "minmax")
  with pytest.raises(gars.GarInputError):
    stats.minmax_factor(sq, sc, 5, "minmax")            # the matrix is too small
  with pytest.raises(gars.GarInputError):
    stats.minmax_factor(sq, sc[:10], 4, "minmax")       # ... the scalars are
  with pytest.raises(gars.GarInputError):
    stats.minmax_factor(sq.float(), sc, 4, "minmax")
  agg = ShardedAggregator(backend=OracleBackend())
  rows8 = [torch.randn(8) for _ in range(3)]
  with pytest.raises(ValueError, match="mode"):
    agg.minmax(rows8, 1, "maxmin")
  with pytest.raises(ValueError, match="perturbation"):
    agg.minmax(rows8, 1, "minmax", "l2")
  with pytest.raises(ValueError, match="2 <= h"):
    agg.minmax(rows8[:1], 1)
  assert agg.minmax(rows8, 0) == [] and agg.minmax(rows8, -1, "minsum", "unit") == []
  for attack in ("minmax", "minsum"):
    with pytest.raises(ValueError, match="attack_evals must be None"):
      AggregationStep(11, 2, 2, attack=attack, attack_evals=4, aggregator=agg)
    with pytest.raises(ValueError, match="perturbation"):
      AggregationStep(11, 2, 2, attack=attack, attack_args={"perturbation": "l2"}, aggregator=agg)
    with pytest.raises(ValueError, match="attack_args"):
      AggregationStep(11, 2, 2, attack=attack, attack_args={"target_idx": 3}, aggregator=agg)
    with pytest.raises(ValueError, match="at least 2 honest"):
      AggregationStep(3, 1, 2, attack=attack, aggregator=agg)
    AggregationStep(11, 2, 2, attack=attack, attack_factor="ignored", attack_args={"perturbation": "sign"}, aggregator=agg)
    AggregationStep(11, 2, 2, attack=attack, attack_args={}, aggregator=agg)


# ---------------------------------------------------------------------------- #
# 5. the plain-torch legs and the step, on the oracle-backed backend

def _rows32(h, d, structure, seed):
  return [torch.from_numpy(r.astype(np.float32)) for r in R.stack(h, d, structure, seed)]


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("perturbation", R.PERTURBATIONS)
def test_torch_legs_against_the_float64_reference(mode, perturbation):
  from byzantinemomentum_amd import sharded, torch_legs
  from tests.sharded_backend import OracleBackend
  for h, d, structure in ((2, 9, "iid"), (9, 130, "common"), (20, 67, "scaled")):
    rows = _rows32(h, d, structure, 5)
    kept = [g.clone() for g in rows]
    agg = sharded.ShardedAggregator(backend=OracleBackend())
    res = agg.minmax(rows, 3, mode, perturbation)
    assert len(res) == 3 and all(r is res[0] for r in res) and all(res[0] is not g for g in rows)
    assert all(torch.equal(a, b) for a, b in zip(kept, rows))
    byz = res[0]
    avg, direction, scal = torch_legs._perturb_stats_torch(agg.backend, rows, perturbation)
    rows64 = np.stack([g.double().numpy() for g in rows])
    assert np.array_equal(avg.numpy(), R.seq_mean32(rows64.astype(np.float32)))
    # the legs' own fp32 average and direction, upcast: only fp64 rounding is left
    own = R.attack(rows64, perturbation, mode, avg=avg.double().numpy(), p=direction.double().numpy())
    gamma = byz.attack_factor.item()
    assert byz.attack_info[5] == 0.0 and abs(gamma - own["gamma"]) <= 1e-12 * own["gamma"]
    assert byz.attack_info[2] == own["binding"]
    # ... and against the reference on float64 vectors throughout: the fp32 average and direction move every scalar by
    # a relative 2^-24 h at the very most, the factor by twice that (the sensitivity the closed form was measured with)
    ref = R.attack(rows64, perturbation, mode)
    assert abs(gamma - ref["gamma"]) <= 4 * h * 2.0 ** -24 * ref["gamma"], (h, gamma, ref["gamma"])
    want = own["avg"] + np.float64(np.float32(gamma)) * own["p"]
    assert np.abs(byz.double().numpy() - want).max() <= 2.0 ** -23 * (np.abs(own["avg"]) + gamma * np.abs(own["p"])).max()


N, F, D_STEP = 11, 2, 130


@pytest.mark.parametrize("attack", R.MODES)
@pytest.mark.parametrize("gar,momentum_at", [("krum", "update"), ("median", "worker"), ("dnc", "server"), ("average", "update")])
def test_step_on_the_oracle_backed_legs(attack, gar, momentum_at):
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from byzantinemomentum_amd.step import AggregationStep
  from tests.sharded_backend import OracleBackend
  agg = ShardedAggregator(backend=OracleBackend())
  step = AggregationStep(N, F, F, gar=gar, momentum_at=momentum_at, attack=attack, attack_factor="unread", nb_past=0,
                         gradient_clip=4.0 if gar == "median" else None, attack_args={"perturbation": "unit"},
                         aggregator=agg)
  assert step.plan.attack.formed == "chain" and not step.single_call and step.plan.first_pass == "plain"
  for it in range(2):
    sampled = _rows32(N - F, D_STEP, "common", 10 + it)
    defense = step.run([g.clone() for g in sampled])
    honests = step.buffers if momentum_at == "worker" else None
    byz = step.last_byzantine
    assert byz is not None and isinstance(step.last_factor, torch.Tensor) and step.last_factor is byz.attack_factor
    assert step.last_search is None
    if honests is not None:  # the rows the rule saw are the step's own buffers: the attack is the one on THOSE rows
      again = ShardedAggregator(backend=OracleBackend()).minmax(list(honests), F, attack, "unit")[0]
      assert torch.equal(again, byz) and torch.equal(again.attack_info, byz.attack_info)
      rule = ShardedAggregator(backend=OracleBackend())
      assert torch.equal(defense, rule.median(list(honests) + [byz] * F))
    elif momentum_at == "update":
      again = ShardedAggregator(backend=OracleBackend()).minmax(sampled, F, attack, "unit")[0]
      assert torch.equal(again, byz)
      want = getattr(ShardedAggregator(backend=OracleBackend()), gar)
      want = want(sampled + [byz] * F) if gar == "average" else want(sampled + [byz] * F, F)
      assert torch.equal(defense, want)
    floats = step.floats()
    assert math.isfinite(floats["attack_norm_avg"]) and floats["attack_norm_avg"] > 0.0
  none = AggregationStep(9, 0, 0, gar="median", momentum_at="update", attack=attack, nb_past=0,
                         aggregator=ShardedAggregator(backend=OracleBackend()))
  rows = _rows32(9, 40, "iid", 2)
  assert torch.equal(none.run([g.clone() for g in rows]), O.median(rows)) and none.last_byzantine is None


def test_one_rank_issues_no_collective_and_would_issue_one():
  from byzantinemomentum_amd import _lib
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from tests.sharded_backend import OracleBackend

  class Counting(ShardedAggregator):
    def _all_reduce(self, tensor, op=None):  # (counted, never handed to torch.distributed: one process)
      self.sizes.append(int(tensor.numel()))
      return tensor
  agg = Counting(backend=OracleBackend())
  agg.sizes = []
  assert not agg.collective
  alone = agg.minmax(_rows32(7, 33, "iid", 1), 2, "minsum", "sign")[0]
  assert agg.sizes == []
  agg.collective = True  # (what force_collectives sets: the exchange is then entered with one rank)
  forced = agg.minmax(_rows32(7, 33, "iid", 1), 2, "minsum", "sign", d_total=33)[0]
  assert agg.sizes == [7 * 7 + _lib.PERTURB_SLOTS]
  assert torch.equal(alone, forced) and torch.equal(alone.attack_info, forced.attack_info)


# ---------------------------------------------------------------------------- #
# 6. the new exports

def test_the_new_exports_exist_and_carry_the_abi_version():
  import byzantinemomentum_amd as pkg
  from byzantinemomentum_amd import _lib, sharded, stats, step
  lib = _lib.load()
  for name in ("bm_perturb_workspace_bytes", "bm_perturb_stats", "bm_minmax_factor", "bm_minmax_factor_device"):
    assert hasattr(lib, name) and name in _lib.SIGNATURES
  assert lib.bm_abi_version() == _lib.ABI_VERSION == 23
  for name in ("perturb_stats", "minmax_factor", "minmax_attack", "minsum_attack"):
    assert name in stats.__all__ and callable(getattr(stats, name))
  assert pkg.minmax_attack is stats.minmax_attack and pkg.minsum_attack is stats.minsum_attack
  assert {"perturb_stats", "minmax_factor"} <= sharded.HipBackend.capabilities
  assert callable(sharded.ShardedAggregator.minmax)
  assert set(step._ATTACK_BEYOND) == {"minmax", "minsum"}
  assert all(row.formed == "chain" and not row.factor and row.first_pass in step._CHAIN for row in step._ATTACK_BEYOND.values())
  assert _lib.PERTURB_SLOTS == _lib.MAX_ROWS + 2 and set(_lib.PERTURB_KINDS) == set(R.PERTURBATIONS)
