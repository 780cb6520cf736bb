"""CAF and DnC through the Python layers on CPU: argument errors by name, the rule tables, the plugin names with a stub
registry, the step's constructor checks, and ShardedAggregator.caf / .dnc with the oracle-backed compute legs
(tests/sharded_backend.OracleBackend declares no capability, so the rules take the plain torch legs of
byzantinemomentum_amd.sharded) against the float64 rules on the vectors and against the host form."""

import math
import sys
import types

import numpy as np
import pytest
import torch

from tests import spectral_cases as sc

# float32 output of a float64 combination against the float64 rule on the vectors: the weights agree to ~1e-15
# (test_spectral_cpu.py), what is left is the rounding of the result to float32, 2^-24 per coordinate
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


# ---------------------------------------------------------------------------- #
# arguments and tables

def test_python_argument_errors_name_the_argument():
  from byzantinemomentum_amd import gars
  sq = torch.zeros((11, 11), dtype=torch.float64)
  for kwargs, word in ((dict(mode="pca", count=2), "mode"), (dict(mode="caf", count=6), "2 f < n"),
                       (dict(mode="caf", count=-1), "f must"), (dict(mode="caf", count=2.0), "f must"),
                       (dict(mode="dnc", count=11), "k < n"), (dict(mode="dnc", count=True), "k must"),
                       (dict(mode="caf", count=2, power_iters=0), "power_iters"),
                       (dict(mode="caf", count=2, power_iters=257), "power_iters"),
                       (dict(mode="dnc", count=2, power_iters=2.5), "power_iters")):
    with pytest.raises(ValueError, match=word):
      gars.spectral_weights(sq, 11, **kwargs)
  with pytest.raises(gars.GarInputError):
    gars.spectral_weights(sq, 65, "caf", 2)
  with pytest.raises(gars.GarInputError):
    gars.spectral_weights(sq.float(), 11, "caf", 2)
  with pytest.raises(gars.GarInputError):
    gars.spectral_weights(sq, 12, "caf", 2)            # too small a matrix
  rows = [torch.zeros(4)] * 5
  # the arguments are checked before the rows are looked at (CPU tensors: a GarInputError would come next)
  with pytest.raises(ValueError, match="2 f < n"):
    gars.caf(rows, 3)
  with pytest.raises(ValueError, match="power_iters"):
    gars.caf(rows, 1, power_iters=0)
  with pytest.raises(ValueError, match="f must"):
    gars.dnc(rows, -1)
  with pytest.raises(ValueError, match="c must"):
    gars.dnc(rows, 1, c=-0.5)
  with pytest.raises(ValueError, match="c must"):
    gars.dnc(rows, 1, c=math.inf)
  with pytest.raises(gars.GarInputError):
    gars.caf(rows, 1)                                   # CPU tensors are refused loudly: there is no fallback
  with pytest.raises(gars.GarInputError):
    gars.dnc(rows, 4, c=3.0)                            # k = min(12, n - 1) = 4 is fine; the CPU rows are not


def test_host_form_through_the_python_entry_point():
  from byzantinemomentum_amd import _lib, gars
  case = sc.cases()[1]
  rows, _ = sc.make_rows(case)
  sq = sc.exact_sqdist(rows)
  for mode in ("caf", "dnc"):
    weights, info = gars.spectral_weights(torch.from_numpy(sq), case.n, mode, case.k)   # power_iters = 16
    code, want, want_info = sc.host_weights(_lib.load(), sq, case.n, mode, case.k, 16)
    assert code == 0 and not weights.is_cuda and weights.shape == (64,) and info.shape == (4,)
    assert np.array_equal(weights.numpy(), want) and np.array_equal(info.numpy(), want_info)


def test_rule_tables_and_exports():
  import byzantinemomentum_amd as bm
  from byzantinemomentum_amd.sharded import HipBackend, ShardedAggregator
  from byzantinemomentum_amd import step
  assert bm.caf is bm.gars.caf and bm.dnc is bm.gars.dnc
  for name in ("caf", "dnc", "spectral_weights"):
    assert name in bm.gars.__all__
  assert bm.gars.NNM_RULES["caf"] is True and bm.gars.NNM_RULES["dnc"] is True     # both take f
  assert bm.gars.SCALAR_RULES == ("krum", "brute", "geomed", "cclip", "average")   # form="scalars" is not theirs
  assert "caf" in ShardedAggregator.NNM_RULES and "dnc" in ShardedAggregator.NNM_RULES
  assert ShardedAggregator.SCALAR_RULES == bm.gars.SCALAR_RULES
  assert "spectral_weights" in HipBackend.capabilities and callable(HipBackend.spectral_weights)
  assert "caf" in step._RULES and "dnc" in step._RULES
  rows = [torch.zeros(4)] * 7
  for rule in ("caf", "dnc"):
    with pytest.raises(ValueError, match="scalars"):
      bm.gars.nnm(rows, 1, rule=rule, form="scalars")
    with pytest.raises(ValueError, match="scalars"):
      bm.gars.bucketing(rows, 2, rule, seed=1, form="scalars", f=1)
    with pytest.raises(bm.gars.GarInputError):
      bm.gars.nnm(rows, 1, rule=rule)                  # the rows path knows the rule: the CPU rows are what is refused


def test_register_spectral_rules_with_a_stub_registry():
  saved = {k: sys.modules.get(k) for k in ("aggregators", "native")}
  pkg = types.ModuleType("aggregators")
  pkg.gars = {}

  def register(name, unchecked, check, upper_bound=None, influence=None):
    rule = types.SimpleNamespace(unchecked=unchecked, check=check, upper_bound=upper_bound, influence=influence)
    pkg.gars.setdefault(name, rule)
  pkg.register = register
  try:
    sys.modules["aggregators"] = pkg
    sys.modules.pop("native", None)
    import native
    at_import = set(pkg.gars)
    assert "native-caf" not in at_import and "native-dnc" not in at_import     # not at import
    assert native.register_spectral_rules() == ["native-caf", "native-dnc"]
    assert native.register_spectral_rules() == ["native-caf", "native-dnc"]    # twice: the same, registered once
    assert set(pkg.gars) == at_import | {"native-caf", "native-dnc"}
    assert native.register_center_rules() == ["native-geomed", "native-cclip"]  # unchanged
    from byzantinemomentum_amd import gars
    for name, fn in (("native-caf", gars.caf), ("native-dnc", gars.dnc)):
      rule = pkg.gars[name]
      assert rule.unchecked is fn and rule.influence is None
      assert rule.check(gradients=[], f=1) is not None and rule.check(gradients=[1, 2, 3], f=1) is None
    with pytest.raises(ValueError):
      pkg.gars["native-caf"].unchecked(gradients=[torch.zeros(4)] * 5, f=1)    # CPU tensors reach gars.caf
    del sys.modules["aggregators"]
    with pytest.raises(RuntimeError):
      native.register_spectral_rules()                                         # no registry imported
  finally:
    for k, v in saved.items():
      if v is None:
        sys.modules.pop(k, None)
      else:
        sys.modules[k] = v


# ---------------------------------------------------------------------------- #
# the sharded aggregator on the plain torch legs

@pytest.mark.parametrize("mode", ["caf", "dnc"])
@pytest.mark.parametrize("case", sc.cases(), ids=sc.case_id)
def test_sharded_rules_match_the_rule_on_the_vectors(case, mode):
  rows, _ = sc.make_rows(case)
  agg = _aggregator()
  assert agg.world_size == 1
  out = getattr(agg, mode)(_tensors(rows), case.k)
  ref = sc.vector_spectral(rows, mode, case.k, 16)
  assert out.dtype == torch.float32 and out.shape == (case.d,)
  assert sc.relative_error(out.double().numpy(), ref.out) <= BAR
  weights, info = agg.last_weights, agg.last_spectral_info.tolist()
  assert weights.shape == (64,) and abs(float(weights.sum()) - 1.0) <= 1e-12
  assert info[0] == ref.rounds and info[2] == case.n and info[3] == ref.kept


def test_torch_leg_equals_the_host_form():
  """The plain torch leg follows the library's definition: the weights of bm_spectral_weights within 1e-12, the same
  rounds, the same exclusions, NaN when no row is usable."""
  from byzantinemomentum_amd import _lib
  from byzantinemomentum_amd.torch_legs import _spectral_weights_torch
  lib = _lib.load()
  items = [(sc.case_id(case) + "-" + mode, sc.exact_sqdist(sc.make_rows(case)[0]), case.n, mode, case.k)
           for case in sc.cases()[::3] for mode in ("caf", "dnc")]
  for name, sq, n, mode, count in items + sc.crafted():
    for T in (1, 16):
      code, want, info = sc.host_weights(lib, sq, n, mode, count, T)
      got, got_info = _spectral_weights_torch(torch.from_numpy(np.array(sq, dtype=np.float64)), n, mode, count, T)
      assert code == 0, name
      np.testing.assert_allclose(got.numpy(), want, rtol=0, atol=1e-12, equal_nan=True, err_msg=name)
      got_info, info = got_info.numpy(), np.array(info)
      assert np.array_equal(got_info[[0, 2, 3]], info[[0, 2, 3]]), (name, got_info, info)
      np.testing.assert_allclose(got_info[1], info[1], rtol=1e-10, err_msg=name)


def test_dnc_count_and_nan_rows_through_the_aggregator():
  case = sc.cases()[4]  # n = 25, k = 5
  rows, _ = sc.make_rows(case)
  local = _tensors(rows)
  agg = _aggregator()
  agg.dnc(local, 5, c=1.5)                                  # k = ceil(7.5) = 8
  assert int((agg.last_weights[:25] == 0).sum()) == 8
  agg.dnc(local, 5, c=100.0)                                # k = min(500, n - 1): one row is left
  assert int((agg.last_weights[:25] != 0).sum()) == 1
  agg.dnc(local, 0)
  assert torch.equal(agg.last_weights[:25], torch.full((25,), 1.0 / 25, dtype=torch.float64))
  # the `nan` attack: five references to one NaN vector never reach the output, which is the rule on the other rows
  nan_row = torch.full_like(local[0], math.nan)
  stack = local[:20] + [nan_row] * 5
  for mode, count_clean in (("caf", None), ("dnc", 0)):
    out = getattr(agg, mode)(stack, 5)
    assert torch.isfinite(out).all() and not agg.last_weights[20:].any()
    assert agg.last_spectral_info.tolist()[2] == 20
    if mode == "dnc":                                       # k' = 5 - 5 = 0: the mean of the twenty
      ref = rows[:20].astype(np.float64).mean(axis=0)
      assert sc.relative_error(out.double().numpy(), ref) <= BAR
  out = agg.caf(local[:10] + [nan_row] * 15, 5)             # a majority of NaN rows: NaN everywhere
  assert torch.isnan(out).all()
  with pytest.raises(ValueError):
    agg.caf(local, 13)                                      # 2 f >= n
  with pytest.raises(ValueError):
    agg.dnc(local, 5, power_iters=0)
  from byzantinemomentum_amd.gars import GarInputError
  with pytest.raises(GarInputError):
    agg.caf([torch.zeros(8) for _ in range(65)], 1)


def test_nnm_and_bucketing_run_the_rules_on_the_rows_path():
  case = sc.cases()[0]
  rows, _ = sc.make_rows(case)
  agg = _aggregator()
  out = agg.nnm(_tensors(rows), case.k, rule="caf")
  assert out.shape == (case.d,) and torch.isfinite(out).all()
  out = agg.nnm(_tensors(rows), case.k, rule="dnc", c=1.0)
  assert out.shape == (case.d,) and torch.isfinite(out).all()
  with pytest.raises(ValueError, match="scalars"):
    agg.nnm(_tensors(rows), case.k, rule="caf", form="scalars")


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


def test_bad_gar_args_raise_in_the_constructor():
  for gar, bad in (("caf", dict(power_iters=0)), ("caf", dict(power_iters=257)), ("caf", dict(power_iters=2.5)),
                   ("caf", dict(c=1.0)), ("caf", dict(nu=1e-6)), ("caf", dict(m=3)), ("dnc", dict(power_iters=0)),
                   ("dnc", dict(c=-1.0)), ("dnc", dict(c=math.nan)), ("dnc", dict(c="1")), ("dnc", dict(iters=3))):
    with pytest.raises(ValueError):
      _step(gar, bad)
  _step("caf", {})
  _step("caf", dict(power_iters=256))
  _step("dnc", dict(c=1.5, power_iters=1))
  _step("dnc", dict(c=100.0))                          # k is capped at n - 1
  from byzantinemomentum_amd.step import AggregationStep
  with pytest.raises(ValueError, match="2 f < n"):
    AggregationStep(10, 5, 5, gar="caf", aggregator=_aggregator())


@pytest.mark.parametrize("gar,gar_args", [("caf", {}), ("caf", dict(power_iters=8)), ("dnc", dict(c=1.5))])
@pytest.mark.parametrize("placement", ["worker", "update", "server"])
@pytest.mark.parametrize("evals", [None, 4])
def test_plan_fields_are_those_of_geomed(gar, gar_args, placement, evals):
  from byzantinemomentum_amd.sharded import HipBackend, ShardedAggregator
  from byzantinemomentum_amd.step import AggregationStep

  class Caps:  # the plan reads the capabilities alone: the HIP backend's, without a GPU
    capabilities = HipBackend.capabilities
    device_search_rules = ("krum", "average")

  for backend in (Caps(), None):
    agg = ShardedAggregator(backend=backend) if backend is not None else _aggregator()
    common = dict(momentum_at=placement, aggregator=agg, attack_evals=evals, single_call=True)
    plan = AggregationStep(25, 5, 5, gar=gar, gar_args=gar_args, **common).plan
    like = AggregationStep(25, 5, 5, gar="geomed", **common).plan
    assert plan.first_pass == like.first_pass == ("direction" if evals else "plain")
    assert plan.search == like.search == ("generic" if evals else None)
    assert plan.accept is None and plan.single_call is False


@pytest.mark.parametrize("gar,gar_args", [("caf", {}), ("dnc", dict(c=1.0, power_iters=8))])
def test_step_runs_the_rule_on_honests_and_byzantine_rows(gar, gar_args):
  step = _step(gar, gar_args)
  for it in range(2):
    defense = step.run([g.clone() for g in _sampled(it, N - F)])
    stack = np.stack([b.numpy() for b in step.buffers] + [step.last_byzantine.numpy()] * F)
    count = F if gar == "caf" else math.ceil(gar_args["c"] * F)
    ref = sc.vector_spectral(stack, gar, count, gar_args.get("power_iters", 16))
    assert sc.relative_error(defense.double().numpy(), ref.out) <= BAR
    assert math.isnan(step.floats()["accept_ratio"])
  searching = _step(gar, gar_args, attack_evals=4)
  assert searching.plan.search == "generic"
  searching.run(_sampled(0, N - F))
  assert len(searching.last_search) == 4
