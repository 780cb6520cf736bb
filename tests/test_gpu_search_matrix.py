"""The device form of the attacks' factor search (csrc/search_device.hip: bm_attack_line_search_device and the RANKING
instance behind bm_attack_ranking_device) against the float64 search on the vectors of tests/search_matrix.py — the
comparison of tests/test_search_matrix_cpu.py (a - e of its header, no inversion admitted), on two sources of the
(h+2)^2 squared distances:

  exact   float64 distances computed on the CPU from the rows and uploaded (h = 63 and 64 included): the search alone,
          at every case of the list, within exact_bar(kind);
  device  bm_pairwise_sqdist over honests + [avg, avg + direction] exactly as step.py forms them (stack_stats_async, then
          multi_fma3 for the unit vector), at d = 2 003 and at d = 20 011: the project's own bar 2e-5 |y64| + floor.
          The reference then takes the fp32 avg and direction the product formed.

and one AggregationStep(line_search="auto", nb_past=0) per rule that searches from these scalars (Krum, Average, Bulyan
with its ranking from the device and pass 2 evaluate-only): abscissae and factor are the float64 search's, the
objectives within the device bar, the aggregated vector within 4e-6 x scale of the float64 rule at that factor.
Every test prints the worst errors it met (profiles/search_errors.txt).  Needs an MI355X: `pytest -m gpu`.
"""

import pytest
import torch

from oracle import gar_oracle as O
from tests import search_matrix as S
from tests.test_gpu_parity_r2 import DEV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


class DeviceForm:
  """stats.attack_search_device / stats.attack_ranking_device on a device matrix."""

  def __init__(self, bm, case, ext_dev):
    self.bm, self.case, self.ext = bm, case, ext_dev

  def search(self, rule):
    c = self.case
    out = self.bm.stats.attack_search_device(self.ext, c.h, c.k, c.f, rule, evals=c.evals, negative=c.negative,
                                             m=c.m if rule == "krum" else None).cpu().tolist()
    return out[0], [(out[1 + 2 * i], out[2 + 2 * i]) for i in range(c.evals)]

  def rankings(self, mode, m, ts):
    c = self.case
    where = torch.tensor(ts, dtype=torch.float64, device=self.ext.device)
    orders = torch.stack([self.bm.stats.attack_ranking_device(self.ext, c.h, c.k, c.f, mode, where[i:i + 1], m)
                          for i in range(len(ts))]).cpu()
    assert not orders[:, c.h + c.k:].any()  # the n rows by rank, then zeros
    return [row[:c.h + c.k].tolist() for row in orders]

  def objective(self, rule, t):
    return None


def _report(case, got, source, bar):
  print("%-8s %-50s worst %.2e (of y64 alone %.2e)  gap %.2e  two best %s" %
        (source, S.case_id(case), got.worst, got.worst_rel, got.gap, got.best_two))
  S.record(source, case, got, bar)


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_device_form_on_exact_distances(bm, case):
  inputs = S.inputs_of(case)
  ext = S.exact_ext(inputs).to(DEV)
  got = S.examine(case, inputs, DeviceForm(bm, case, ext), S.within_exact(case.kind), rankings_need_copies=True)
  _report(case, got, "exact", "%.2e*max(y64,floor)" % S.exact_bar(case.kind))


def device_inputs(bm, case, d):
  """(Inputs with the avg and the direction the product forms, the device matrix) exactly as step.py forms them."""
  rows = S.honest_rows(case.kind, case.h, case.k, case.f, d, case.seed)
  honests = [r.contiguous().to(DEV) for r in rows]
  avg, _, direction = bm.stats.stack_stats_async(honests, scale=1.0, attack=case.attack, direction=True)
  unit = torch.empty_like(avg)
  bm.stats.multi_fma3([unit], [avg], [direction], 1.0, 1.0)
  ext = bm.gars.pairwise_sqdist(honests + [avg, unit])
  return S.Inputs(rows, avg.cpu(), direction.cpu()), ext


@pytest.mark.parametrize("case", S.DEVICE_CASES, ids=S.case_id)
def test_device_form_on_the_distances_of_the_device_pass(bm, case):
  inputs, ext = device_inputs(bm, case, S.D_SMALL)
  got = S.examine(case, inputs, DeviceForm(bm, case, ext), S.within_device, rankings_need_copies=True)
  _report(case, got, "device", "2e-5*y64+floor")


@pytest.mark.parametrize("case", S.LONG_CASES, ids=S.case_id)
def test_device_form_on_the_distances_of_a_long_device_pass(bm, case):
  inputs, ext = device_inputs(bm, case, S.D_PASS)
  got = S.examine(case, inputs, DeviceForm(bm, case, ext), S.within_device, rankings_need_copies=True)
  assert got.gap >= 4 * S.G and not S.two_best_condition(case, got.best_two, S.DEVICE_REL), (got.gap, got.best_two)
  _report(case, got, "device-d%d" % S.D_PASS, "2e-5*y64+floor")


# ---------------------------------------------------------------------------------------------------------------------
# One step

def _rule64(gar, grads, f):
  if gar == "krum":
    return O.krum(grads, f, precision="f64")
  if gar == "bulyan":
    return O.bulyan(grads, f, precision="f64")
  return O.average(grads, precision="f64")


@pytest.mark.parametrize("cfg", S.STEP_CASES, ids=lambda c: "%s-n%d-f%d-%s%s" % (c.gar, c.n, c.f, c.attack, "neg" if c.negative else ""))
def test_step_searches_as_the_float64_search_on_the_vectors(bm, cfg):
  from byzantinemomentum_amd.step import AggregationStep
  n, f, h, d = cfg.n, cfg.f, cfg.n - cfg.f, S.D_PASS
  step = AggregationStep(n, f, f, gar=cfg.gar, attack=cfg.attack, attack_evals=16, attack_negative=cfg.negative,
                         line_search="auto", nb_past=0)
  # the form that searched: the scalars on the device for Krum and Average; for Bulyan the ranking from the device
  # (the cursor lives there) and pass 2 evaluate-only
  if cfg.gar == "bulyan":
    assert step.plan.search == "bulyan" and step.plan.device_cursor and "bulyan_pass2_eval" in step.plan.capabilities
    assert step.ops.bulyan_pass2_eval_supported(n, f, n - f - 2, d)
  else:
    assert step.plan.search == "scalar_device"
  sampled = [g.to(DEV) for g in O.make_stack("hetero", n, f, d, cfg.seed)[0][:h]]
  defense = step.run([g.clone() for g in sampled]).clone()
  # the honest rows the rule saw: the workers' momentum buffers after their first step (the reference's default placement)
  honests = [b.clone() for b in step.buffers]
  avg, _, direction = bm.stats.stack_stats_async(honests, scale=1.0, attack=cfg.attack, direction=True)
  rows = torch.stack([b.cpu() for b in honests])
  inputs = S.Inputs(rows, avg.cpu(), direction.cpu())
  case = S.Case("hetero", h, f, f, None, cfg.attack, cfg.negative, 16, cfg.seed)
  ref = S.Reference(inputs, f)
  floor = S.objective_floor(inputs)
  if cfg.gar == "bulyan":
    want_factor, want_trace = S.bulyan_search(ref, case)
  else:
    want_factor, want_trace, _ = S.vector_search(ref, case, cfg.gar)
  trace, factor = step.last_search, step.last_factor
  S.replay(trace, factor)
  assert [x for x, _ in trace] == [x for x, _ in want_trace] and factor == want_factor, (cfg, trace, want_trace)
  worst = 0.0
  for (x, y), (_, y64) in zip(trace, want_trace):
    assert S.within_device(y, y64, floor), (cfg, x, y, y64, floor)
    worst = max(worst, abs(y - y64) / max(y64, floor))
  print("step     %-40s worst %.2e  two best %.2e" % (cfg, worst, S.two_best_differ_by(want_trace)))
  S.record("step-" + cfg.gar, case, S.Study(worst, 0.0, float("inf"), float("inf"), {cfg.gar: S.two_best_differ_by(want_trace)}, None),
           "2e-5*y64+floor")
  # the aggregated vector against the float64 rule on the rows the step aggregated, at that factor
  byz = step.last_byzantine.cpu()
  want = _rule64(cfg.gar, [r for r in rows] + [byz] * f, f)
  scale = float(rows.abs().max()) * max(1.0, abs(factor))
  assert float((defense.cpu().double() - want).abs().max()) <= 4e-6 * scale, cfg
