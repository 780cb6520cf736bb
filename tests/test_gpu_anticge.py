"""The `anticge` attack on the device (bm_anticge_sum / bm_anticge_scale, byzantinemomentum_amd.anticge_attack) and in
AggregationStep, against the restatements of tests/anticge_reference.py: the norm order and the unscaled sum bit for
bit (same additions, same order), the scaled vector within 1e-6 of max|want| of the float64 restatement (the project's
tolerance for an fp32 arithmetic output; the device's own error is the two fp32 roundings of the multiplier and the
product) and within 1e-5 of the reference's vector."""

import functools
import itertools
import math

import pytest
import torch

from oracle import gar_oracle as O
from tests import anticge_reference as A
from tests.step_reference import assert_floats_close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def run_attack(honests_dev, f_decl, f_real=1):
  """(order, unscaled sum, list of f_real vectors) of the two legs, as anticge_attack chains them."""
  from byzantinemomentum_amd import stats
  sq = stats.row_sqnorms(honests_dev).contiguous()
  total, order, scal = stats.anticge_sum(honests_dev, f_decl, sq)
  kept = total.clone()
  return order[:len(honests_dev)].tolist(), kept.cpu(), [stats.anticge_scale(total, scal)] * f_real


def restatements(honests, f_decl):
  want32, want64 = A.anticge_f32(honests, f_decl, 1), A.anticge_f64(honests, f_decl, 1)
  assert want32.order == want64.order          # (the generators keep the norms 1e-4 apart)
  return want32, want64


def check_against_restatements(honests, honests_dev, f_decl, tag, wants=None):
  want32, want64 = wants or restatements(honests, f_decl)
  order, total, res = run_attack(honests_dev, f_decl)
  assert order == want32.order, tag
  assert torch.equal(total, want32.sum), tag
  scale = float(want64.vector.abs().max())
  err = float((res[0].cpu().double() - want64.vector).abs().max())
  assert err <= 1e-6 * scale, (tag, err / max(scale, 1e-300))
  return res[0]


@pytest.mark.parametrize("name", A.CASES)
def test_fixtures_through_anticge_attack(name):
  import byzantinemomentum_amd as bm
  fx = A.Fixture(name)
  dev = [g.to(DEV) for g in fx.honests]
  kept = [g.clone() for g in dev]
  res = bm.anticge_attack(dev, fx.f_decl, fx.f_real)
  assert len(res) == fx.f_real and all(r is res[0] for r in res)
  assert all(res[0].data_ptr() != g.data_ptr() for g in dev) and res[0].shape == dev[0].shape
  assert all(torch.equal(a, b) for a, b in zip(kept, dev))
  if fx.f_real > fx.f_decl:
    assert bool(torch.isnan(res[0]).all())
    return
  got = check_against_restatements(fx.honests, dev, fx.f_decl, name)
  assert torch.equal(got, res[0])                                    # the wrapper is the two legs
  assert float((res[0].cpu() - fx.vector).abs().max()) <= 1e-5 * float(fx.vector.abs().max())
  assert bm.anticge_attack(dev, fx.f_decl, 0) == []


# ---------------------------------------------------------------------------- #
# Every instance: row counts, selections, lengths (every tail length, one and several workgroups), vector widths

ROWS = (1, 2, 9, 20, 39, 64)
LENGTHS = (1, 3, 130, 4099, 65539)
OFFSETS = (0, 1, 2)  # floats past a 16-byte boundary: 16-, 4- and 8-byte columns


@functools.lru_cache(maxsize=None)
def seeded_rows(h, d):
  """`hetero` honest rows whose norms are 1e-4 apart: the first seed from 100 h + 7 on that gives them (short rows have
  norms as random as their few coordinates)."""
  for seed in range(100 * h + 7, 100 * h + 57):
    rows = O.make_stack("hetero", h + 1, 1, d, seed)[0][:h]
    if A.norm_gap(rows) >= A.MIN_NORM_GAP:
      return tuple(rows)
  raise AssertionError(f"no seed gives {h} rows of {d} coordinates with norms 1e-4 apart")


def f_decls(h):
  return sorted({1, max(h // 2, 1), h})


def placed(rows, offset):
  """The rows on the device, each `offset` floats past a 256-byte boundary of an allocation of its own."""
  out = []
  for g in rows:
    base = torch.empty(g.numel() + 64, dtype=torch.float32, device=DEV)
    view = base[offset:offset + g.numel()]
    view.copy_(g)
    assert view.data_ptr() % 16 == 4 * offset
    out.append(view)
  return out


@pytest.mark.parametrize("h,d", list(itertools.product(ROWS, LENGTHS)))
def test_instance_matrix(h, d):
  rows = list(seeded_rows(h, d))
  assert A.norm_gap(rows) >= A.MIN_NORM_GAP
  wants = {f_decl: restatements(rows, f_decl) for f_decl in f_decls(h)}   # computed once, shared by the placements
  for offset in OFFSETS:
    dev = placed(rows, offset)
    for f_decl in f_decls(h):
      check_against_restatements(rows, dev, f_decl, (h, d, offset, f_decl), wants[f_decl])


def test_instance_matrix_leaves_no_case_out():
  assert [f_decls(h) for h in ROWS] == [[1], [1, 2], [1, 4, 9], [1, 10, 20], [1, 19, 39], [1, 32, 64]]
  for h, d in itertools.product(ROWS, LENGTHS):
    assert len(seeded_rows(h, d)) == h and seeded_rows(h, d)[0].numel() == d


# ---------------------------------------------------------------------------- #
# Edge cases

def test_more_byzantine_workers_than_declared_gives_nan():
  import byzantinemomentum_amd as bm
  dev = [g.to(DEV) for g in seeded_rows(9, 130)]
  res = bm.anticge_attack(dev, 2, 3)
  assert len(res) == 3 and all(r is res[0] for r in res) and bool(torch.isnan(res[0]).all())
  with pytest.raises(ValueError):
    bm.anticge_attack(dev, 10, 1)


def test_a_row_with_a_nan_ranks_last_and_is_never_read():
  rows = [g.clone() for g in seeded_rows(9, 4099)]
  rows[3][17] = math.nan
  dev = [g.to(DEV) for g in rows]
  got = check_against_restatements(rows, dev, 2, "nan row")
  order, total, _ = run_attack(dev, 2)
  assert order[-1] == 3 and bool(torch.isfinite(total).all()) and bool(torch.isfinite(got).all())


def test_all_zero_rows_come_back_untouched():
  import byzantinemomentum_amd as bm
  dev = [torch.zeros(4099, device=DEV) for _ in range(9)]
  res = bm.anticge_attack(dev, 2, 2)
  assert torch.equal(res[0], torch.zeros(4099, device=DEV)) and not bool(torch.signbit(res[0]).any())


# ---------------------------------------------------------------------------- #
# AggregationStep(attack="anticge") on the device

STEP_CASES = [(n, f, d, gar, at, None) for (n, f, d) in ((11, 2, 4099), (25, 5, 1031))
              for gar, at in itertools.product(("cge", "krum", "median"), ("worker", "server", "update"))]
STEP_CASES.append((11, 2, 4099, "krum", "worker", 74.0))  # clips the two largest sampled rows (norms ~ 34..84 at d = 4099)


def selected_gap(honests, f_decl):
  """norm_gap over the rows the attack reads and the first one it leaves out (rows past it may share a norm: clipping)."""
  ranked = sorted(honests, key=lambda g: g.double().pow(2).sum().item())
  return A.norm_gap(ranked[:len(honests) - f_decl + 1])


@pytest.mark.parametrize("n,f,d,gar,momentum_at,clip", STEP_CASES)
def test_step_on_the_device(n, f, d, gar, momentum_at, clip):
  from byzantinemomentum_amd.step import AggregationStep
  h = n - f
  step = AggregationStep(n, f, f, gar=gar, momentum=0.9, dampening=0.9, momentum_at=momentum_at, attack="anticge",
                         nb_past=3, gradient_clip=clip)
  assert "anticge" in step.plan.capabilities and step.plan.first_pass == "plain" and not step.plan.single_call
  loop = A.AnticgeLoop(n, f, f, gar, momentum_at, clip=clip)
  for it in range(2):  # (the second run: the updated worker buffers are the attack's input)
    sampled = A.sampled_for_step(it, h, d)
    honests, want = loop.begin(sampled)
    assert selected_gap(honests, f) >= A.MIN_NORM_GAP
    got_def = step.run([g.to(DEV) for g in sampled]).cpu()
    byz = step.last_byzantine.cpu()
    scale = float(want.vector.abs().max())
    assert float((byz - want.vector).abs().max()) <= 2e-6 * scale, (it, float((byz - want.vector).abs().max()) / scale)
    want_def, _, floats = loop.finish(byz, observed=got_def)
    print(f"{gar}-{momentum_at} step {it}: CGE ranking taken with the Byzantine norms x {loop.cge_choice!r}")
    assert float((got_def - want_def).abs().max()) <= 2e-6 * float(torch.stack(sampled).abs().max()), it
    assert_floats_close(step.floats(), floats, tag=(gar, momentum_at, it), tol=1e-5)
