"""bm_attack_vector on the device — every kind at every vector width, both launches of a cut pass, every place the
targeted coordinate can fall —, the public `nan_attack` / `bulyan_attack` / `empire_strict_attack` on the fixtures of the
reference, and AggregationStep(attack="nan" | "hidden" | "empire-strict") with the HIP backend against the restatement
loop of tests/attack_vectors_reference.py.

Bounds: the kernel's output is ONE fp32 expression per coordinate, so it is compared bit for bit with the same
expression in torch on the CPU copy.  The step's honest rows come from fused multiply-adds on the device and from
separate roundings in the loop: vectors then agree within 1e-6 of max|want| (the project's tolerance for one fp32
arithmetic output), statistics within 1e-5."""

import ctypes
import math

import pytest
import torch

from tests import attack_vectors_reference as R
from tests.golden_io import same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 32        # floats on each side of an output
SENTINEL = 777.0
LENGTHS = (1, 3, 130, 4099, 65539)
OFFSETS = (0, 1, 2)  # floats past a 16-byte boundary: 16-, 4- and 8-byte columns
FACTOR = -1.7


def placed_input(values, offset):
  base = torch.empty(values.numel() + 64, dtype=torch.float32, device=DEV)
  view = base[offset:offset + values.numel()]
  view.copy_(values)
  assert view.data_ptr() % 16 == 4 * offset
  return view


def guarded_output(d, offset):
  """(the whole allocation, filled with a sentinel; the d floats of it the kernel may write, `offset` floats past a
  16-byte boundary with GUARD + offset floats before and at least GUARD behind)."""
  base = torch.full((d + 2 * GUARD + 8,), SENTINEL, dtype=torch.float32, device=DEV)
  start = GUARD + offset
  view = base[start:start + d]
  assert view.data_ptr() % 16 == 4 * offset
  return base, view, start


def guards_intact(base, start, d):
  host = base.cpu()
  return bool((host[:start] == SENTINEL).all()) and bool((host[start + d:] == SENTINEL).all())


def special_average(d):
  gen = torch.Generator().manual_seed(40 + d)
  avg = torch.randn(d, generator=gen)
  for i, value in enumerate((-0.0, math.inf, 1e-41)):   # a negative zero, an infinity, a denormal
    if d > 2 * i + 1 or (d == 1 and i == 0):
      avg[(2 * i + 1) % d] = value
  return avg


def expected(kind, avg, factor32, target):
  if kind == "nan":
    return torch.full_like(avg, math.nan), None
  if kind == "scale":
    return avg * factor32, None
  direction = torch.ones_like(avg) if kind == "shift_all" else torch.zeros_like(avg)
  if kind == "shift_one" and target >= 0:
    direction[target] = 1
  return avg + factor32 * direction, direction


def bits_equal(a, b):
  """The same fp32 bit patterns, the sign of a zero included."""
  a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
  return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def targets_of(d):
  return sorted({t for t in (0, 1, 3, d - 4, d - 2, d - 1) if 0 <= t < d}) + [-1]


def launch(kind, avg, target, factor, out, direction):
  from byzantinemomentum_amd import _lib, gars
  lib = _lib.load()
  host = ctypes.c_float(0.0 if isinstance(factor, torch.Tensor) else factor)
  dev = gars._ptr(factor) if isinstance(factor, torch.Tensor) else None
  with torch.cuda.device(avg.device):
    rc = lib.bm_attack_vector(_lib.ATTACK_VECTOR_KINDS[kind], gars._ptr(avg), avg.numel(), target, host, dev, gars._ptr(out),
                              gars._ptr(direction) if direction is not None else None, gars._stream(avg.device))
  assert rc == 0, (kind, rc)


@pytest.mark.parametrize("d", LENGTHS)
def test_instance_matrix(d):
  avg_host = special_average(d)
  factor32 = torch.tensor(FACTOR, dtype=torch.float32)
  factor_dev = torch.tensor([FACTOR, 123.0], dtype=torch.float64, device=DEV)
  runs = 0
  for offset in OFFSETS:
    avg = placed_input(avg_host, offset)
    cases = [("nan", -1, False), ("scale", -1, False)]
    cases += [("shift_all", -1, with_dir) for with_dir in (False, True)]
    cases += [("shift_one", t, with_dir) for t in targets_of(d) for with_dir in (False, True)]
    for kind, target, with_dir in cases:
      want, want_dir = expected(kind, avg_host, factor32, target)
      for factor in (FACTOR, factor_dev):
        base, out, start = guarded_output(d, offset)
        dbase, dview, dstart = guarded_output(d, offset) if with_dir else (None, None, None)
        launch(kind, avg, target, factor, out, dview)
        tag = (d, offset, kind, target, with_dir, isinstance(factor, torch.Tensor))
        got = out.cpu()
        if kind == "nan":
          assert bool((got.view(torch.int32) == 0x7FC00000).all()), tag
        else:
          assert bits_equal(got, want), tag
        assert guards_intact(base, start, d), tag
        if with_dir:
          assert bits_equal(dview, want_dir) and guards_intact(dbase, dstart, d), tag
        assert bits_equal(avg, avg_host), tag
        runs += 1
  assert runs == 3 * 2 * (4 + 2 * len(targets_of(d)))


def test_instance_matrix_leaves_no_case_out():
  assert [targets_of(d) for d in LENGTHS] == [[0, -1], [0, 1, 2, -1], [0, 1, 3, 126, 128, 129, -1],
                                              [0, 1, 3, 4095, 4097, 4098, -1], [0, 1, 3, 65535, 65537, 65538, -1]]
  for d in LENGTHS:
    avg = special_average(d)
    assert bool(torch.signbit(avg[1 % d])) and float(avg[1 % d]) == 0.0
    if d > 3:
      assert math.isinf(float(avg[3])) and 0.0 < float(avg[5]) < 1.2e-38
  # mixed placements: the width is the narrowest any pointer allows (avg 16-byte, out 8-byte, direction 4-byte aligned)
  avg_host = special_average(4099)
  avg = placed_input(avg_host, 0)
  base, out, start = guarded_output(4099, 2)
  dbase, dview, dstart = guarded_output(4099, 1)
  launch("shift_one", avg, 4097, FACTOR, out, dview)
  want, want_dir = expected("shift_one", avg_host, torch.tensor(FACTOR, dtype=torch.float32), 4097)
  assert bits_equal(out, want) and bits_equal(dview, want_dir)
  assert guards_intact(base, start, 4099) and guards_intact(dbase, dstart, 4099)


def test_python_leg():
  from byzantinemomentum_amd import stats
  avg_host = special_average(4099)
  avg = avg_host.to(DEV)
  f32 = torch.tensor(0.1, dtype=torch.float32)
  got, direction = stats.attack_vector("shift_one", avg, 0.1, target=4098, want_direction=True)
  want, want_dir = expected("shift_one", avg_host, f32, 4098)
  assert bits_equal(got, want) and bits_equal(direction, want_dir)
  assert bits_equal(stats.attack_vector("shift_one", avg, 0.1), expected("shift_one", avg_host, f32, -1)[0])
  dev = torch.tensor([0.1], dtype=torch.float64, device=DEV)
  assert bits_equal(stats.attack_vector("scale", avg, dev), avg_host * f32)
  assert bits_equal(stats.attack_vector("shift_all", avg, dev), avg_host + f32)
  assert bool((stats.attack_vector("nan", avg).cpu().view(torch.int32) == 0x7FC00000).all())
  assert bits_equal(avg, avg_host)
  from byzantinemomentum_amd.gars import GarInputError
  for bad in (lambda: stats.attack_vector("shift", avg, 1.0), lambda: stats.attack_vector("scale", avg),
              lambda: stats.attack_vector("scale", avg, 1.0, want_direction=True),
              lambda: stats.attack_vector("shift_one", avg, 1.0, target=4099),
              lambda: stats.attack_vector("scale", avg, torch.tensor([1.0], device=DEV))):
    with pytest.raises(GarInputError):
      bad()


# ---------------------------------------------------------------------------- #
# The public functions on the fixtures

def device_rule(gar):
  import byzantinemomentum_amd as bm
  if gar == "median":
    return lambda gradients, f, model=None: bm.median(gradients)
  return lambda gradients, f, model=None: getattr(bm, gar)(gradients, f)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_public_functions_on_the_fixtures(name):
  import byzantinemomentum_amd as bm
  fx = R.Fixture(name)
  c = fx.case
  dev = [g.to(DEV) for g in fx.honests]
  kept = [g.clone() for g in dev]
  defense = device_rule(c["gar"]) if c["gar"] else None
  if c["attack"] == "nan":
    call = lambda f_real: bm.nan_attack(dev, f_real, f_decl=fx.f, defense=defense, model=None)  # noqa: E731
  elif c["attack"] == "bulyan":
    call = lambda f_real: bm.bulyan_attack(dev, f_real, f_decl=fx.f, defense=defense, model=None, factor=c["arg"],  # noqa: E731
                                           negative=c["negative"], target_idx=c["target_idx"])
  else:
    call = lambda f_real: bm.empire_strict_attack(dev, f_real, f_decl=fx.f, defense=defense, model=None,  # noqa: E731
                                                  epsilon=c["arg"])
  res = call(fx.f)
  assert len(res) == fx.f and all(r is res[0] for r in res)
  assert all(res[0].data_ptr() != g.data_ptr() for g in dev) and res[0].shape == dev[0].shape
  assert all(torch.equal(a, b) for a, b in zip(kept, dev))
  assert call(0) == []
  got = res[0].cpu()
  if c["attack"] == "nan":
    assert same_bits(got, fx.vector)
    return
  # the fp32 restatement on the sequential mean the device forms, at the factor the reference applied
  factor = fx.factor if fx.factor is not None else (-c["arg"] if c["negative"] else c["arg"])
  want = R.vector_from(c["attack"], R.seq_mean(fx.honests), factor, c["target_idx"])
  assert same_bits(got, want), name
  assert float((got - fx.vector).abs().max()) <= 1e-5 * float(fx.vector.abs().max())


def test_public_functions_check_their_arguments():
  import byzantinemomentum_amd as bm
  dev = [g.to(DEV) for g in R.Fixture("nan_n7_f1").honests]
  for bad in (R.D, -R.D - 1):
    with pytest.raises(IndexError):
      bm.bulyan_attack(dev, 1, factor=1.0, target_idx=bad)
  with pytest.raises(ValueError):
    bm.bulyan_attack(dev, 1, factor=1.0, target_idx=1.5)
  with pytest.raises(ValueError):
    bm.bulyan_attack(dev, 1, f_decl=1, defense=None, factor=-4)     # a search needs the rule
  first = bm.bulyan_attack(dev, 1, factor=1.0, target_idx=-R.D)[0].cpu()
  assert same_bits(first, R.vector_from("bulyan", R.seq_mean([g.cpu() for g in dev]), 1.0, 0))


# ---------------------------------------------------------------------------- #
# AggregationStep with the HIP backend

N, F, D = 11, 2, 4099
STEP_NAME = {"nan": "nan", "bulyan": "hidden", "empire-strict": "empire-strict"}
FIXED = {"nan": (1.1, None), "bulyan": (1.5, {"target_idx": -1}), "empire-strict": (2, None)}
STEP_CASES = [(attack, gar, at) for attack in R.ATTACKS for gar in ("krum", "median") for at in ("worker", "server", "update")]
STEP_CASES += [(attack, "bulyan", "worker") for attack in R.ATTACKS]
STEP_CASES += [("bulyan-all", "median", "worker"), ("bulyan-4097", "krum", "update")]


def make_step(attack, gar, momentum_at, factor=1.1, args=None, evals=None, negative=False, nb_past=3):
  from byzantinemomentum_amd.step import AggregationStep
  return AggregationStep(N, F, F, gar=gar, momentum=0.9, dampening=0.9, momentum_at=momentum_at, attack=STEP_NAME[attack],
                         attack_factor=factor, attack_args=args, attack_evals=evals, attack_negative=negative,
                         nb_past=nb_past)


def close(got, want, scale, bound, tag):
  assert torch.equal(got.isnan(), want.isnan()), tag
  err = float((got - want).nan_to_num(0.0).abs().max())
  assert err <= bound * scale, (tag, err / scale)


def finish_and_compare(step, loop, sampled, got_def, tag):
  byz = step.last_byzantine.cpu()
  want_def, want_upd, floats = loop.finish(byz)
  scale = float(torch.stack(sampled).abs().max())
  close(got_def.cpu(), want_def, scale, 1e-6, tag)
  close(step.update_gradient().cpu(), want_upd, scale, 1e-6, tag)
  got = step.floats()
  R.assert_floats_close_nan(got, floats, tag=tag, tol=1e-5)
  want_ratio = floats["accept_ratio"]
  assert got["accept_ratio"] == want_ratio or (math.isnan(want_ratio) and got["accept_ratio"] is math.nan), tag
  return got


@pytest.mark.parametrize("attack,gar,momentum_at", STEP_CASES)
def test_step_on_the_device(attack, gar, momentum_at):
  from byzantinemomentum_amd import stats
  if attack.startswith("bulyan-"):
    target = attack.split("-")[1]
    attack, factor, args = "bulyan", -2.0, {"target_idx": "all" if target == "all" else int(target)}
  else:
    factor, args = FIXED[attack]
  target_idx = (args or {}).get("target_idx", -1)
  step = make_step(attack, gar, momentum_at, factor, args)
  assert "attack_vector" in step.plan.capabilities
  assert step.plan.first_pass == "plain" and step.plan.search is None and not step.plan.single_call
  loop = R.Loop(N, F, F, gar, momentum_at)
  for it in range(3):
    sampled = R.sampled_for_step(it, N - F, D)
    honests, avg = loop.begin(sampled)
    got_def = step.run([g.to(DEV) for g in sampled])
    byz = step.last_byzantine.cpu()
    tag = (attack, gar, momentum_at, it)
    if attack == "nan":
      assert bool((byz.view(torch.int32) == 0x7FC00000).all()), tag
    else:
      want = R.vector_from(attack, avg, factor, target_idx)
      close(byz, want, float(want.abs().max()), 1e-6, tag)
      if momentum_at == "worker":  # the step's own honest rows are at hand: the same fp32 expression on THEIR average
        own = stats.stack_stats_async(list(step.buffers))[0].cpu()
        assert same_bits(byz, R.vector_from(attack, own, factor, target_idx)), tag
    got = finish_and_compare(step, loop, sampled, got_def, tag)
    if attack == "nan":
      assert all(math.isnan(got[k]) for k in ("attack_norm_avg", "attack_norm_dev", "attack_norm_max", "cosin_splatt",
                                              "cosin_honatt", "cosin_attdef"))


SEARCHES = [("bulyan", "median", False, "device"), ("bulyan", "krum", False, "scalar_device"),
            ("empire-strict", "krum", False, "scalar_host"), ("empire-strict", "trmean", False, "device")]


@pytest.mark.parametrize("attack,gar,negative,form", SEARCHES)
def test_searched_step_on_the_device(attack, gar, negative, form):
  step = make_step(attack, gar, "worker", evals=R.EVALS, negative=negative, args={"target_idx": -1} if attack == "bulyan" else None)
  plan = step.plan
  assert not plan.single_call
  if form == "device":
    assert plan.device_cursor and plan.search in ("median", "colwise_eval")
  else:
    assert plan.search == form and plan.device_cursor == (form == "scalar_device")
  assert plan.first_pass == ("direction" if attack == "empire-strict" else "plain")
  loop = R.Loop(N, F, F, gar, "worker")
  for it in range(2):
    sampled = R.sampled_for_step(it, N - F, D)
    honests, avg = loop.begin(sampled)
    got_def = step.run([g.to(DEV) for g in sampled])
    want = R.restate(attack, honests, F, F, defense=lambda grads, f: loop.rule(grads), arg=-R.EVALS, negative=negative,
                     target_idx=-1, precision="f64", avg=avg)
    tag = (attack, gar, it)
    print(f"{attack}-{gar} step {it}: factor {step.last_factor!r} against {want.factor!r}")
    assert step.last_factor == want.factor, tag
    assert [x for x, _ in step.last_search] == [x for x, _ in want.trace], tag
    for (_, y), (_, y_want) in zip(step.last_search, want.trace):
      assert abs(y - y_want) <= 1e-5 * max(abs(y_want), 1e-6), tag
    close(step.last_byzantine.cpu(), want.vector, float(want.vector.abs().max()), 1e-6, tag)
    finish_and_compare(step, loop, sampled, got_def, tag)


def test_a_captured_hidden_step_is_the_eager_step():
  """One `hidden` step at a fixed factor recorded through graphs.GraphedCall and replayed once.  nb_past = 0: a replay
  does not run the Python of the step again.  Warm-up (2 runs) + one replay = three steps on the same sampled
  gradients; the eager twin runs three."""
  from byzantinemomentum_amd.graphs import GraphedCall
  sampled = [g.to(DEV) for g in R.sampled_for_step(0, N - F, D)]
  graphed = make_step("bulyan", "median", "worker", 1.5, {"target_idx": 4097}, nb_past=0)
  eager = make_step("bulyan", "median", "worker", 1.5, {"target_idx": 4097}, nb_past=0)
  call = GraphedCall(lambda: graphed.run(sampled), warmup=2)
  defense = call()
  got = graphed.floats()
  for _ in range(3):
    want_defense = eager.run(sampled)
  assert same_bits(defense.cpu(), want_defense.cpu())
  assert same_bits(graphed.last_byzantine.cpu(), eager.last_byzantine.cpu())
  for x, y in zip(graphed.buffers, eager.buffers):
    assert torch.equal(x, y)
  assert got == eager.floats()
