"""The `nan`, `bulyan` (here "hidden") and `empire-strict` attacks without a GPU: the restatements of
tests/attack_vectors_reference.py against the committed outputs of the reference (and the live reference where its
checkout is staged), AggregationStep(attack="nan" | "hidden" | "empire-strict") on the oracle-backed legs, the argument
checks of the step and of bm_attack_vector, and the sharded attacks over two gloo ranks."""

import ctypes
import itertools
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import gar_oracle as O
from oracle import reference_loader
from tests import attack_vectors_reference as R
from tests.golden_io import same_bits

STEP_NAME = {"nan": "nan", "bulyan": "hidden", "empire-strict": "empire-strict"}


# ---------------------------------------------------------------------------- #
# The restatements against the reference

def _restate_case(fx, precision):
  c = fx.case
  rule = R.oracle_rule(c["gar"]) if c["gar"] else None
  return R.restate(c["attack"], fx.honests, fx.f, fx.f, defense=rule, arg=c["arg"], negative=c["negative"],
                   target_idx=c["target_idx"], precision=precision)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_f32_restatement_is_the_reference_bit_for_bit(name):
  fx = R.Fixture(name)
  assert fx.case == R.CASES[name]
  rows, h = O.make_stack("hetero", fx.case["n"], fx.f, R.D, fx.seed)
  assert all(torch.equal(a, b) for a, b in zip(rows[:h], fx.honests))
  got = _restate_case(fx, "f32")
  assert same_bits(got.vector, fx.vector)
  if fx.case["attack"] == "nan":
    assert bool((fx.vector.view(torch.int32) == 0x7FC00000).all())
  if fx.factor is not None:
    assert got.factor == fx.factor and len(got.trace) == R.EVALS
  if reference_loader.available():
    kept = [g.clone() for g in fx.honests]
    defense = R.reference_rule(fx.case["gar"]) if fx.case["gar"] else None
    live = R.reference_attack(fx.case["attack"])(grad_honests=fx.honests, f_real=fx.f, f_decl=fx.f, defense=defense,
                                                 model=None, **R.reference_kwargs(fx.case))
    assert len(live) == fx.f and all(v is live[0] for v in live) and all(live[0] is not g for g in fx.honests)
    assert same_bits(live[0], got.vector)
    assert all(torch.equal(a, b) for a, b in zip(kept, fx.honests))


@pytest.mark.parametrize("name", R.SEARCHED)
def test_f64_objective_settles_on_the_reference_factor(name):
  """The condition under which a searched fixture was kept (scripts/make_golden_attacks.py)."""
  fx = R.Fixture(name)
  got = _restate_case(fx, "f64")
  assert got.factor == fx.factor
  assert same_bits(got.vector, fx.vector)


def test_restatement_edge_cases():
  rows = [torch.tensor([1.0, -0.0, 3.0]), torch.tensor([3.0, -0.0, 5.0])]
  assert R.restate("bulyan", rows, 0, arg=1.0).vector is None
  assert torch.equal(R.restate("bulyan", rows, 1, arg=2.0, target_idx=-1).vector, torch.tensor([2.0, 0.0, 6.0]))
  assert torch.equal(R.restate("bulyan", rows, 1, arg=2.0, negative=True, target_idx=0).vector, torch.tensor([0.0, 0.0, 4.0]))
  got = R.vector_from("bulyan", rows[0], 2.0, -1)
  assert torch.equal(got, torch.tensor([1.0, 0.0, 5.0])) and not bool(torch.signbit(got[1]))   # -0.0 + 2 * 0 = +0.0
  got = R.vector_from("bulyan", rows[0], -2.0, 0)
  assert torch.equal(got, torch.tensor([-1.0, 0.0, 3.0])) and bool(torch.signbit(got[1]))      # -0.0 + -2 * 0 = -0.0
  with pytest.raises(IndexError):
    R.restate("bulyan", rows, 1, arg=2.0, target_idx=3)
  assert torch.equal(R.restate("empire-strict", rows, 1, arg=2).vector, torch.tensor([-4.0, 0.0, -8.0]))


# ---------------------------------------------------------------------------- #
# The C ABI, no GPU: bad arguments are refused before any HIP call

def test_entry_point_validates_arguments_without_gpu():
  from byzantinemomentum_amd import build, _lib
  build.build()
  lib = _lib.load()
  avg, out, direction = ((ctypes.c_float * 16)() for _ in range(3))
  buf = (ctypes.c_double * 1)()
  one = ctypes.c_float(1.0)
  call = lib.bm_attack_vector
  NAN, ONE, ALL, SCALE = (_lib.ATTACK_VECTOR_KINDS[k] for k in ("nan", "shift_one", "shift_all", "scale"))
  assert (NAN, ONE, ALL, SCALE) == (0, 1, 2, 3)
  assert call(4, avg, 16, 0, one, None, out, None, None) == _lib.EINVAL          # an unknown kind
  assert call(-1, avg, 16, 0, one, None, out, None, None) == _lib.EINVAL
  assert call(ONE, avg, -1, -1, one, None, out, None, None) == _lib.EINVAL       # d < 0
  assert call(ONE, avg, 16, 0, one, None, None, None, None) == _lib.EINVAL       # nowhere to write
  assert call(ONE, None, 16, 0, one, None, out, None, None) == _lib.EINVAL       # no average
  assert call(ALL, None, 16, -1, one, None, out, None, None) == _lib.EINVAL
  assert call(SCALE, None, 16, -1, one, None, out, None, None) == _lib.EINVAL
  assert call(NAN, None, -1, -1, one, None, out, None, None) == _lib.EINVAL      # (NAN needs no average, d < 0 still refused)
  assert call(ONE, avg, 16, 16, one, None, out, None, None) == _lib.EINVAL       # target == d
  assert call(ONE, avg, 16, -2, one, None, out, None, None) == _lib.EINVAL       # target < -1
  assert call(ONE, avg, 0, 0, one, None, out, None, None) == _lib.EINVAL         # no coordinate 0 in an empty buffer
  assert call(NAN, avg, 16, -1, one, None, out, direction, None) == _lib.EINVAL  # no direction with NAN
  assert call(SCALE, avg, 16, -1, one, None, out, direction, None) == _lib.EINVAL  # nor with SCALE
  assert call(ONE, avg, 16, 0, one, None, avg, None, None) == _lib.EINVAL        # out is avg
  assert call(ONE, avg, 16, 0, one, None, out, out, None) == _lib.EINVAL         # out is direction_out
  assert call(ONE, avg, 8, 0, one, buf, ctypes.byref(avg, 16), None, None) == _lib.EINVAL   # out overlaps avg
  for kind in (NAN, ONE, ALL, SCALE):                                            # an empty shard: nothing to do
    assert call(kind, avg, 0, -1, one, None, out, None, None) == 0
  assert call(NAN, None, 0, -1, one, None, out, None, None) == 0
  assert lib.bm_abi_version() == 23


def test_signatures_still_mirror_the_header():
  from byzantinemomentum_amd import _lib
  from tests.test_abi import declared_functions
  names = declared_functions()
  assert sorted(_lib.SIGNATURES) == names and "bm_attack_vector" in names


def test_the_package_exports_the_reference_names():
  import byzantinemomentum_amd as bm
  from byzantinemomentum_amd.sharded import HipBackend
  assert callable(bm.nan_attack) and callable(bm.bulyan_attack) and callable(bm.empire_strict_attack)
  assert "attack_vector" in HipBackend.capabilities and callable(HipBackend.attack_vector)


# ---------------------------------------------------------------------------- #
# AggregationStep on the oracle-backed legs

N, F = 11, 2
RULES = ("krum", "median", "trmean", "bulyan", "cge")
# attack of the reference -> (attack_factor, attack_args) of the fixed-factor runs, one target form per placement
FIXED_ARGS = {
  ("nan", "worker"): (1.1, None), ("nan", "server"): (1.1, None), ("nan", "update"): (1.1, None),
  ("bulyan", "worker"): (1.5, None), ("bulyan", "server"): (0.75, {"target_idx": "all"}),
  ("bulyan", "update"): (-2.0, {"target_idx": 17}),
  ("empire-strict", "worker"): (2, None), ("empire-strict", "server"): (1, None), ("empire-strict", "update"): (3, None),
}


def make_step(attack, gar, momentum_at, factor=1.1, args=None, evals=None, negative=False, clip=None, aggregator=None,
              n=N, f=F, nb_past=3):
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from byzantinemomentum_amd.step import AggregationStep
  from tests.sharded_backend import OracleBackend
  agg = aggregator or ShardedAggregator(backend=OracleBackend())
  return AggregationStep(n, f, f, gar=gar, momentum=0.9, dampening=0.9, momentum_at=momentum_at, attack=STEP_NAME[attack],
                         attack_factor=factor, attack_args=args, attack_evals=evals, attack_negative=negative,
                         nb_past=nb_past, gradient_clip=clip, aggregator=agg)


def run_and_compare(step, loop, attack, factor, target_idx, steps=3, clip_f32=False):
  h = loop.h
  for it in range(steps):
    sampled = R.sampled_for_step(it, h, R.D)
    honests, avg = loop.begin(sampled, clip_f32=clip_f32)
    got_def = step.run([g.clone() for g in sampled])
    byz = step.last_byzantine
    want = R.vector_from(attack, avg, factor, target_idx)
    assert same_bits(byz, want), (attack, it)
    assert all(byz.data_ptr() != g.data_ptr() for g in sampled) and byz.data_ptr() != got_def.data_ptr()
    want_def, want_upd, floats = loop.finish(byz)
    assert R.same_values(got_def, want_def), (attack, it)
    assert R.same_values(step.update_gradient(), want_upd)
    got = step.floats()
    if attack == "nan":
      assert all(math.isnan(got[k]) for k in ("attack_norm_avg", "attack_norm_dev", "attack_norm_max", "cosin_splatt",
                                              "cosin_honatt", "cosin_attdef"))
    R.assert_floats_close_nan(got, floats, tag=(attack, it), tol=1e-5)
    want_ratio = floats["accept_ratio"]
    assert got["accept_ratio"] == want_ratio or (math.isnan(want_ratio) and got["accept_ratio"] is math.nan)


@pytest.mark.parametrize("attack,momentum_at,gar", list(itertools.product(R.ATTACKS, ("worker", "server", "update"), RULES)))
def test_step_matches_the_restatement(attack, momentum_at, gar):
  assert not dist.is_initialized()
  factor, args = FIXED_ARGS[(attack, momentum_at)]
  step = make_step(attack, gar, momentum_at, factor, args)
  assert step.plan.first_pass == "plain" and step.plan.search is None and not step.plan.single_call
  run_and_compare(step, R.Loop(N, F, F, gar, momentum_at), attack, factor, (args or {}).get("target_idx", -1))


def test_step_with_clipping():
  """(clips the largest rows; the step's clipping factor is an fp32 number and so is the loop's here)"""
  step = make_step("bulyan", "median", "worker", 1.5, {"target_idx": 5}, clip=19.0)
  run_and_compare(step, R.Loop(N, F, F, "median", "worker", clip=19.0), "bulyan", 1.5, 5, steps=2, clip_f32=True)


@pytest.mark.parametrize("name", R.FIXED)
def test_step_on_the_fixtures(name):
  """The fixture's honest rows as the sampled gradients of an update-placement step: the step's sequential average
  against the reference's `mean(dim=0)` — one fp32 arithmetic output apart at the most."""
  fx = R.Fixture(name)
  c = fx.case
  factor = (-c["arg"] if c["negative"] else c["arg"]) if c["arg"] is not None else 1.1
  args = {"target_idx": c["target_idx"]} if c["attack"] == "bulyan" else None
  step = make_step(c["attack"], "median", "update", factor, args, n=c["n"], f=fx.f, nb_past=0)
  step.run([g.clone() for g in fx.honests])
  if c["attack"] == "nan":
    assert same_bits(step.last_byzantine, fx.vector)
  else:
    scale = float(fx.vector.abs().max())
    assert float((step.last_byzantine - fx.vector).abs().max()) <= 1e-6 * scale


SEARCHES = [("bulyan", gar, negative, target) for gar in RULES for negative, target in ((False, -1), (True, "all"))]
SEARCHES += [("bulyan", "median", True, -1), ("bulyan", "krum", False, "all")]
SEARCHES += [("empire-strict", gar, False, -1) for gar in RULES]


@pytest.mark.parametrize("attack,gar,negative,target", SEARCHES)
def test_searched_step_matches_the_f64_objective_restatement(attack, gar, negative, target):
  """The same factor and the same abscissae as the restatement whose objective is float64, on the step's own honest
  rows; the vector is the fp32 expression at that factor on the step's average."""
  args = {"target_idx": target} if attack == "bulyan" else None
  step = make_step(attack, gar, "worker", evals=R.EVALS, negative=negative, args=args)
  plan = step.plan
  assert not plan.single_call and not plan.device_cursor
  assert plan.search == ("scalar_host" if gar == "krum" else {"median": "median", "bulyan": "bulyan"}.get(gar, "generic"))
  assert plan.first_pass == ("direction" if attack == "empire-strict" else "plain")
  loop = R.Loop(N, F, F, gar, "worker")
  for it in range(2):
    sampled = R.sampled_for_step(it, N - F, R.D)
    honests, avg = loop.begin(sampled)
    got_def = step.run([g.clone() for g in sampled])
    want = R.restate(attack, honests, F, F, defense=lambda grads, f: loop.rule(grads), arg=-R.EVALS, negative=negative,
                     target_idx=target, precision="f64", avg=avg)
    print(f"{attack}-{gar} step {it}: factor {step.last_factor!r} against {want.factor!r}")
    assert step.last_factor == want.factor
    assert [x for x, _ in step.last_search] == [x for x, _ in want.trace]
    for (_, y), (_, y_want) in zip(step.last_search, want.trace):
      assert abs(y - y_want) <= 1e-5 * max(abs(y_want), 1e-6)
    assert same_bits(step.last_byzantine, want.vector)
    want_def, _, floats = loop.finish(step.last_byzantine)
    assert R.same_values(got_def, want_def)
    R.assert_floats_close_nan(step.floats(), floats, tag=(attack, gar, it), tol=1e-5)


def test_step_rejects_bad_arguments():
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from byzantinemomentum_amd.step import AggregationStep
  from tests.sharded_backend import OracleBackend
  agg = ShardedAggregator(backend=OracleBackend())

  def step(**kw):
    return AggregationStep(11, 2, 2, aggregator=agg, **kw)

  with pytest.raises(ValueError, match="unknown attack.*hidden"):
    step(attack="bulyan")
  with pytest.raises(ValueError, match="unknown attack"):
    step(attack="empire_strict")
  with pytest.raises(ValueError, match="attack_evals"):
    step(attack="nan", attack_evals=4)
  step(attack="nan", attack_factor="ignored")
  for bad in ({"target": 3}, {"target_idx": 3, "more": 1}, [3]):
    with pytest.raises(ValueError, match="attack_args"):
      step(attack="hidden", attack_args=bad)
  for bad in (1.5, "last", None, True):
    with pytest.raises(ValueError, match="target_idx"):
      step(attack="hidden", attack_args={"target_idx": bad})
  for other in ("empire", "little", "anticge", "nan", "empire-strict"):
    with pytest.raises(ValueError, match="attack_args"):
      step(attack=other, attack_factor=2, attack_args={"target_idx": 3})
    with pytest.raises(ValueError, match="attack_args"):
      step(attack=other, attack_factor=2, attack_args={})
  for bad in (1.1, 2.0, 0, -3, True, None):
    with pytest.raises(ValueError, match="epsilon"):
      step(attack="empire-strict", attack_factor=bad)
  step(attack="empire-strict", attack_factor=2)
  step(attack="empire-strict", attack_evals=4)                     # (attack_factor is not read with a search)
  with pytest.raises(ValueError, match="negative"):
    step(attack="empire-strict", attack_factor=2, attack_negative=True)
  with pytest.raises(ValueError, match="attack_evals"):
    step(attack="hidden", attack_evals=0)
  step(attack="hidden", attack_args={"target_idx": "all"}, attack_evals=4, attack_negative=True)
  # target_idx out of range: IndexError when the vector's length is known, as indexing raises in the reference
  rows = R.sampled_for_step(0, 9, 64)
  for bad in (64, -65):
    with pytest.raises(IndexError):
      step(attack="hidden", attack_args={"target_idx": bad}, momentum_at="update", nb_past=0).run([g.clone() for g in rows])
    with pytest.raises(IndexError):
      agg.attack_vector("shift_one", rows[0], 1.0, target_idx=bad)
  step(attack="hidden", attack_args={"target_idx": -64}, momentum_at="update", nb_past=0).run([g.clone() for g in rows])
  with pytest.raises(ValueError):
    agg.attack_vector("shift", rows[0], 1.0, target_idx=0)
  with pytest.raises(ValueError):
    agg.attack_vector("scale", rows[0], 1.0, want_direction=True)
  with pytest.raises(ValueError):
    agg.attack_vector("shift_one", rows[0], 1.0, target_idx="all")


@pytest.mark.parametrize("attack", R.ATTACKS)
def test_no_byzantine_worker_no_attack(attack):
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from byzantinemomentum_amd.step import AggregationStep
  from tests.sharded_backend import OracleBackend
  rows = R.sampled_for_step(0, 9, 64)
  for evals in ((None,) if attack == "nan" else (None, 4)):
    none = AggregationStep(9, 0, 0, gar="median", momentum_at="update", attack=STEP_NAME[attack], attack_factor=2,
                           attack_evals=evals, nb_past=0, aggregator=ShardedAggregator(backend=OracleBackend()))
    assert torch.equal(none.run([g.clone() for g in rows]), O.median(rows)) and none.last_byzantine is None
    assert math.isnan(none.floats()["attack_norm_avg"])


def test_torch_leg_keeps_the_sign_of_zero_and_reads_a_tensor_factor():
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from tests.sharded_backend import OracleBackend
  agg = ShardedAggregator(backend=OracleBackend())
  avg = torch.tensor([1.0, -0.0, 3.0, -0.0])
  got, direction = agg.attack_vector("shift_one", avg, 2.0, target_idx=-4, want_direction=True)
  assert torch.equal(got, torch.tensor([3.0, 0.0, 3.0, 0.0])) and not bool(torch.signbit(got).any())
  assert torch.equal(direction, torch.tensor([1.0, 0.0, 0.0, 0.0]))
  got = agg.attack_vector("shift_one", avg, -2.0, target_idx=2)
  assert torch.equal(got, torch.tensor([1.0, -0.0, 1.0, -0.0])) and torch.signbit(got).tolist() == [False, True, False, True]
  third = torch.tensor([1.0 / 3.0, 7.0], dtype=torch.float64)   # rounded to fp32 before it meets the vector
  assert same_bits(agg.attack_vector("scale", avg, third), avg * torch.tensor(1.0 / 3.0).float())
  assert same_bits(agg.attack_vector("shift_all", avg, third), avg + torch.tensor(1.0 / 3.0).float())
  nan = agg.attack_vector("nan", avg)
  assert bool((nan.view(torch.int32) == 0x7FC00000).all()) and nan.data_ptr() != avg.data_ptr()


# ---------------------------------------------------------------------------- #
# Two gloo ranks, each holding a slice of the coordinates

def _free_port():
  with socket.socket() as s:
    s.bind(("127.0.0.1", 0))
    return s.getsockname()[1]


D_SHARDED = 100   # slices [0, 64) and [64, 100)
SHARDED = [("bulyan", 1.5, {"target_idx": 63}), ("bulyan", 1.5, {"target_idx": 64}), ("bulyan", -2.0, {"target_idx": -1}),
           ("bulyan", 0.75, {"target_idx": "all"}), ("empire-strict", 2, None), ("nan", 1.1, None)]


def _sharded_case(ci, aggregator, shard):
  """(the whole Byzantine vector, the study row) of two steps of case `ci` over `aggregator`."""
  attack, factor, args = SHARDED[ci]
  step = make_step(attack, "median", "worker", factor, args, aggregator=aggregator)
  out = []
  for it in range(2):
    rows = R.sampled_for_step(it, N - F, D_SHARDED)
    step.run(shard(rows))
    out.append((aggregator.all_gather_output(step.last_byzantine, D_SHARDED).numpy().copy(), dict(step.floats())))
  return out


def _worker(rank, world, port, queue):
  os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
  dist.init_process_group("gloo", rank=rank, world_size=world)
  try:
    from byzantinemomentum_amd import sharded
    from tests.sharded_backend import OracleBackend
    assert sharded.shard_bounds(D_SHARDED, world, rank) == ((0, 64), (64, 100))[rank]
    out = {}
    for ci in range(len(SHARDED)):
      agg = sharded.ShardedAggregator(backend=OracleBackend())
      assert agg.collective
      out[ci] = _sharded_case(ci, agg, lambda rows: agg.shard_rows([g.clone() for g in rows]))
    queue.put((rank, out))
    dist.barrier()
  finally:
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_sharded_attacks_match_single_process():
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from tests.sharded_backend import OracleBackend
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
  for ci in range(len(SHARDED)):
    single = _sharded_case(ci, ShardedAggregator(backend=OracleBackend()), lambda rows: [g.clone() for g in rows])
    for r in range(world):
      for it, ((vector, floats), (want_vector, want_floats)) in enumerate(zip(results[r][ci], single)):
        assert same_bits(torch.from_numpy(vector), torch.from_numpy(want_vector)), (SHARDED[ci], r, it)
        assert set(floats) == set(want_floats)
        for key, want in want_floats.items():   # (fp64 sums over two slices: the last places may differ)
          got = floats[key]
          assert (math.isnan(got) and math.isnan(want)) or abs(got - want) <= 1e-12 * max(abs(want), 1.0), (ci, r, it, key)
