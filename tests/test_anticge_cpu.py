"""The `anticge` attack (attacks/anticge.py:49-78) without a GPU: the restatements the other tests compare with against
the committed outputs of the reference (and the live reference where its checkout is staged), the argument checks of
the three C entry points, AggregationStep(attack="anticge") on the oracle-backed legs, and the sharded attack over two
gloo ranks.

A deviation from the issue that asked for these tests: it wants `last_byzantine` of the step on the oracle-backed legs
to EQUAL the f32 restatement.  That cannot hold bit for bit with the design the same issue sets: the step's scalars are
the backend's float64 `row_sqnorms` rounded to fp32 (what makes the two small collectives possible), the restatement's
are torch's fp32 `norm()`, and the two differ by an ulp in some cases (vectors up to 2.0e-7 of max|want| apart, equal
bits in 10 of the 18 steps below).  test_step_matches_the_restatement therefore pins the unscaled sum bit for bit (the
vector is `sum * m` for one fp32 number m), m within 1e-6 of the restatement's, and the vector within 1e-6 of max|want|
of the float64 restatement."""

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
from tests import anticge_reference as A
from tests.golden_io import same_bits
from tests.step_reference import assert_floats_close


@pytest.mark.parametrize("name", A.CASES)
def test_f32_restatement_is_the_reference_bit_for_bit(name):
  fx = A.Fixture(name)
  got = A.anticge_f32(fx.honests, fx.f_decl, fx.f_real)
  assert got.order == fx.order
  assert same_bits(got.vector, fx.vector)
  if fx.f_real > fx.f_decl:
    assert bool(torch.isnan(fx.vector).all())
  else:
    assert A.norm_gap(fx.honests) >= A.MIN_NORM_GAP
  if reference_loader.available():
    kept = [g.clone() for g in fx.honests]
    live = A.reference_attack()(grad_honests=fx.honests, f_decl=fx.f_decl, f_real=fx.f_real)
    assert len(live) == fx.f_real and all(v is live[0] for v in live) and all(live[0] is not g for g in fx.honests)
    assert same_bits(live[0], got.vector)
    assert all(torch.equal(a, b) for a, b in zip(kept, fx.honests))
    if fx.order is not None:
      assert A.reference_order(fx.honests) == got.order


@pytest.mark.parametrize("name", [c for c in A.CASES if c not in ("hetero_n7_freal2",)])
def test_f64_restatement_is_within_the_fp32_tolerance_of_the_reference(name):
  """(measured when the fixtures were made: at most 2.2e-7 of max|want|)"""
  fx = A.Fixture(name)
  got = A.anticge_f64(fx.honests, fx.f_decl, fx.f_real)
  assert got.order == fx.order
  err = float((got.vector - fx.vector.double()).abs().max())
  print(f"{name}: f64 restatement - reference = {err / float(fx.vector.abs().max()):.3e} of max|want|")
  assert err <= 1e-6 * float(fx.vector.abs().max())


def test_f64_restatement_of_the_nan_case():
  fx = A.Fixture("hetero_n7_freal2")
  assert bool(torch.isnan(A.anticge_f64(fx.honests, fx.f_decl, fx.f_real).vector).all())


def test_restatements_check_f_decl():
  rows = [torch.ones(4), torch.full((4,), 2.0)]
  for fn in (A.anticge_f32, A.anticge_f64):
    for f_decl in (0, 3):
      with pytest.raises(ValueError):
        fn(rows, f_decl, 0)
    assert torch.equal(fn(rows, 2, 1).sum.float(), rows[0])                   # maxpos = 0: the smallest row once
    assert torch.equal(fn(rows, 1, 1).sum.float(), rows[0] + rows[0])         # maxpos = 1: the smallest row twice


# ---------------------------------------------------------------------------- #
# The C ABI, no GPU: bad arguments are refused before any HIP call

def test_entry_points_validate_arguments_without_gpu():
  from byzantinemomentum_amd import build, _lib
  build.build()
  lib = _lib.load()
  rows = (ctypes.c_void_p * 64)()          # a table of null row pointers
  full = (ctypes.c_void_p * 64)(*([ctypes.addressof(rows)] * 64))  # non-null entries (never dereferenced)
  buf = (ctypes.c_double * 64)()
  ws = (ctypes.c_double * 64)()
  out = (ctypes.c_float * 16)()
  call = lib.bm_anticge_sum
  assert call(full, 0, 10, 1, buf, out, None, buf, ws, None) == _lib.EINVAL       # h < 1
  assert call(full, 65, 10, 1, buf, out, None, buf, ws, None) == _lib.EINVAL      # h > BM_MAX_ROWS
  assert call(full, 9, 10, 0, buf, out, None, buf, ws, None) == _lib.EINVAL       # f_decl < 1
  assert call(full, 9, 10, 10, buf, out, None, buf, ws, None) == _lib.EINVAL      # f_decl > h
  assert call(None, 9, 10, 2, buf, out, None, buf, ws, None) == _lib.EINVAL       # no rows
  assert call(rows, 9, 10, 2, buf, out, None, buf, ws, None) == _lib.EINVAL       # a null row
  assert call(full, 9, 10, 2, None, out, None, buf, ws, None) == _lib.EINVAL      # no squared norms
  assert call(full, 9, 10, 2, buf, None, None, buf, ws, None) == _lib.EINVAL      # nowhere to write the sum
  assert call(full, 9, 10, 2, buf, out, None, None, ws, None) == _lib.EINVAL      # nowhere to write the scalars
  assert call(full, 9, 10, 2, buf, out, None, buf, None, None) == _lib.EINVAL     # no workspace
  assert call(full, 9, -1, 2, buf, out, None, buf, ws, None) == _lib.EINVAL       # d < 0
  scale = lib.bm_anticge_scale
  assert scale(None, 10, buf, None) == _lib.EINVAL                                # no vector
  assert scale(out, 10, None, None) == _lib.EINVAL                                # no scalars
  assert scale(out, -1, buf, None) == _lib.EINVAL                                 # d < 0
  assert scale(None, 0, buf, None) == 0                                           # an empty shard: nothing to do
  assert lib.bm_anticge_workspace_bytes(-1) == _lib.EINVAL
  small, long = lib.bm_anticge_workspace_bytes(0), lib.bm_anticge_workspace_bytes((1 << 29) + 1)
  assert small >= 64 * 4 + 8 and long > small and lib.bm_anticge_workspace_bytes(1 << 29) == small
  assert lib.bm_abi_version() == 23


def test_signatures_still_mirror_the_header():
  from byzantinemomentum_amd import _lib
  from tests.test_abi import declared_functions
  names = declared_functions()
  assert sorted(_lib.SIGNATURES) == names
  assert {"bm_anticge_workspace_bytes", "bm_anticge_sum", "bm_anticge_scale"} <= set(names)


# ---------------------------------------------------------------------------- #
# AggregationStep(attack="anticge") on the oracle-backed legs

N, F, D = 11, 2, 257


def make_step(gar, momentum_at, aggregator=None, clip=None, n=N, f=F):
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from byzantinemomentum_amd.step import AggregationStep
  from tests.sharded_backend import OracleBackend
  agg = aggregator or ShardedAggregator(backend=OracleBackend())
  return AggregationStep(n, f, f, gar=gar, momentum=0.9, dampening=0.9, momentum_at=momentum_at, attack="anticge",
                         attack_factor=123.0, nb_past=3, gradient_clip=clip, aggregator=agg)


@pytest.mark.parametrize("momentum_at,gar", list(itertools.product(("worker", "server", "update"), ("cge", "krum", "median"))))
def test_step_matches_the_restatement(momentum_at, gar):
  """The scalars of the step's attack are float64 squared norms rounded to fp32, the restatement's are torch's fp32
  `norm()`: the two multipliers may differ in their last places (measured on these cases: the vectors differ by at most
  2.0e-7 of max|want|, and are the same bits in 10 of the 18 steps).  So: the unscaled sum is the restatement's bit for
  bit — the vector is `sum * m` for ONE fp32 number m — and m is the restatement's within the 1e-6 the project allows an
  fp32 arithmetic output."""
  assert not dist.is_initialized()
  h = N - F
  step = make_step(gar, momentum_at)
  assert step.plan.first_pass == "plain" and step.plan.search is None and not step.plan.single_call
  loop = A.AnticgeLoop(N, F, F, gar, momentum_at)
  for it in range(2):
    sampled = A.sampled_for_step(it, h, D)
    honests, want = loop.begin(sampled)
    assert A.norm_gap(honests) >= A.MIN_NORM_GAP
    got_def = step.run([g.clone() for g in sampled])
    byz = step.last_byzantine
    assert all(byz.data_ptr() != g.data_ptr() for g in sampled) and byz.data_ptr() != got_def.data_ptr()
    m = A.multiplier_of(byz, want.sum)
    m_want = A.multiplier_of(want.vector, want.sum)
    assert m is not None and m_want is not None, (momentum_at, gar, it)
    print(f"{momentum_at}-{gar} step {it}: multiplier {m!r} against {m_want!r}")
    assert abs(m - m_want) <= 1e-6 * abs(m_want)
    assert float((byz.double() - A.anticge_f64(honests, F, F).vector).abs().max()) <= 1e-6 * float(want.vector.abs().max())
    want_def, want_upd, floats = loop.finish(byz)
    assert torch.equal(got_def, want_def), (momentum_at, gar, it)
    assert torch.equal(step.update_gradient(), want_upd)
    got = step.floats()
    assert abs(got["attack_norm_avg"] - floats["attack_norm_avg"]) <= 1e-5 * floats["attack_norm_avg"]
    assert_floats_close(got, floats, tag=(momentum_at, gar, it), tol=1e-5)


def test_step_with_clipping_and_more_byzantine_workers_than_declared():
  step = make_step("median", "worker", clip=19.0)  # (clips the two largest rows: the selected ones keep distinct norms)
  loop = A.AnticgeLoop(N, F, F, "median", "worker", clip=19.0)
  sampled = A.sampled_for_step(0, N - F, D)
  honests, want = loop.begin(sampled)
  got_def = step.run([g.clone() for g in sampled])
  # (the clipping factor is an fp32 number on the step's side, a double on the loop's: rows equal to a rounding only)
  assert float((step.last_byzantine - want.vector).abs().max()) <= 2e-6 * float(want.vector.abs().max())
  assert float((got_def - loop.finish(step.last_byzantine)[0]).abs().max()) <= 2e-6 * float(torch.stack(sampled).abs().max())
  # f_real > f_decl: the all-NaN vector of anticge.py:60-63 reaches the rule
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from byzantinemomentum_amd.step import AggregationStep
  from tests.sharded_backend import OracleBackend
  nan_step = AggregationStep(11, 1, 2, gar="median", momentum_at="update", attack="anticge", nb_past=0,
                             aggregator=ShardedAggregator(backend=OracleBackend()))
  nan_step.run(A.sampled_for_step(0, 9, D))
  assert bool(torch.isnan(nan_step.last_byzantine).all())
  # no Byzantine worker: no attack, whatever f_decl is
  none = AggregationStep(9, 0, 0, gar="median", momentum_at="update", attack="anticge", nb_past=0,
                         aggregator=ShardedAggregator(backend=OracleBackend()))
  rows = A.sampled_for_step(0, 9, D)
  assert torch.equal(none.run([g.clone() for g in rows]), O.median(rows)) and none.last_byzantine is None


def test_step_rejects_bad_arguments():
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from byzantinemomentum_amd.step import AggregationStep
  from tests.sharded_backend import OracleBackend
  agg = ShardedAggregator(backend=OracleBackend())
  with pytest.raises(ValueError, match="attack_evals"):
    AggregationStep(11, 2, 2, attack="anticge", attack_evals=4, aggregator=agg)
  with pytest.raises(ValueError, match="nb_decl_byz"):
    AggregationStep(11, 0, 2, attack="anticge", aggregator=agg)       # f_decl < 1
  with pytest.raises(ValueError, match="nb_decl_byz"):
    AggregationStep(11, 10, 2, attack="anticge", aggregator=agg)      # f_decl > h = 9
  AggregationStep(11, 9, 2, attack="anticge", aggregator=agg)         # f_decl = h
  with pytest.raises(ValueError, match="unknown attack"):
    AggregationStep(11, 2, 2, attack="bulyan", aggregator=agg)
  rows = A.sampled_for_step(0, 9, 64)
  assert agg.anticge(rows, 2, 0) == []
  with pytest.raises(ValueError):
    agg.anticge(rows, 10, 1)                                           # f_decl > h
  assert bool(torch.isnan(agg.anticge(rows, 0, 1)[0]).all())           # f_real > f_decl comes first, as in the reference


# ---------------------------------------------------------------------------- #
# Two gloo ranks, each holding a slice of the coordinates

def _free_port():
  with socket.socket() as s:
    s.bind(("127.0.0.1", 0))
    return s.getsockname()[1]


SHARDED = [("hetero", 11, 2, 1000, 2), ("momentum", 25, 5, 130, 5), ("hetero", 7, 1, 40, 6)]  # kind, n, f, d, f_decl


class _Counting:
  """ShardedAggregator whose all-reduces are counted, with their sizes."""

  @staticmethod
  def make(backend):
    from byzantinemomentum_amd.sharded import ShardedAggregator

    class Counting(ShardedAggregator):
      def _all_reduce(self, tensor, op=None):
        self.reduced = getattr(self, "reduced", []) + [int(tensor.numel())]
        return super()._all_reduce(tensor, op)
    return Counting(backend=backend)


def _worker(rank, world, port, queue):
  os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
  dist.init_process_group("gloo", rank=rank, world_size=world)
  try:
    from byzantinemomentum_amd import sharded, torch_legs
    from tests.sharded_backend import OracleBackend
    out = {}
    for ci, (kind, n, f, d, f_decl) in enumerate(SHARDED):
      rows, h = O.make_stack(kind, n, f, d, seed=3)
      lo, hi = sharded.shard_bounds(d, world, rank)
      local = [g[lo:hi].clone() for g in rows[:h]]
      agg = _Counting.make(OracleBackend())
      assert agg.collective
      sq = agg._all_reduce(agg.backend.row_sqnorms(local))
      total, _, _ = torch_legs._anticge_sum_torch(agg.backend, local, f_decl, sq)   # the unscaled sum of this slice
      agg.reduced = []
      res = agg.anticge(local, f_decl, f)
      assert len(res) == f and all(r is res[0] for r in res) and all(res[0] is not g for g in local)
      out[ci] = (agg.all_gather_output(total, d).numpy().copy(), agg.all_gather_output(res[0], d).numpy().copy(),
                 list(agg.reduced))
    queue.put((rank, out))
    dist.barrier()
  finally:
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_sharded_attack_matches_single_process():
  """d = 130: the second rank's shard is short; d = 40: it is EMPTY (it still enters both collectives)."""
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
  for ci, (kind, n, f, d, f_decl) in enumerate(SHARDED):
    rows, h = O.make_stack(kind, n, f, d, seed=3)
    honests = rows[:h]
    assert A.norm_gap(honests) >= A.MIN_NORM_GAP
    single = _Counting.make(OracleBackend())
    single.reduced = []
    want = single.anticge(honests, f_decl, f)[0]
    assert single.reduced == [h, 1] and not single.collective   # (counted, never issued: one rank)
    f32 = A.anticge_f32(honests, f_decl, f)
    assert A.multiplier_of(want, f32.sum) is not None
    for r in range(world):
      total, vector, reduced = results[r][ci]
      assert torch.equal(torch.from_numpy(total), f32.sum), (ci, r)          # the unscaled sum: bit for bit
      err = float((torch.from_numpy(vector) - want).abs().max())
      assert err <= 1e-6 * float(want.abs().max()), (ci, r, err)
      assert reduced == [h, 1]                                               # two small collectives, never a d-sized one
    assert (results[0][ci][1] == results[1][ci][1]).all()                    # every rank holds the same vector
