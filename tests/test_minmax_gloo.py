"""ShardedAggregator.minmax over two gloo ranks, each holding a slice of the coordinates (oracle-backed backend: the
plain-torch fp64 legs).  Both ranks get the factor of the unsharded call to 1e-12 — the distances and the scalars are
sums over coordinates, added over the ranks by ONE all-reduce of h^2 + PERTURB_SLOTS doubles — and the gathered vector is
the unsharded one."""

import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import minmax_reference as R

CASES = [(9, 1000, "common", "minmax", "std"), (20, 130, "iid", "minsum", "unit"), (5, 7, "scaled", "minmax", "sign"),
         (3, 1, "iid", "minsum", "sign")]   # d = 130: the second shard is short; d = 1: it is EMPTY
F_REAL = 2


def _free_port():
  with socket.socket() as s:
    s.bind(("127.0.0.1", 0))
    return s.getsockname()[1]


def _rows(h, d, structure):
  return [torch.from_numpy(r.astype(np.float32)) for r in R.stack(h, d, structure, 8)]


def _counting(backend):
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
    from byzantinemomentum_amd import sharded
    from tests.sharded_backend import OracleBackend
    out = {}
    for ci, (h, d, structure, mode, perturbation) in enumerate(CASES):
      lo, hi = sharded.shard_bounds(d, world, rank)
      local = sharded.Shards([g[lo:hi].clone() for g in _rows(h, d, structure)], d_total=d)
      agg = _counting(OracleBackend())
      assert agg.collective
      agg.reduced = []
      res = agg.minmax(local, F_REAL, mode, perturbation)
      assert len(res) == F_REAL and all(r is res[0] for r in res) and all(res[0] is not g for g in local)
      reduced = list(agg.reduced)
      out[ci] = (res[0].attack_info.numpy().copy(), agg.all_gather_output(res[0], d).numpy().copy(), reduced)
    queue.put((rank, out))
    dist.barrier()
  finally:
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_sharded_attack_matches_the_unsharded_call():
  from byzantinemomentum_amd import _lib
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
  for ci, (h, d, structure, mode, perturbation) in enumerate(CASES):
    rows = _rows(h, d, structure)
    single = _counting(OracleBackend())
    single.reduced = []
    want = single.minmax(rows, F_REAL, mode, perturbation)[0]
    assert single.reduced == [] and not single.collective          # no collective with one rank
    info = want.attack_info.numpy()
    assert info[5] == 0.0 and info[0] > 0.0
    for r in range(world):
      got_info, vector, reduced = results[r][ci]
      assert reduced == [h * h + _lib.PERTURB_SLOTS], (ci, r, reduced)  # ONE all-reduce, never a d-sized one
      assert abs(got_info[0] - info[0]) <= 1e-12 * info[0], (ci, r, got_info, info)
      assert got_info[2] == info[2] and got_info[5] == 0.0
      for slot in (1, 3, 4):
        assert abs(got_info[slot] - info[slot]) <= 1e-12 * abs(info[slot]), (ci, r, slot)
      # the vector: the same fp32 average and direction per coordinate, the factor rounded to fp32 — equal unless the
      # factors differ in their last bits
      err = np.abs(vector - want.numpy()).max()
      assert err <= 2.0 ** -22 * np.abs(want.numpy()).max(), (ci, r, err)
    assert (results[0][ci][0] == results[1][ci][0]).all()            # every rank holds the same numbers
