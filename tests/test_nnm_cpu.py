"""Nearest-neighbour mixing without a GPU: the host form of the neighbour masks against a numpy restatement of the
contract on crafted matrices, the plain-torch legs of ShardedAggregator.nnm (bit for bit against the float32 numpy loop;
against a float64 pipeline on one rank and on the gloo world of two), header and library, the plugin names."""

import ctypes
import math
import os
import re
import socket
import sys
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import nnm_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("bm_nnm_masks", "bm_nnm_masks_device", "bm_mix_rows", "bm_colwise_mixed", "bm_colwise_mixed_max_rows")


@pytest.fixture(scope="module")
def bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


# ---------------------------------------------------------------------------- #
# 1. bm_nnm_masks

@pytest.mark.parametrize("case", nc.mask_cases(), ids=lambda c: c[0])
def test_host_masks_follow_the_contract(bm, case):
  name, sq, n, f = case
  got = bm.gars.nnm_masks(torch.from_numpy(np.ascontiguousarray(sq)), n, f)
  assert got.dtype == torch.int64 and got.shape == (nc.MAX_ROWS,) and not got.is_cuda
  words = nc.from_int64(got.tolist())
  assert words[:n] == nc.masks_reference(sq, n, f), name
  assert words[n:] == [0] * (nc.MAX_ROWS - n)
  for i in range(n):
    assert (words[i] >> i) & 1 and bin(words[i]).count("1") == n - f      # row i itself, n - f rows in all


def test_masks_spelled_out():
  """The restatement itself on a matrix small enough to read: ties to the lower index, NaN last, +inf before NaN."""
  nan, inf = math.nan, math.inf
  sq = np.array([[9.0, 1.0, 1.0, nan, inf],
                 [1.0, 0.0, 2.0, 2.0, 2.0],
                 [nan, nan, nan, nan, nan],
                 [5.0, 4.0, 3.0, 0.0, 3.0],
                 [inf, nan, 7.0, nan, 0.0]])
  assert nc.masks_reference(sq, 5, 2) == [0b00111, 0b00111, 0b00111, 0b11100, 0b10101]
  assert nc.masks_reference(sq, 5, 1) == [0b10111, 0b01111, 0b01111, 0b11110, 0b10111]


def test_full_and_self_only_masks(bm):
  sq = torch.rand(11, 11, dtype=torch.float64)
  assert nc.from_int64(bm.gars.nnm_masks(sq, 11, 0).tolist())[:11] == [(1 << 11) - 1] * 11
  assert nc.from_int64(bm.gars.nnm_masks(sq, 11, 10).tolist())[:11] == [1 << i for i in range(11)]
  assert nc.from_int64(bm.gars.nnm_masks(torch.full((1, 1), math.nan, dtype=torch.float64), 1, 0).tolist())[0] == 1
  assert nc.from_int64(bm.gars.nnm_masks(torch.zeros(64, 64, dtype=torch.float64), 64, 0).tolist()) == [(1 << 64) - 1] * 64


def test_refused_arguments(bm):
  lib = bm._lib.load()
  sq = (ctypes.c_double * (64 * 64))()
  masks = (ctypes.c_uint64 * 64)()
  rows = (ctypes.c_void_p * 64)()
  for n, f in nc.REFUSED:
    assert lib.bm_nnm_masks(sq, n, f, masks) == bm._lib.EINVAL, (n, f)
    assert lib.bm_nnm_masks_device(sq, n, f, masks, None) == bm._lib.EINVAL, (n, f)    # before any HIP call
    if n >= 1:
      with pytest.raises(bm.gars.GarInputError):
        bm.gars.nnm_masks(torch.zeros(64, 64, dtype=torch.float64), n, f)
  assert lib.bm_nnm_masks(None, 11, 2, masks) == bm._lib.EINVAL
  assert lib.bm_nnm_masks(sq, 11, 2, None) == bm._lib.EINVAL
  assert lib.bm_nnm_masks_device(None, 11, 2, masks, None) == bm._lib.EINVAL
  with pytest.raises(bm.gars.GarInputError):
    bm.gars.nnm_masks(torch.zeros(11, 11, dtype=torch.float32), 11, 2)
  with pytest.raises(bm.gars.GarInputError):
    bm.gars.nnm_masks(torch.zeros(10, 10, dtype=torch.float64), 11, 2)
  # the d-sized entry points: refused before any HIP call as well
  assert lib.bm_mix_rows(rows, 0, masks, 1, 10, rows, None) == bm._lib.EINVAL          # n < 1
  assert lib.bm_mix_rows(rows, 65, masks, 1, 10, rows, None) == bm._lib.EINVAL         # n > BM_MAX_ROWS
  assert lib.bm_mix_rows(rows, 11, masks, 0, 10, rows, None) == bm._lib.EINVAL         # no output row
  assert lib.bm_mix_rows(rows, 11, masks, 65, 10, rows, None) == bm._lib.EINVAL
  assert lib.bm_mix_rows(rows, 11, None, 11, 10, rows, None) == bm._lib.EINVAL         # no masks
  assert lib.bm_mix_rows(rows, 11, masks, 11, -1, rows, None) == bm._lib.EINVAL
  assert lib.bm_mix_rows(rows, 11, masks, 11, 10, rows, None) == bm._lib.EINVAL        # null rows (the table is empty)
  assert lib.bm_mix_rows(rows, 11, masks, 11, 0, rows, None) == 0                      # empty vectors: nothing to do
  limit = lib.bm_colwise_mixed_max_rows()
  assert 25 <= limit <= nc.MAX_ROWS
  op_median, op_trmean, op_phocas = bm._lib.OP_MEDIAN, bm._lib.OP_TRMEAN, bm._lib.OP_PHOCAS
  assert lib.bm_colwise_mixed(op_median, rows, limit + 1, masks, 10, 0, rows, None) == bm._lib.EINVAL
  assert lib.bm_colwise_mixed(op_median, rows, 0, masks, 10, 0, rows, None) == bm._lib.EINVAL
  assert lib.bm_colwise_mixed(op_phocas, rows, 11, masks, 10, 2, rows, None) == bm._lib.EINVAL     # no such fused rule
  assert lib.bm_colwise_mixed(7, rows, 11, masks, 10, 2, rows, None) == bm._lib.EINVAL
  assert lib.bm_colwise_mixed(op_trmean, rows, 11, masks, 10, 6, rows, None) == bm._lib.EINVAL     # n < 2 f + 1
  assert lib.bm_colwise_mixed(op_trmean, rows, 11, masks, 10, -1, rows, None) == bm._lib.EINVAL
  assert lib.bm_colwise_mixed(op_trmean, rows, 11, None, 10, 2, rows, None) == bm._lib.EINVAL
  assert lib.bm_colwise_mixed(op_trmean, rows, 11, masks, 10, 2, rows, None) == bm._lib.EINVAL     # null rows
  assert lib.bm_colwise_mixed(op_trmean, rows, 11, masks, 0, 2, None, None) == 0


def test_python_layer_refuses_before_the_gpu(bm):
  cpu = [torch.zeros(4) for _ in range(3)]
  with pytest.raises(bm.gars.GarInputError):
    bm.nnm(cpu, 1)                                    # CPU tensors: there is no fallback
  with pytest.raises(ValueError):
    bm.nnm(cpu, 1, rule="mode")                       # unknown rule, said before anything else
  with pytest.raises(ValueError):
    bm.bucketing(cpu, 2, "mode")
  assert bm.nnm is bm.gars.nnm and bm.bucketing is bm.gars.bucketing
  assert bm.gars.bucket_masks(5, 2, [4, 0, 2, 1, 3]) == [0b10001, 0b00110, 0b01000]
  assert bm.gars.bucket_masks(4, 1, [0, 1, 2, 3]) == [1, 2, 4, 8]


# ---------------------------------------------------------------------------- #
# 2. The plain-torch legs

@pytest.mark.parametrize("n,d", [(1, 5), (7, 1027), (25, 130), (64, 33)])
def test_torch_mixing_is_the_float32_loop(n, d):
  from byzantinemomentum_amd.torch_legs import _mix_rows_torch, _nnm_masks_torch
  rows = nc.random_rows(n, d, seed=n)
  if n >= 7:
    rows[2] = np.full(d, np.nan, dtype=np.float32)
    rows[3] = np.full(d, np.inf, dtype=np.float32)
  masks = nc.random_masks(n, n, seed=d) + [0]
  if n >= 7:
    masks[0] &= ~0b1100          # the NaN and the inf row excluded: that output stays finite
    masks[0] |= 1
  got = _mix_rows_torch([torch.from_numpy(r) for r in rows], torch.tensor(nc.to_int64(masks)), len(masks))
  want = nc.mix_reference(rows, masks)
  for r, (g, w) in enumerate(zip(got, want)):
    assert nc.same_bits(g.numpy(), w), r
  assert np.isnan(got[-1].numpy()).all()                                   # the empty mask
  if n >= 7:
    assert np.isfinite(got[0].numpy()).all()
  for f in nc.f_values(n):
    sq = nc.sqdist64([r for r in nc.random_rows(n, 16, seed=f)])
    words = nc.from_int64(_nnm_masks_torch(torch.from_numpy(sq), n, f).tolist())
    assert words[:n] == nc.masks_reference(sq, n, f) and not any(words[n:])


@pytest.mark.parametrize("case", [c for c in nc.mask_cases() if c[2] <= 25], ids=lambda c: c[0])
def test_torch_masks_follow_the_contract(case):
  from byzantinemomentum_amd.torch_legs import _nnm_masks_torch
  name, sq, n, f = case
  words = nc.from_int64(_nnm_masks_torch(torch.from_numpy(np.ascontiguousarray(sq)), n, f).tolist())
  assert words[:n] == nc.masks_reference(sq, n, f), name


N, F, D = 11, 2, 1000


def _pipeline64(rows, f, rule):
  """Distances, neighbours, mixing and rule in float64 on the vectors."""
  n = len(rows)
  masks = nc.masks_reference(nc.sqdist64(rows), n, f)
  mixed, _ = nc.mix_reference64(rows, masks)
  y = np.stack(mixed)
  if rule == "median":
    return np.sort(y, axis=0)[(n - 1) // 2]
  if rule == "trmean":
    return np.sort(y, axis=0)[f:n - f].mean(axis=0)
  sq = nc.sqdist64(mixed)
  dist = np.sqrt(sq)
  scores = [np.sort(np.delete(dist[i], i))[:n - f - 1].sum() for i in range(n)]
  order = np.argsort(np.array(scores), kind="stable")[:n - f - 2]
  return y[order].mean(axis=0)


def _close(got, want):
  # float32 sums of at most 11 values of size O(1), mixed twice (neighbours, rule): a few units of 2^-24 of the scale
  return np.abs(got.astype(np.float64) - want).max() <= 64 * nc.U * max(1.0, np.abs(want).max())


def test_sharded_nnm_on_one_rank_without_capabilities():
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from tests.sharded_backend import OracleBackend
  rows = nc.ladder_rows(N, D, 1.3, seed=1)
  local = [torch.from_numpy(r) for r in rows]
  agg = ShardedAggregator(backend=OracleBackend(), local_only=True)
  for rule in ("trmean", "median", "krum"):
    out = agg.nnm(local, F, rule=rule)
    assert out.dtype == torch.float32 and _close(out.numpy(), _pipeline64(rows, F, rule)), rule
    assert nc.from_int64(agg.last_masks.tolist())[:N] == nc.masks_reference(nc.sqdist64(rows), N, F)
  with pytest.raises(ValueError):
    agg.nnm(local, F, rule="mode")
  with pytest.raises(ValueError):
    agg.nnm(local, N, rule="median")


def _free_port():
  with socket.socket() as s:
    s.bind(("127.0.0.1", 0))
    return s.getsockname()[1]


def _worker(rank, world, port, queue):
  os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
  dist.init_process_group("gloo", rank=rank, world_size=world)
  try:
    from byzantinemomentum_amd.sharded import ShardedAggregator, shard_bounds
    from tests.sharded_backend import OracleBackend
    rows = nc.ladder_rows(N, D, 1.3, seed=1)
    lo, hi = shard_bounds(D, world, rank)
    local = [torch.from_numpy(r[lo:hi].copy()) for r in rows]
    agg = ShardedAggregator(backend=OracleBackend())
    res = {rule: agg.all_gather_output(agg.nnm(local, F, rule=rule), D).numpy().copy() for rule in ("trmean", "median", "krum")}
    res["masks"] = agg.last_masks.numpy().copy()
    queue.put((rank, res))
    dist.barrier()
  finally:
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sharded_nnm_on_the_gloo_world_of_two():
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
  rows = nc.ladder_rows(N, D, 1.3, seed=1)
  for r in range(world):
    # the neighbours are those of the WHOLE vectors, the same on every rank
    assert nc.from_int64(results[r]["masks"].tolist())[:N] == nc.masks_reference(nc.sqdist64(rows), N, F)
    for rule in ("trmean", "median", "krum"):
      assert results[r][rule].shape == (D,) and _close(results[r][rule], _pipeline64(rows, F, rule)), (r, rule)


# ---------------------------------------------------------------------------- #
# 3. Header and library

def test_header_declares_and_library_exports_the_five(bm):
  text = open(os.path.join(ROOT, "include", "bm_gar.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  declared = set(re.findall(r"\b(bm_[a-z0-9_]+)\s*\(", text))
  lib = bm._lib.load()
  for name in NEW_NAMES:
    assert name in declared and name in bm._lib.SIGNATURES and hasattr(lib, name), name
  assert bm._lib.ABI_VERSION == 23 and lib.bm_abi_version() == 23


# ---------------------------------------------------------------------------- #
# 5. The plugin names

def test_register_nnm_rules_with_a_stub_registry():
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
    assert not any(name.startswith("native-nnm-") for name in at_import)       # not at import
    names = native.register_nnm_rules()
    from byzantinemomentum_amd import gars
    assert names == ["native-nnm-" + rule for rule in gars.NNM_RULES]
    assert native.register_nnm_rules() == names                                # twice: the same, registered once
    assert set(pkg.gars) == at_import | set(names)
    for name in names:
      rule = pkg.gars[name]
      assert rule.influence is None
      assert rule.check(gradients=[], f=1) is not None and rule.check(gradients=[1, 2, 3], f=1) is None
    with pytest.raises(GarInputErrorOrValue):
      pkg.gars["native-nnm-krum"].unchecked(gradients=[torch.zeros(4)] * 5, f=1)     # CPU tensors reach gars.nnm
    del sys.modules["aggregators"]
    with pytest.raises(RuntimeError):
      native.register_nnm_rules()                                              # no registry imported
  finally:
    for k, v in saved.items():
      if v is None:
        sys.modules.pop(k, None)
      else:
        sys.modules[k] = v


GarInputErrorOrValue = ValueError   # GarInputError is a ValueError
