"""Nearest-neighbour mixing on the GPU: the device masks against the host form, bm_mix_rows bit for bit against the
float32 numpy loop of the contract (every row count class, vector width, tail, several workgroups, several pieces, NaN
and inf rows, aliased inputs), the fused median / trimmed mean against bm_colwise on the rows bm_mix_rows wrote,
gars.nnm end to end against numpy-mixed rows and against a float64 pipeline, bucketing, and a graph replay.
Needs an MI355X: `pytest -m gpu`."""

import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import nnm_cases as nc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1, 3, 1027, 3074)     # one lane; tail only; body + tail; several workgroups
OFFSETS = (0, 1, 2)              # floats behind a 16-byte boundary: 16 / 4 / 8-byte accesses
ROW_COUNTS = (1, 2, 7, 11, 25, 51, 64)


@pytest.fixture(scope="module")
def bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


def _upload(host, offset):
  """The rows cut from ONE allocation, every one starting `offset` floats behind a 256-byte boundary."""
  n, d = len(host), host[0].shape[0]
  per = -(-(d + offset) // 64) * 64
  pool = torch.zeros(n * per, dtype=torch.float32, device=DEV)
  dev = []
  for i, h in enumerate(host):
    view = pool[i * per + offset:i * per + offset + d]
    view.copy_(torch.from_numpy(h))
    dev.append(view)
  assert all(v.data_ptr() % 16 == 4 * offset for v in dev)
  return dev


def _masks(words):
  return torch.tensor(nc.to_int64(words), dtype=torch.int64, device=DEV)


@functools.lru_cache(maxsize=None)
def _rows(n, d):
  return tuple(nc.random_rows(n, d, seed=1000 * n + d))


@functools.lru_cache(maxsize=None)
def _mask_sets(n, d):
  """The mask sets one (n, d) is mixed with, each with its float32 reference — computed once, shared by the alignments:
  the neighbour masks of every f, random masks with an empty one and bits beyond n, bucket masks (n_out < n)."""
  rows = list(_rows(n, d))
  sq = nc.sqdist64(rows)
  sets = [(f"nnm-f{f}", nc.masks_reference(sq, n, f)) for f in nc.f_values(n)]
  rnd = nc.random_masks(n, min(n, 9), seed=n + d) + [0]
  if n < 64:
    rnd[0] |= 1 << n | 1 << 63      # bits at positions >= n are ignored
  sets.append(("random", rnd))
  if n >= 2:
    perm = np.random.default_rng(n).permutation(n).tolist()
    sets.append(("buckets", [sum(1 << j for j in perm[lo:lo + 2]) for lo in range(0, n, 2)]))
  visible = (1 << n) - 1
  return tuple((name, tuple(words), nc.mix_reference(rows, [w & visible for w in words]),
                nc.mix_reference64(rows, [w & visible for w in words])) for name, words in sets)


def _assert_mixed(got, want, want64, tag):
  for r, g in enumerate(got):
    g = g.cpu().numpy()
    assert nc.same_bits(g, want[r]), (tag, r, int(np.flatnonzero(g.view(np.uint32) != want[r].view(np.uint32))[0]))
    if want64 is not None:
      y64, bound = want64
      ok = np.isfinite(y64[r])
      assert (np.abs(g.astype(np.float64) - y64[r])[ok] <= bound[r][ok]).all(), (tag, r, "float64 bound")


# ---------------------------------------------------------------------------- #
# 6. masks

@pytest.mark.parametrize("case", nc.mask_cases(), ids=lambda c: c[0])
def test_device_masks_equal_host_masks(bm, case):
  name, sq, n, f = case
  host = torch.from_numpy(np.ascontiguousarray(sq))
  want = bm.gars.nnm_masks(host, n, f)
  got = bm.gars.nnm_masks(host.to(DEV), n, f)
  assert got.is_cuda and got.dtype == torch.int64 and got.shape == (nc.MAX_ROWS,)
  assert torch.equal(got.cpu(), want), name
  assert nc.from_int64(want.tolist())[:n] == nc.masks_reference(sq, n, f)


# ---------------------------------------------------------------------------- #
# 7. bm_mix_rows

@pytest.mark.parametrize("n", ROW_COUNTS)
def test_mix_rows_is_the_float32_loop(bm, n):
  for d in LENGTHS:
    host = list(_rows(n, d))
    for offset in OFFSETS:
      dev = _upload(host, offset)
      for name, words, want, want64 in _mask_sets(n, d):
        got = bm.gars.mix_rows(dev, _masks(words), len(words))
        assert len(got) == len(words) and all(g.shape == (d,) and g.dtype == torch.float32 for g in got)
        _assert_mixed(got, want, want64, (n, d, offset, name))
        if name == "random":
          assert torch.isnan(got[-1]).all()          # the empty mask: 0 / 0


@pytest.mark.parametrize("n", [7, 25, 51])
def test_nan_and_inf_rows_outside_a_mask_are_not_read(bm, n):
  d = 1027
  host = list(_rows(n, d))
  host[2] = np.full(d, np.nan, dtype=np.float32)
  host[4] = np.full(d, np.inf, dtype=np.float32)
  host[5] = host[5].copy()
  host[5][::7] = -np.inf                              # single coordinates as well
  words = nc.random_masks(n, n, seed=n)
  for r in range(0, n, 2):
    words[r] &= ~0b110100                             # rows 2, 4, 5 excluded: finite outputs
    words[r] |= 1
  words[1] |= 0b000100                                # the NaN row included
  words[3] = (words[3] | 0b010000) & ~0b100100        # the +inf row included, NaN and -inf excluded: +inf
  want = nc.mix_reference(host, words)
  for offset in OFFSETS:
    got = bm.gars.mix_rows(_upload(host, offset), _masks(words), n)
    _assert_mixed(got, want, None, (n, offset))
    for r in range(0, n, 2):
      assert torch.isfinite(got[r]).all(), r
    assert torch.isnan(got[1]).all() and (got[3] == float("inf")).all()


def test_tiny_sums_take_the_division_itself(bm):
  """Quotients in the subnormal range (and sums that are exactly zero): the bits of one IEEE division."""
  n, d = 7, 1027
  rng = np.random.default_rng(5)
  host = [(rng.normal(size=d) * 2.0 ** -124).astype(np.float32) for _ in range(n)]
  host[1] = -host[0]                                  # rows 0 and 1 cancel: +0
  words = [0b11, 0b1111111, 0b1010101, 0b0000100, 0b1111000]
  got = bm.gars.mix_rows(_upload(host, 0), _masks(words), len(words))
  _assert_mixed(got, nc.mix_reference(host, words), None, "tiny")
  assert not got[0].any() and not torch.signbit(got[0]).any()


@pytest.mark.parametrize("n,f", [(11, 3), (25, 5)])
def test_aliased_inputs(bm, n, f):
  d = 3074
  host = list(_rows(n, d))
  dev = _upload(host[:n - f + 1], 0)
  stack = dev[:n - f] + [dev[n - f]] * f              # the f copies of a Byzantine vector are one tensor
  hstack = host[:n - f] + [host[n - f]] * f
  words = nc.masks_reference(nc.sqdist64(hstack), n, f)
  got = bm.gars.mix_rows(stack, _masks(words), n)
  _assert_mixed(got, nc.mix_reference(hstack, words), nc.mix_reference64(hstack, words), ("aliased", n))


def test_outputs_may_not_alias(bm):
  lib = bm._lib.load()
  n, d = 5, 64
  pool = torch.zeros(16 * d, dtype=torch.float32, device=DEV)
  rows = [pool[i * d:(i + 1) * d] for i in range(n)]
  outs = [pool[(8 + i) * d:(9 + i) * d] for i in range(n)]
  masks = _masks([0b11111] * n)
  table = bm._lib.pointer_table

  def call(ins, os_):
    return lib.bm_mix_rows(table(ins), n, ctypes.c_void_p(masks.data_ptr()), n, d, table(os_), None)

  assert call(rows, [rows[2]] + outs[1:]) == bm._lib.EINVAL                      # an output is an input
  assert call(rows, [pool[4 * d + 8:5 * d + 8]] + outs[1:]) == bm._lib.EINVAL    # overlaps an input
  assert call(rows, [outs[1]] + outs[1:]) == bm._lib.EINVAL                      # two outputs are one
  assert call(rows, [pool[9 * d - 4:10 * d - 4]] + outs[1:]) == bm._lib.EINVAL   # two outputs overlap
  assert call([rows[0]] * n, outs) == 0                                          # inputs may
  torch.cuda.synchronize()


_PIECE_CHILD = r"""
import numpy as np, torch
from tests import nnm_cases as nc
from tests.test_gpu_nnm import _upload, _masks, _assert_mixed
import byzantinemomentum_amd as bm
n, f, d = 11, 2, 3074
host = nc.random_rows(n, d, seed=77)
words = nc.masks_reference(nc.sqdist64(host), n, f)
want = nc.mix_reference(host, words)
for offset in (0, 1, 2):
  dev = _upload(host, offset)
  _assert_mixed(bm.gars.mix_rows(dev, _masks(words), n), want, None, ("pieces", offset))
  for rule in ("median", "trmean"):
    fused = bm.gars.colwise_mixed(rule, dev, _masks(words), f)
    plain = getattr(bm.gars, rule)(bm.gars.mix_rows(dev, _masks(words), n), f=f)
    assert torch.equal(fused, plain), (rule, offset)
torch.cuda.synchronize()
print("pieces ok")
"""


def test_three_launch_pieces():
  """BM_WSUM_PIECE=1024 at d = 3074: three pieces (1024, 1024, 1026 columns) are walked, by bm_mix_rows and by the fused
  kernels; same bits as the float32 loop.  In a child process: the library reads the variable once."""
  env = dict(os.environ, BM_WSUM_PIECE="1024", PYTHONPATH=ROOT)
  run = subprocess.run([sys.executable, "-c", _PIECE_CHILD], capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
  assert run.returncode == 0, run.stderr[-2000:]
  assert run.stdout.strip().splitlines()[-1] == "pieces ok"


# ---------------------------------------------------------------------------- #
# 8. the fused kernels

def _fused_counts(bm):
  limit = bm._lib.load().bm_colwise_mixed_max_rows()
  return sorted({2, 7, 11, 25, limit}), limit


@pytest.mark.parametrize("rule", ["median", "trmean"])
def test_fused_equals_mixing_then_rule(bm, rule):
  counts, limit = _fused_counts(bm)
  for n in counts:
    for d in LENGTHS:
      host = [h.copy() for h in _rows(n, d)]
      host[1][d // 2] = np.nan                         # a NaN in a row most masks include
      if d > 8:
        host[0][5] = np.inf
      sq = nc.sqdist64(list(_rows(n, d)))
      for offset in OFFSETS:
        dev = _upload(host, offset)
        for f in nc.f_values(n):
          if rule == "trmean" and n < 2 * f + 1:
            continue
          words = nc.masks_reference(sq, n, f)
          masks = _masks(words)
          fused = bm.gars.colwise_mixed(rule, dev, masks, f)
          mixed = bm.gars.mix_rows(dev, masks, n)
          plain = getattr(bm.gars, rule)(mixed, f=f)
          assert nc.same_bits(fused.cpu().numpy(), plain.cpu().numpy()), (rule, n, d, offset, f)
          # the column that holds the NaN: the median is NaN as soon as one mixed value is; the trimmed mean follows
          # its nan_count > f rule
          col = d // 2
          nan_count = sum(1 for w in words if (w >> 1) & 1)
          expect_nan = nan_count > 0 if rule == "median" else nan_count > f
          assert bool(torch.isnan(fused[col])) == expect_nan, (rule, n, d, f, nan_count)


def test_beyond_the_row_limit_the_composition_runs(bm):
  lib = bm._lib.load()
  _, limit = _fused_counts(bm)
  n, f, d = limit + 1, 3, 1027
  if n > nc.MAX_ROWS:
    pytest.skip("the fused form covers every row count")
  host = list(_rows(n, d))
  dev = _upload(host, 0)
  masks = bm.gars.nnm_masks(bm.gars.pairwise_sqdist(dev), n, f)
  out = torch.empty(d, dtype=torch.float32, device=DEV)
  for op in (bm._lib.OP_MEDIAN, bm._lib.OP_TRMEAN):
    assert lib.bm_colwise_mixed(op, bm._lib.pointer_table(dev), n, ctypes.c_void_p(masks.data_ptr()), d, f,
                                ctypes.c_void_p(out.data_ptr()), None) == bm._lib.EINVAL
  mixed = bm.gars.mix_rows(dev, masks, n)
  assert torch.equal(bm.gars.nnm(dev, f, rule="median"), bm.gars.median(mixed))
  assert torch.equal(bm.gars.nnm(dev, f, rule="trmean"), bm.gars.trmean(mixed, f))


# ---------------------------------------------------------------------------- #
# 9. end to end, robust form: the masks rebuilt in numpy from the matrix the GPU computed

@pytest.mark.parametrize("n,f", [(11, 2), (25, 5), (51, 12)])
def test_nnm_equals_the_rule_on_numpy_mixed_rows(bm, n, f):
  d = 3074
  host = list(_rows(n, d))
  dev = _upload(host, 0)
  sq = bm.gars.pairwise_sqdist(dev).cpu().numpy()
  words = nc.masks_reference(sq, n, f)
  assert nc.from_int64(bm.gars.nnm_masks(bm.gars.pairwise_sqdist(dev), n, f).tolist())[:n] == words
  mixed = [torch.from_numpy(y).to(DEV) for y in nc.mix_reference(host, words)]
  for y, g in zip(mixed, bm.gars.nnm_rows(dev, f)):
    assert torch.equal(y, g)
  for rule in ("trmean", "median", "krum", "geomed", "average"):
    bm.gars.invalidate_rank_cache()
    got = bm.gars.nnm(dev, f, rule=rule)
    want = bm.gars._rule_on(rule, mixed, f, {})
    assert torch.equal(got, want), (rule, n, f)       # the same bits in, the same kernels: the same bits out
  assert bm.gars.krum_selection(bm.gars.nnm_rows(dev, f), f) == bm.gars.krum_selection(mixed, f)


# ---------------------------------------------------------------------------- #
# 10. end to end against float64 on the vectors

@pytest.mark.parametrize("n,f,ratio", [(7, 1, 1.3), (11, 2, 1.3), (25, 5, 1.15)])
@pytest.mark.parametrize("d", [1027, 3074])
def test_nnm_against_float64(bm, n, f, ratio, d):
  host, sq64, seed, gap = nc.separated_case(n, f, d, ratio)
  assert gap >= 1e-2                                   # a condition on the inputs, not a tolerance
  dev = _upload(host, 0)
  words = nc.masks_reference(sq64, n, f)
  got_words = nc.from_int64(bm.gars.nnm_masks(bm.gars.pairwise_sqdist(dev), n, f).tolist())[:n]
  assert got_words == words, (seed, gap)               # the float64 neighbour sets, exactly
  y64, bound = nc.mix_reference64(host, words)
  y64, bound = np.stack(y64), np.stack(bound)
  order = np.argsort(y64, axis=0, kind="stable")
  cols = np.arange(d)
  # median: the bound of the selected mixed value
  sel = order[(n - 1) // 2]
  med = bm.gars.nnm(dev, f, rule="median").cpu().numpy().astype(np.float64)
  excess = np.abs(med - y64[sel, cols]) - bound[sel, cols]
  print(f"n={n} f={f} d={d} seed={seed} gap={gap:.3g} median excess max {excess.max():.3g}")
  assert excess.max() <= 0
  # trimmed mean: the mean of the kept values' bounds plus (n - 2f + 1) 2^-24 mean|y|
  kept = order[f:n - f]
  want = np.take_along_axis(y64, kept, axis=0).mean(axis=0)
  bar = (np.take_along_axis(bound, kept, axis=0).mean(axis=0)
         + (n - 2 * f + 1) * nc.U * np.abs(np.take_along_axis(y64, kept, axis=0)).mean(axis=0))
  trm = bm.gars.nnm(dev, f, rule="trmean").cpu().numpy().astype(np.float64)
  excess = np.abs(trm - want) - bar
  print(f"n={n} f={f} d={d} trmean excess max {excess.max():.3g}")
  assert excess.max() <= 0


# ---------------------------------------------------------------------------- #
# 11. bucketing

@pytest.mark.parametrize("n", [11, 25])
def test_bucketing(bm, n):
  d = 1027
  host = list(_rows(n, d))
  dev = _upload(host, 0)
  perm = np.random.default_rng(n).permutation(n).tolist()
  words = bm.gars.bucket_masks(n, 2, perm)
  assert len(words) == (n + 1) // 2 and bin(words[-1]).count("1") == 1          # a ragged last bucket
  means = nc.mix_reference(host, words)
  got = bm.gars.mix_rows(dev, _masks(words), len(words))
  _assert_mixed(got, means, nc.mix_reference64(host, words), ("buckets", n))
  out = bm.gars.bucketing(dev, 2, "median", perm=perm)
  assert torch.equal(out, bm.gars.median([torch.from_numpy(m).to(DEV) for m in means]))
  # s = 1, identity: the rows themselves (x / 1 after 0 + x)
  same = bm.gars.mix_rows(dev, _masks(bm.gars.bucket_masks(n, 1, list(range(n)))), n)
  for g, h in zip(same, host):
    assert nc.same_bits(g.cpu().numpy(), h + np.float32(0))
  # a drawn permutation is reproducible from its seed, and the rule's f travels in rule_args
  a = bm.gars.bucketing(dev, 2, "trmean", seed=3, f=1)
  b = bm.gars.bucketing(dev, 2, "trmean", seed=3, f=1)
  assert torch.equal(a, b)
  with pytest.raises(ValueError):
    bm.gars.bucketing(dev, 2, "median", perm=[0] * n)


# ---------------------------------------------------------------------------- #
# 12. graph capture

def test_nnm_replays_in_a_graph(bm):
  n, f, d = 11, 2, 3074
  dev = _upload(nc.ladder_rows(n, d, 1.3, seed=1), 0)
  graphed = bm.graphs.GraphedCall(lambda: bm.gars.nnm(dev, f, rule="trmean"))
  for seed in (2, 3):
    fresh = nc.ladder_rows(n, d, 1.3, seed=seed)
    for t, h in zip(dev, fresh):
      t.copy_(torch.from_numpy(h))
    out = graphed().clone()
    assert torch.equal(out, bm.gars.nnm(dev, f, rule="trmean")), seed           # the replay followed the inputs
    words = nc.masks_reference(nc.sqdist64(fresh), n, f)
    mixed = np.stack(nc.mix_reference(fresh, words))
    assert nc.same_bits(out.cpu().numpy(), bm.gars.trmean([torch.from_numpy(y).to(DEV) for y in mixed], f).cpu().numpy())
