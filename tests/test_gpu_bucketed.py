"""bm_colwise_bucketed on the GPU, bit for bit against bm_mix_rows followed by bm_colwise: every bucket count class, the
three vector widths (rows at 16 / 8 / 4-byte offsets), tails, several workgroups, the counter-drawn partitions, an
overlapping and an empty mask, NaN and inf inside and outside a mask, aliased rows, and the fall-back of gars.bucketing
where no instance exists.  Needs an MI355X: `pytest -m gpu`."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BLOCK = 256                                   # kColBlock: a workgroup spans BLOCK * VEC columns
LENGTHS = (1, 3, 259, 2 * BLOCK * 4 + 3)      # one lane; a tail alone; body + tail; beyond one workgroup's span at every
                                              # width (4, 2, 1 columns per lane), with a ragged tail
OFFSETS = (0, 2, 1)                           # floats behind a 16-byte boundary: vector width 4 / 2 / 1
SHAPES = [(2, 1), (3, 2), (5, 2), (5, 3), (11, 6), (11, 4), (25, 13), (25, 9)]
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


@functools.lru_cache(maxsize=None)
def largest_n(s):
  """The largest row count with an instance for buckets of s (each bucket size has its own measured limit)."""
  from byzantinemomentum_amd import _lib
  lib = _lib.load()
  return max(n for n in range(2, 65) if lib.bm_colwise_bucketed_supported(0, n, -(-n // s)))


def all_shapes():
  return SHAPES + [(largest_n(s), -(-largest_n(s) // s)) for s in (2, 3)]


@functools.lru_cache(maxsize=None)
def host_rows(n, d):
  gen = torch.Generator().manual_seed(100 * n + d)
  # sums that round: values of mixed magnitude, so that the order of the float32 sum shows in the bits
  return tuple(torch.randn(d, generator=gen) * (10.0 ** torch.randint(-3, 4, (d,), generator=gen).float()) for _ in range(n))


def upload(host, offset):
  """The rows cut from ONE allocation, every one starting `offset` floats behind a 256-byte boundary."""
  n, d = len(host), host[0].shape[0]
  per = -(-(d + offset) // 64) * 64
  pool = torch.zeros(n * per, dtype=torch.float32, device=DEV)
  dev = []
  for i, h in enumerate(host):
    view = pool[i * per + offset:i * per + offset + d]
    view.copy_(h)
    dev.append(view)
  assert all(v.data_ptr() % 16 == 4 * offset for v in dev)
  return dev


def words(masks):
  return torch.tensor([w - (1 << 64) if w >= (1 << 63) else w for w in masks], dtype=torch.int64, device=DEV)


def same_bits(a, b):
  return torch.equal(a.view(torch.int32), b.view(torch.int32))


def composed(bm, rule, rows, masks, n_out, f):
  means = bm.gars.mix_rows(rows, masks, n_out)
  return bm.gars.median(means) if rule == "median" else bm.gars.trmean(means, f)


def check(bm, rows, masks, n_out, tag):
  for rule, fs in (("median", (0,)), ("trmean", sorted({0, (n_out - 1) // 2}))):
    for f in fs:
      got = bm.gars.colwise_bucketed(rule, rows, masks, n_out, f)
      want = composed(bm, rule, rows, masks, n_out, f)
      assert same_bits(got, want), (tag, rule, f, int((got.view(torch.int32) != want.view(torch.int32)).nonzero()[0]))


def partition(bm, n, n_out, counter):
  s = 2 if n_out == -(-n // 2) else 3
  assert -(-n // s) == n_out
  return bm.gars.bucket_masks_host(n, s, 7, counter).to(DEV)


@pytest.mark.parametrize("n,n_out", all_shapes(), ids=lambda v: str(v))
def test_partitions_at_every_width_and_length(bm, n, n_out):
  assert bm.gars.colwise_bucketed_supported("median", n, n_out) and bm.gars.colwise_bucketed_supported("trmean", n, n_out)
  for d in LENGTHS:
    for offset in OFFSETS:   # (offset 1: a row table 4 bytes off forces one column per lane)
      rows = upload(host_rows(n, d), offset)
      for counter in (0, 1):
        check(bm, rows, partition(bm, n, n_out, counter), n_out, (n, n_out, d, offset, counter))


@pytest.mark.parametrize("n,n_out", all_shapes(), ids=lambda v: str(v))
def test_general_masks_and_non_finite_values(bm, n, n_out):
  d = LENGTHS[-1]
  host = [r.clone() for r in host_rows(n, d)]
  gen = torch.Generator().manual_seed(n * 64 + n_out)
  # overlapping masks (bits beyond n are ignored), then the same set with one mask empty: a NaN row
  over = [int(torch.randint(1, 1 << min(n, 30), (1,), generator=gen)) | (1 << (r % n)) for r in range(n_out)]
  if n < 64:
    over[0] |= (1 << n) | (1 << 63)
  empty = list(over)
  empty[n_out // 2] = 0
  # NaN / inf in row 0 and in the last row, each at a few columns: the partition keeps them out of most means (outside
  # a mask they must not show), the overlapping set has them inside several
  for j, value in ((0, float("nan")), (0, float("inf")), (n - 1, float("-inf")), (n - 1, float("nan"))):
    at = torch.randint(0, d, (5,), generator=gen)
    host[j][at] = value
  host[0][d - 1] = float("inf")       # the ragged tail too
  for offset in OFFSETS:
    rows = upload(host, offset)
    check(bm, rows, partition(bm, n, n_out, 3), n_out, (n, n_out, offset, "partition + non-finite"))
    check(bm, rows, words(over), n_out, (n, n_out, offset, "overlapping"))
    check(bm, rows, words(empty), n_out, (n, n_out, offset, "empty"))
  # a row outside every mask does not show, whatever it holds
  rows = upload(host, 0)
  masks = partition(bm, n, n_out, 3)
  if n >= 3:
    first = int(masks[0].item()) & U64
    lone = first.bit_length() - 1                      # a row of bucket 0, taken out of it
    rest = first & ~(1 << lone)
    if rest:
      cut = masks.clone()
      cut[0] = rest - (1 << 64) if rest >= (1 << 63) else rest
      before = bm.gars.colwise_bucketed("median", rows, cut, n_out)
      rows[lone].fill_(float("nan"))
      after = bm.gars.colwise_bucketed("median", rows, cut, n_out)
      assert same_bits(before, after)


@pytest.mark.parametrize("n,n_out", [(5, 3), (11, 6), (25, 9)])
def test_a_stack_whose_last_rows_alias_one_tensor(bm, n, n_out):
  d = 259
  rows = upload(host_rows(n, d), 0)
  k = max(2, n // 5)
  rows = rows[:n - k] + [rows[n - k]] * k        # the step's stack: honests + [byz] * f_real
  for counter in (0, 5):
    check(bm, rows, partition(bm, n, n_out, counter), n_out, (n, n_out, "aliased", counter))


def test_unsupported_shapes_are_refused_and_bucketing_falls_back(bm):
  lib, EINVAL = bm._lib.load(), bm._lib.EINVAL
  n, d = 11, 259
  rows = upload(host_rows(n, d), 0)
  out = torch.full((d,), 7.0, device=DEV)
  for n_out in (1, 2, 3, 5, 7, 11):
    assert not bm.gars.colwise_bucketed_supported("median", n, n_out)
    masks = words([1 << r for r in range(n_out)])
    rc = lib.bm_colwise_bucketed(bm._lib.OP_MEDIAN, bm._lib.pointer_table(rows), n, masks.data_ptr(), n_out, d, 0,
                                 out.data_ptr(), None)
    assert rc == EINVAL
  for s in (2, 3):
    big = largest_n(s) + 1
    assert big <= 64 and not bm.gars.colwise_bucketed_supported("median", big, -(-big // s))
  torch.cuda.synchronize()
  assert bool((out == 7.0).all())              # nothing was launched
  with pytest.raises(RuntimeError):
    bm.gars.colwise_bucketed("median", rows, words([1, 2, 4, 8, 16]), 5)
  # gars.bucketing: s = 4 -> 3 means, no instance: mix_rows + the rule, the bits the fused form would have given;
  # s = 2 / 3 take the fused kernel — in both cases the composition's bits
  for s in (2, 3, 4):
    n_out = -(-n // s)
    for counter in (0, 1):
      perm = bm.gars.bucket_permutation(n, 5, counter)
      masks = words(bm.gars.bucket_masks(n, s, perm))
      got = bm.gars.bucketing(rows, s, "median", seed=5, counter=counter)
      assert same_bits(got, composed(bm, "median", rows, masks, n_out, 0)), (s, counter)
      assert same_bits(got, bm.gars.bucketing(rows, s, "median", perm=perm))
      if n_out >= 3:
        got = bm.gars.bucketing(rows, s, "trmean", seed=5, counter=counter, f=1)
        assert same_bits(got, composed(bm, "trmean", rows, masks, n_out, 1)), (s, counter)
  # without a counter the draw is torch.randperm's, as it was
  a = bm.gars.bucketing(rows, 2, "median", seed=3)
  perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).tolist()
  assert same_bits(a, bm.gars.bucketing(rows, 2, "median", perm=perm))
  with pytest.raises(ValueError):
    bm.gars.bucketing(rows, 2, "median", perm=perm, counter=0)


def test_zero_length_rows(bm):
  rows = [torch.empty(0, device=DEV) for _ in range(5)]
  out = bm.gars.colwise_bucketed("median", rows, words([3, 12, 16]), 3)
  assert out.shape == (0,)
  assert bm.gars.bucketing(rows, 2, "median", counter=0).shape == (0,)
