"""Bucket masks from a counter without a GPU: the host form bm_bucket_masks against the same definition in Python
integers (gars.bucket_permutation), the anchors the contract pins, the partition property, how evenly the definition
draws, the refusals, header and library."""

import collections
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("bm_bucket_masks", "bm_bucket_masks_device", "bm_colwise_bucketed", "bm_colwise_bucketed_supported")
MAX_ROWS = 64
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


def host_words(bm, n, s, seed, counter):
  got = bm.gars.bucket_masks_host(n, s, seed, counter)
  assert got.dtype == torch.int64 and got.shape == (MAX_ROWS,) and not got.is_cuda
  return [w & U64 for w in got.tolist()]


def perm_of(words, n, s):
  """The permutation back from the masks — up to the order inside a bucket, which the masks do not keep: the buckets
  as sorted index lists."""
  return [[j for j in range(n) if (w >> j) & 1] for w in words[:-(-n // s)]]


# ---------------------------------------------------------------------------- #
# 1. The anchors of the contract (include/bm_gar.h)

def test_anchor_permutations_in_python(bm):
  P = bm.gars.bucket_permutation
  assert P(11, 0, 0) == [6, 5, 0, 3, 4, 10, 2, 1, 8, 9, 7]
  assert P(11, 0, 1) == [10, 4, 7, 5, 3, 6, 8, 0, 9, 2, 1]
  assert P(64, 2 ** 63 + 5, 2 ** 40)[:8] == [16, 57, 58, 23, 62, 13, 33, 17]
  assert bm.gars.bucket_masks(11, 2, P(11, 0, 0)) == [0x60, 0x9, 0x410, 0x6, 0x300, 0x80]


def test_anchor_masks_from_the_library(bm):
  assert host_words(bm, 11, 2, 0, 0) == [0x60, 0x9, 0x410, 0x6, 0x300, 0x80] + [0] * (MAX_ROWS - 6)
  # s = 1: word b is the single bit perm[b] — the permutation itself, in order
  ones = lambda words, n: [w.bit_length() - 1 for w in words[:n]]  # noqa: E731
  assert ones(host_words(bm, 11, 1, 0, 0), 11) == [6, 5, 0, 3, 4, 10, 2, 1, 8, 9, 7]
  assert ones(host_words(bm, 11, 1, 0, 1), 11) == [10, 4, 7, 5, 3, 6, 8, 0, 9, 2, 1]
  assert ones(host_words(bm, 64, 1, 2 ** 63 + 5, 2 ** 40), 8) == [16, 57, 58, 23, 62, 13, 33, 17]


# ---------------------------------------------------------------------------- #
# 2. Host C against Python, and the partition property

@pytest.mark.parametrize("n", [1, 2, 5, 11, 25, 63, 64])
def test_host_form_equals_python_and_partitions(bm, n):
  for s in sorted({1, 2, 3, n} & set(range(1, n + 1))):
    for seed in (0, 1, U64):
      for counter in (0, 1, 2 ** 32, U64):
        perm = bm.gars.bucket_permutation(n, seed, counter)
        assert sorted(perm) == list(range(n))
        want = bm.gars.bucket_masks(n, s, perm)
        words = host_words(bm, n, s, seed, counter)
        n_out = -(-n // s)
        assert words[:n_out] == want and words[n_out:] == [0] * (MAX_ROWS - n_out), (n, s, seed, counter)
        # a partition of 0 .. n-1, bucket sizes s, s, ..., n mod s
        union = 0
        for w in words[:n_out]:
          assert union & w == 0
          union |= w
        assert union == (1 << n) - 1
        sizes = [bin(w).count("1") for w in words[:n_out]]
        assert sizes == [s] * (n // s) + ([n % s] if n % s else []), (n, s, sizes)


def test_consecutive_counters_and_seeds_differ(bm):
  seen = {tuple(bm.gars.bucket_permutation(25, seed, c)) for seed in (0, 1) for c in range(50)}
  assert len(seen) == 100


# ---------------------------------------------------------------------------- #
# 3. How evenly the definition draws: n = 5, all 120 permutations, 12 000 counters per seed.  A uniform draw gives 100
#    each with a standard deviation of 10; the definition itself gives 76 .. 129 over these three seeds.

@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_every_permutation_of_five_occurs_about_evenly(bm, seed):
  counts = collections.Counter(tuple(bm.gars.bucket_permutation(5, seed, c)) for c in range(12000))
  assert len(counts) == 120
  assert 70 <= min(counts.values()) and max(counts.values()) <= 130, (min(counts.values()), max(counts.values()))


# ---------------------------------------------------------------------------- #
# 4. Refusals

def test_refusals(bm):
  lib, EINVAL = bm._lib.load(), bm._lib.EINVAL
  out = torch.zeros(MAX_ROWS, dtype=torch.int64)
  ptr = out.data_ptr()
  for n, s in ((0, 1), (65, 1), (-1, 1), (11, 0), (11, 12), (11, -2)):
    assert lib.bm_bucket_masks(n, s, 0, 0, ptr) == EINVAL, (n, s)
  assert lib.bm_bucket_masks(11, 2, 0, 0, None) == EINVAL
  # the device form refuses the same before any HIP call (no GPU is touched here)
  for n, s in ((0, 1), (65, 1), (11, 0), (11, 12)):
    assert lib.bm_bucket_masks_device(n, s, 0, ptr, ptr, None) == EINVAL, (n, s)
  assert lib.bm_bucket_masks_device(11, 2, 0, None, ptr, None) == EINVAL
  assert lib.bm_bucket_masks_device(11, 2, 0, ptr, None, None) == EINVAL
  assert out.eq(0).all()
  for bad in ((0, 1), (65, 2), (5, 0), (5, 6)):
    with pytest.raises(ValueError):
      bm.gars.bucket_masks_host(*bad, 0, 0)
  with pytest.raises(ValueError):
    bm.gars.bucket_permutation(0, 0, 0)
  with pytest.raises(ValueError):
    bm.gars.bucket_permutation(65, 0, 0)


def test_fused_rule_refusals_before_any_launch(bm):
  """bm_colwise_bucketed returns BM_EINVAL for every bad argument before it touches the device."""
  lib, EINVAL = bm._lib.load(), bm._lib.EINVAL
  rows = [torch.zeros(8) for _ in range(5)]
  table = bm._lib.pointer_table(rows)
  masks, out = torch.zeros(MAX_ROWS, dtype=torch.int64), torch.zeros(8)
  M, T = bm._lib.OP_MEDIAN, bm._lib.OP_TRMEAN
  call = lambda op, tab, n, m, n_out, d, f, o: lib.bm_colwise_bucketed(op, tab, n, m, n_out, d, f, o, None)  # noqa: E731
  assert call(M, None, 5, masks.data_ptr(), 3, 8, 0, out.data_ptr()) == EINVAL
  assert call(M, table, 5, None, 3, 8, 0, out.data_ptr()) == EINVAL
  assert call(M, table, 5, masks.data_ptr(), 3, 8, 0, None) == EINVAL
  assert call(M, table, 5, masks.data_ptr(), 0, 8, 0, out.data_ptr()) == EINVAL
  assert call(M, table, 5, masks.data_ptr(), 6, 8, 0, out.data_ptr()) == EINVAL
  assert call(M, table, 5, masks.data_ptr(), 3, -1, 0, out.data_ptr()) == EINVAL
  assert call(T, table, 5, masks.data_ptr(), 3, 8, 2, out.data_ptr()) == EINVAL   # n_out < 2 f + 1
  assert call(T, table, 5, masks.data_ptr(), 3, 8, -1, out.data_ptr()) == EINVAL
  assert call(bm._lib.OP_PHOCAS, table, 5, masks.data_ptr(), 3, 8, 1, out.data_ptr()) == EINVAL
  assert call(M, table, 5, masks.data_ptr(), 4, 8, 0, out.data_ptr()) == EINVAL   # no instance for (5, 4)
  assert call(M, table, 5, masks.data_ptr(), 3, 0, 0, None) == 0                  # d == 0 launches nothing


# ---------------------------------------------------------------------------- #
# 5. Header and library

def test_header_declares_and_library_exports_the_four(bm):
  text = open(os.path.join(ROOT, "include", "bm_gar.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  declared = set(re.findall(r"\b(bm_[a-z0-9_]+)\s*\(", text))
  lib = bm._lib.load()
  for name in NEW_NAMES:
    assert name in declared and name in bm._lib.SIGNATURES and hasattr(lib, name), name
  assert bm._lib.ABI_VERSION == 23 and lib.bm_abi_version() == 23
  from byzantinemomentum_amd.sharded import HipBackend
  assert {"colwise_bucketed", "bucket_masks"} <= HipBackend.capabilities
