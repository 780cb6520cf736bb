"""bm_weighted_sum on the GPU against a float64 sum: every vector width (row alignments of 4, 8 and 16 bytes), lengths
that are no multiple of the width or of the block, more than one workgroup, 1 to 64 rows, aliased rows, weights that
are exactly zero on NaN rows, negative weights, a NaN weight, and several launch pieces; and bit for bit against the
kernel's definition evaluated on the CPU (the same fused steps in the same order) on inputs where that evaluation is exact.
Needs an MI355X: `pytest -m gpu`."""

import math

import numpy as np
import pytest
import torch

from tests import center_cases as cc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LENGTHS = (1, 3, 4, 63, 1027, 4099, 2 ** 20 + 3)
ROW_COUNTS = (1, 2, 11, 25, 64)


@pytest.fixture(scope="module")
def bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


def _rows(n, d, offset, seed):
  """n float32 rows of d values on the device, every one starting `offset` floats behind a 256-byte boundary (offset
  0: 16-byte aligned rows, 2: 8-byte, 1: 4-byte), and their host copies."""
  rng = np.random.default_rng(seed)
  host = [rng.normal(size=d).astype(np.float32) for _ in range(n)]
  return _upload(host, offset), host


def _upload(host, offset):
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


def _check(bm, dev, host, weights, tag):
  """The bar of the kernel's definition, per coordinate: |out_j - sum_i w_i x_ij| <= (N + 1) 2^-24 sum_i |w_i x_ij| with
  w_i = float32(c_i), aliased groups merged, the reference sum in float64 — N fused steps plus one rounding of each
  weight; nothing in it is measured."""
  out = bm.gars.weighted_sum(dev, torch.tensor(weights, dtype=torch.float64, device=DEV))
  want, bound = cc.weighted_sum_reference(host, weights)
  got = out.cpu().double().numpy()
  assert out.dtype == torch.float32 and got.shape == want.shape, tag
  excess = np.abs(got - want) - bound
  assert np.isfinite(got).all() and excess.max() <= 0, (tag, float(excess.max()), int(excess.argmax()))
  return out


@pytest.mark.parametrize("offset", [0, 2, 1], ids=["align16", "align8", "align4"])
@pytest.mark.parametrize("d", LENGTHS)
def test_lengths_and_alignments(bm, d, offset):
  dev, host = _rows(11, d, offset, seed=d + offset)
  rng = np.random.default_rng(7 * d + offset)
  weights = list(rng.uniform(0.0, 1.0, size=11) / 5.5)
  _check(bm, dev, host, weights, (d, offset))


@pytest.mark.parametrize("case", cc.WSUM_EXACT_CASES, ids=lambda c: c.name)
def test_bit_for_bit(bm, case):
  """Every coordinate against the kernel's definition evaluated on the CPU (cc.weighted_sum_exact): the same operations
  in the same order, not only a sum inside a rounding bound.  tests/test_weighted_sum_cases_cpu.py proves that the
  emulated fma meets no midpoint on these inputs, so no coordinate is left out."""
  rows, stack, weights = cc.wsum_exact_inputs(case)
  want, midpoints = cc.weighted_sum_exact([rows[i] for i in stack], weights)
  assert midpoints == 0
  dev = _upload(rows, case.offset)
  out = bm.gars.weighted_sum([dev[i] for i in stack], torch.tensor(weights, dtype=torch.float64, device=DEV))
  got = out.cpu().numpy()
  assert got.dtype == np.float32 and got.shape == want.shape
  differ = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
  assert differ.size == 0, (case.name, int(differ.size), int(differ[0]), float(got[differ[0]]), float(want[differ[0]]))


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts_signs_and_zero_weights(bm, n):
  d = 4099
  dev, host = _rows(n, d, 0, seed=n)
  rng = np.random.default_rng(n)
  weights = list(rng.normal(size=n))              # negative weights among them
  _check(bm, dev, host, weights, (n, "signed"))
  if n >= 2:
    # rows of weight exactly 0 hold NaN: they are not read, the sum stays finite
    zeroed = list(weights)
    for i in range(0, n, 3):
      zeroed[i] = 0.0 if i % 2 else -0.0
      dev[i].fill_(math.nan)
      host[i] = np.full(d, np.nan, dtype=np.float32)
    if all(w == 0 for w in zeroed):
      zeroed[-1] = 0.25
      dev[-1].normal_()
      host[-1] = dev[-1].cpu().numpy()
    clean = [np.zeros(d, dtype=np.float32) if w == 0 else h for h, w in zip(host, zeroed)]
    out = bm.gars.weighted_sum(dev, torch.tensor(zeroed, dtype=torch.float64, device=DEV))
    want, bound = cc.weighted_sum_reference(clean, zeroed)
    got = out.cpu().double().numpy()
    assert np.isfinite(got).all() and (np.abs(got - want) - bound).max() <= 0
  # every weight zero: the zero vector
  out = bm.gars.weighted_sum(dev, torch.zeros(n, dtype=torch.float64, device=DEV))
  assert not out.any()


def test_a_weight_too_small_for_float32_counts_as_zero(bm):
  dev, host = _rows(3, 1027, 0, seed=3)
  dev[1].fill_(math.nan)
  out = bm.gars.weighted_sum(dev, torch.tensor([0.5, 1e-60, 0.5], dtype=torch.float64, device=DEV))
  want, bound = cc.weighted_sum_reference([host[0], np.zeros(1027, dtype=np.float32), host[2]], [0.5, 0.0, 0.5])
  assert (np.abs(out.cpu().double().numpy() - want) - bound).max() <= 0


@pytest.mark.parametrize("d", [3, 4099])
def test_aliased_rows_are_one_group(bm, d):
  """Five references to one tensor (the copies of a Byzantine vector): their fp64 weights are added in index order and
  rounded once, the row is read once — also when the weights of the group cancel exactly (the row may then be NaN)."""
  dev, host = _rows(7, d, 0, seed=d)
  stack = dev[:6] + [dev[6]] * 5
  hstack = host[:6] + [host[6]] * 5
  rng = np.random.default_rng(d)
  weights = list(rng.uniform(0.01, 0.2, size=11))
  _check(bm, stack, hstack, weights, "aliased")
  # aliased rows in the middle of the stack, at non-adjacent indices
  mixed = [dev[0], dev[6], dev[1], dev[6], dev[2], dev[3], dev[6]]
  hmixed = [host[0], host[6], host[1], host[6], host[2], host[3], host[6]]
  _check(bm, mixed, hmixed, list(rng.normal(size=7)), "aliased-mixed")
  # a group whose weights cancel: dropped, not read
  dev[6].fill_(math.nan)
  cancel = weights[:6] + [0.125, -0.25, 0.0, 0.125, 0.0]
  out = bm.gars.weighted_sum(stack, torch.tensor(cancel, dtype=torch.float64, device=DEV))
  want, bound = cc.weighted_sum_reference(host[:6], cancel[:6])
  got = out.cpu().double().numpy()
  assert np.isfinite(got).all() and (np.abs(got - want) - (11 + 1) / 7 * bound).max() <= 0


@pytest.mark.parametrize("where", [0, 5, 10])
def test_a_nan_weight_gives_nan_everywhere(bm, where):
  for d in (3, 4099):
    dev, _ = _rows(11, d, 0, seed=where)
    weights = [1.0 / 11] * 11
    weights[where] = math.nan
    out = bm.gars.weighted_sum(dev, torch.tensor(weights, dtype=torch.float64, device=DEV))
    assert torch.isnan(out).all()
  # ... also inside an aliased group, and next to zero weights
  stack = dev[:9] + [dev[9]] * 2
  out = bm.gars.weighted_sum(stack, torch.tensor([0.0] * 9 + [0.5, math.nan], dtype=torch.float64, device=DEV))
  assert torch.isnan(out).all()


@pytest.mark.parametrize("piece", [1024, 1000, 7])
def test_several_launch_pieces(bm, piece):
  """The pass is cut into pieces of 2^29 columns; BM_WSUM_PIECE lowers the piece so that a short vector walks several
  (a piece that is no multiple of 4 also moves the following pieces to the narrower widths).  Same bits as one piece:
  the arithmetic per coordinate does not depend on the cut."""
  lib = bm._lib.load()
  d = 4099 if piece > 7 else 63
  dev, host = _rows(11, d, 0, seed=piece)
  rng = np.random.default_rng(piece)
  weights = list(rng.normal(size=11))
  whole = _check(bm, dev, host, weights, "one piece")
  assert lib.bm_tuning_set(b"BM_WSUM_PIECE", piece) == 0
  try:
    cut = _check(bm, dev, host, weights, ("pieces of", piece))
  finally:
    assert lib.bm_tuning_set(b"BM_WSUM_PIECE", 0) == 0
  assert torch.equal(whole, cut)


def test_empty_vectors_and_bad_arguments(bm):
  empty = [torch.empty(0, dtype=torch.float32, device=DEV) for _ in range(3)]
  out = bm.gars.weighted_sum(empty, torch.ones(3, dtype=torch.float64, device=DEV))
  assert out.shape == (0,)
  dev, _ = _rows(3, 8, 0, seed=1)
  with pytest.raises(bm.gars.GarInputError):
    bm.gars.weighted_sum(dev, torch.ones(2, dtype=torch.float64, device=DEV))       # fewer weights than rows
  with pytest.raises(bm.gars.GarInputError):
    bm.gars.weighted_sum(dev, torch.ones(3, dtype=torch.float32, device=DEV))       # float32 weights
  with pytest.raises(bm.gars.GarInputError):
    bm.gars.weighted_sum(dev, torch.ones(3, dtype=torch.float64))                   # weights on the host
