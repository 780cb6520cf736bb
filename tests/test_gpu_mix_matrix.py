"""Every compiled instance of the two mixing kernels (tests/mix_matrix.py): mix_rows_kernel<N, VEC> at N = 1..64 and
colwise_mixed_kernel<N, OP, VEC> at N = 1..36, at every vector width, with the tail group alone, behind one workgroup
and in a wave with body groups, with widths forced by the outputs, launch pieces that narrow, and one case per kernel
whose grid-stride loop takes a second trip.

Expected values are made of the inputs alone.  bm_mix_rows: every output row and column bit for bit against the
float32 loop of the contract (nnm_cases.mix_reference; a NaN matches any NaN).  The fused kernels: the numpy-mixed
rows, never rows bm_mix_rows wrote — the median bit for bit their lower median (no zero-sign exemption:
tests/test_mix_matrix_cpu.py proves no mixed value is -0), the trimmed mean within 1e-6 of scale of the oracle on them
(instance_matrix.check_colwise; NaN iff more than f mixed values are NaN), and both bit for bit the plain rule run on
the numpy-mixed rows uploaded to the device.  Special columns (NaN, infinities, zeros, cancelling rows, subnormal
quotients, overflowing sums) sit among ordinary ones, so one launch has waves on the rare paths next to waves on the
common one.  Needs an MI355X: `pytest -m gpu`."""

import functools

import numpy as np
import pytest
import torch

from tests import instance_matrix as M
from tests import mix_matrix as X
from tests import nnm_cases as nc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bm():
  return X._bm()


def _tag(case, **more):
  return dict(kernel=case.kernel, rule=case.rule, N=case.n, offset=case.offset, out_offset=case.out_offset, d=case.d,
              piece=case.piece, masks=case.masks, f=case.f, **more)


def _check_mix_rows(case, got):
  want = X.mixed_reference(case.kernel, case.n, case.d, case.masks)
  assert got.shape == want.shape and got.dtype == np.float32, _tag(case, shape=got.shape)
  if not nc.same_bits(got, want):
    for r in range(want.shape[0]):
      col = X.first_difference(got[r], want[r])
      assert col is None, _tag(case, row=r, column=col, got=got[r, col], want=want[r, col],
                               kind=X.KINDS[X.special_columns(case.n, case.d)[col]]
                               if col in X.special_columns(case.n, case.d) else "ordinary")
  if case.masks == "onehot":
    assert nc.same_bits(got, X.values(case.n, case.d) + np.float32(0)), _tag(case)       # y_r = x_r + 0


@functools.lru_cache(maxsize=32)
def _fused_reference(bm, rule, n, d, masks, f):
  """(the lower median of the numpy-mixed values or None, the plain rule's output on the numpy-mixed rows uploaded to
  the device) — the same for every offset of (n, d, masks, f)."""
  mixed = X.mixed_reference(X.FUSED, n, d, masks)
  dev = [torch.tensor(mixed[r], device=X.DEV) for r in range(n)]
  if rule == X.MEDIAN:
    return X.lower_median(mixed), bm.gars.median(dev).cpu().numpy()
  return None, bm.gars.trmean(dev, f).cpu().numpy()


def _check_fused(bm, case, got):
  n, d, f = case.n, case.d, case.f
  mixed = X.mixed_reference(X.FUSED, n, d, case.masks)
  want, plain = _fused_reference(bm, case.rule, n, d, case.masks, f)
  assert got.shape == (d,) and got.dtype == np.float32
  nan_count = np.isnan(mixed).sum(axis=0)
  if case.rule == X.MEDIAN:
    col = X.first_difference(got, want)
    assert col is None, _tag(case, column=col, got=got[col], want=want[col], against="lower median of the numpy-mixed values")
    assert np.array_equal(np.isnan(got), nan_count > 0), _tag(case)
  else:
    # the overflowing columns have a scale of their own (3e38): held to the bar apart from the others
    huge = np.zeros(d, dtype=bool)
    huge[X.columns_of_kind(n, d, "huge")] = True
    for part in (huge, ~huge):
      if part.any():
        bad = M.check_colwise(M.TRMEAN, f, torch.from_numpy(got[part]), torch.from_numpy(mixed[:, part]))
        assert int(bad.sum()) == 0, _tag(case, column=int(np.flatnonzero(part)[int(torch.nonzero(bad)[0])]),
                                         against="oracle trimmed mean of the numpy-mixed values")
    # NaN iff more than f mixed values are NaN (an infinity of each sign inside the kept window is the other way to one)
    plain_columns = ~np.isinf(mixed).any(axis=0)
    assert np.array_equal(np.isnan(got)[plain_columns], (nan_count > f)[plain_columns]), _tag(case)
  col = X.first_difference(got, plain)
  assert col is None, _tag(case, column=col, got=got[col], want=plain[col], against="the plain rule on the numpy-mixed rows")
  if case.masks == "random":
    assert (nan_count >= 1).all()                                  # the empty mask: one mixed value is NaN everywhere


def _run_and_check(bm, todo):
  """Runs the cases of `todo`, the input of an (n, d, offset) uploaded once."""
  rows, key = None, None
  for case in todo:
    if (case.n, case.d, case.offset) != key:
      key = (case.n, case.d, case.offset)
      rows = X.upload(*key)
    got = X.run(case, rows)
    if case.kernel == X.MIX_ROWS:
      _check_mix_rows(case, got)
    else:
      _check_fused(bm, case, got)
  return len(todo)


def _ordered(cases):
  """One upload per (n, d, offset); the references of an (n, d, mask set, f) are cached across the offsets."""
  return sorted(cases, key=lambda c: (c.n, c.d, c.offset, c.out_offset, c.masks, c.f))


# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", range(1, X.BM_MAX_ROWS + 1))
def test_mix_rows_every_row_count(bm, n):
  """mix_rows_kernel<n, 4 / 2 / 1> (2 / 1 beyond 28 rows) at d = 3 and 1027 with every mask set."""
  todo = [c for c in X.cases("every_n") if c.kernel == X.MIX_ROWS and c.n == n]
  assert {i for c in todo for i in X.instances(c)} == {i for i in X.universe() if i[0] == X.MIX_ROWS and i[1] == n}
  assert _run_and_check(bm, _ordered(todo)) >= 6 * 4


@pytest.mark.parametrize("rule", X.FUSED_RULES)
@pytest.mark.parametrize("n", range(1, X.K_MIXED_MAX_ROWS + 1))
def test_fused_every_row_count(bm, n, rule):
  """colwise_mixed_kernel<n, rule, 2 / 1> at d = 3 and 1027: one-hot masks, complements, neighbour masks of every f
  under rule f's that differ from it, random masks with an empty one."""
  todo = [c for c in X.cases("every_n") if c.kernel == X.FUSED and c.n == n and c.rule == rule]
  assert {i for c in todo for i in X.instances(c)} == {i for i in X.universe() if i[0] == X.FUSED and i[1:3] == (n, rule)}
  assert _run_and_check(bm, _ordered(todo)) >= 6 * 4


@pytest.mark.parametrize("n", X.FLAGSHIP)
def test_flagship_row_counts_at_more_lengths(bm, n):
  """d = 1 (one lane), 259 (the tail group a wave's first lane) and 3074 (several workgroups), both kernels."""
  todo = [c for c in X.cases("flagship") if c.n == n]
  assert {c.d for c in todo} == set(X.D_FLAGSHIP)
  _run_and_check(bm, _ordered(todo))


@pytest.mark.parametrize("kernel,n", X.FORCED)
def test_widths_forced_by_the_outputs(bm, kernel, n):
  """Inputs at 16 bytes, outputs 4 and 8 bytes off (through the C entry points): the width follows the outputs, the
  bits are those of the reference all the same."""
  todo = [c for c in X.cases("out_forced") if (c.kernel, c.n) == (kernel, n)]
  assert any(X.launches(c)[0].vec < X.input_width(c) for c in todo)
  _run_and_check(bm, _ordered(todo))


@pytest.mark.parametrize("piece,d", X.PIECES)
def test_pieces_that_narrow(bm, piece, d):
  """BM_WSUM_PIECE = 1002 at d = 3074 and 7 at d = 63 from 16-byte rows: later pieces start 8 and 4 bytes off and run
  the narrower instances; the bits of the uncut call, which has the bits of the reference."""
  todo = [c for c in X.cases("pieces") if (c.piece, c.d) == (piece, d)]
  rows = X.upload(11, d, 0)
  for case in _ordered(todo):
    assert len({l.vec for l in X.launches(case)}) >= 2 or (case.kernel == X.FUSED and piece == 1002)   # (all VEC 2)
    cut = X.run(case, rows)
    whole = X.run(case._replace(piece=0), rows)
    col = X.first_difference(cut.ravel(), whole.ravel())
    assert col is None, _tag(case, flat_index=col, against="the uncut call")
    if case.kernel == X.MIX_ROWS:
      _check_mix_rows(case, cut)
    else:
      _check_fused(bm, case, cut)


@pytest.mark.parametrize("kernel,rule", [(X.MIX_ROWS, None), (X.FUSED, X.MEDIAN), (X.FUSED, X.TRMEAN)])
def test_second_trip_of_the_grid_stride_loop(bm, kernel, rule):
  """N = 3 at 4-byte rows, d = 16384 * 256 + 259: the first 259 lanes of the capped grid take a second body trip.
  Every column is compared."""
  todo = [c for c in X.cases("long") if (c.kernel, c.rule) == (kernel, rule)]
  assert all(X.launches(c)[0].body_trips == 2 for c in todo)
  _run_and_check(bm, _ordered(todo))
