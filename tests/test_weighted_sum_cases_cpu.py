"""What tests/test_gpu_weighted_sum.py::test_bit_for_bit claims about its inputs (no GPU needed): the fma emulation
behind its expected values is exact on every one of them, and the cases are the ones it says."""

import numpy as np
import pytest

from tests import center_cases as cc


def test_the_case_list():
  shapes = {(c.n, c.d, c.offset) for c in cc.WSUM_EXACT_CASES if c.name != "aliased"}
  assert shapes == {(11, 4099, 0), (11, 4099, 2), (11, 4099, 1), (64, 1027, 0), (11, 3, 0)}
  aliased = [c for c in cc.WSUM_EXACT_CASES if c.name == "aliased"]
  assert len(aliased) == 1 and aliased[0].d == 4099
  assert cc.wsum_exact_inputs(aliased[0])[1] == [0, 1, 2, 3, 4, 5, 6, 6, 6, 6, 6]


@pytest.mark.parametrize("case", cc.WSUM_EXACT_CASES, ids=lambda c: c.name)
def test_the_emulation_meets_no_midpoint(case):
  """fma_emulated rounds twice (to float64, then to fp32); the two roundings are the one rounding of an fma unless the
  float64 sum lies exactly halfway between two fp32 numbers.  No step of any coordinate of a case does, so the GPU test
  may compare every coordinate.  The result is also inside the rounding bound of the float64 reference."""
  rows, stack, weights = cc.wsum_exact_inputs(case)
  points = [rows[i] for i in stack]
  want, midpoints = cc.weighted_sum_exact(points, weights)
  assert midpoints == 0
  assert want.dtype == np.float32 and want.shape == (case.d,) and np.isfinite(want).all()
  ref, bound = cc.weighted_sum_reference(points, weights)
  assert (np.abs(want.astype(np.float64) - ref) - bound).max() <= 0
