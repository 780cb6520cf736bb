"""bm_center_weights (csrc/center.cpp over csrc/center_core.h): the geometric median and centered clipping iterated on
the WEIGHTS of an affine combination of the rows, from their squared distances alone — against the same iteration run
on the vectors in float64 numpy (tests/center_cases.py), and on crafted matrices.  Host code only: no GPU."""

import ctypes
import math

import numpy as np
import pytest

from tests import center_cases as cc

# |v - v_ref| / |v_ref| between the combination of the rows under the library's weights (float64 distances computed
# from the rows) and the vector iteration.  A numpy prototype of the iteration on weights gives 1.5e-13 at worst on
# these cases: the bar leaves about three orders of margin for other seeds.
BAR = 1e-10


@pytest.fixture(scope="module")
def lib():
  from byzantinemomentum_amd import build, _lib
  build.build()
  return _lib.load()


@pytest.mark.parametrize("mode", ["geomed", "cclip"])
@pytest.mark.parametrize("case", cc.cases(), ids=cc.case_id)
def test_weights_reproduce_the_vector_iteration(lib, case, mode):
  rows, start = cc.make_rows(case)
  param, iters = cc.params(case, mode)
  points = rows if mode == "geomed" else np.concatenate([rows, start[None, :]])
  code, weights, info = cc.host_weights(lib, cc.exact_sqdist(points), case.n, mode, param, iters,
                                        has_start=mode == "cclip")
  assert code == 0
  ref, done = cc.vector_iteration(rows, mode, param, iters, start=start if mode == "cclip" else None)
  err = cc.relative_error(cc.combine(weights, points), ref)
  print(f"{cc.case_id(case)} {mode}: relative error {err:.3e}")
  assert err <= BAR
  assert info[0] == done == iters and info[2] == case.n
  assert abs(weights[:len(points)].sum() - 1.0) <= 1e-12 and not weights[len(points):].any()
  if mode == "geomed":
    assert (weights[:case.n] > 0).all()


@pytest.mark.parametrize("mode", ["geomed", "cclip"])
def test_uniform_start_without_a_start_vector(lib, mode):
  case = cc.cases()[1]
  rows, _ = cc.make_rows(case)
  param, iters = cc.params(case, mode)
  code, weights, info = cc.host_weights(lib, cc.exact_sqdist(rows), case.n, mode, param, iters)
  assert code == 0
  ref, _ = cc.vector_iteration(rows, mode, param, iters)
  assert cc.relative_error(cc.combine(weights, rows), ref) <= BAR


def test_one_row():
  from byzantinemomentum_amd import _lib
  lib = _lib.load()
  for mode, param in (("geomed", 1e-6), ("cclip", 1.0)):
    code, weights, info = cc.host_weights(lib, np.zeros((1, 1)), 1, mode, param, 5)
    assert code == 0 and weights[0] == 1.0 and not weights[1:].any()
    assert list(info) == [5.0, 0.0, 1.0]
  # one row and a start at distance 2, tau = 1: v = start + (x - start) / 2
  code, weights, info = cc.host_weights(lib, np.array([[0.0, 4.0], [4.0, 0.0]]), 1, "cclip", 1.0, 1, has_start=True)
  assert code == 0 and list(weights[:3]) == [0.5, 0.5, 0.0]
  assert info[0] == 1 and info[1] == 1.0 and info[2] == 1  # the step has length 1: move^2 = 1


def test_two_rows_stay_at_their_middle(lib):
  sq = np.array([[0.0, 9.0], [9.0, 0.0]])
  for mode, param in (("geomed", 1e-6), ("cclip", 0.5)):
    code, weights, info = cc.host_weights(lib, sq, 2, mode, param, 7)
    assert code == 0 and np.allclose(weights[:2], 0.5, rtol=1e-15, atol=0) and weights[2] == 0.0
    assert info[1] <= 1e-30 and info[2] == 2


@pytest.mark.parametrize("mode", ["geomed", "cclip"])
def test_sixty_four_points(lib, mode):
  rng = np.random.default_rng(64)
  has_start = mode == "cclip"
  n = 63 if has_start else 64
  rows = rng.normal(size=(n, 37)).astype(np.float32)
  rows[-5:] = rows[-1] + 20.0
  start = rng.normal(size=37).astype(np.float32) * 0.1
  points = np.concatenate([rows, start[None, :]]) if has_start else rows
  param = 1e-6 if mode == "geomed" else 4.0
  code, weights, info = cc.host_weights(lib, cc.exact_sqdist(points), n, mode, param, 16, has_start=has_start)
  assert code == 0 and info[2] == n
  ref, _ = cc.vector_iteration(rows, mode, param, 16, start=start if has_start else None)
  assert cc.relative_error(cc.combine(weights, points), ref) <= BAR


def _with_nan_rows(sq, which):
  sq = sq.copy()
  sq[which, :] = math.nan
  sq[:, which] = math.nan
  return sq


@pytest.mark.parametrize("mode", ["geomed", "cclip"])
def test_a_minority_of_nan_rows_is_excluded_and_the_rest_unchanged(lib, mode):
  case = cc.cases()[0]  # n = 11
  rows, start = cc.make_rows(case)
  param, iters = cc.params(case, mode)
  h = 8  # 3 NaN rows: each usable row misses 3 of its 10 distances
  clean = cc.exact_sqdist(rows[:h])
  # NaN rows last (where the `nan` attack puts them): the usable rows keep their indices, the same bits come out
  sq = _with_nan_rows(cc.exact_sqdist(rows), list(range(h, 11)))
  code, weights, info = cc.host_weights(lib, sq, 11, mode, param, iters)
  code2, expect, info2 = cc.host_weights(lib, clean, h, mode, param, iters)
  assert code == 0 and code2 == 0 and info[2] == h == info2[2]
  assert np.array_equal(weights[:h], expect[:h]) and not weights[h:].any()
  assert np.array_equal(info, info2)
  # NaN rows in the middle: the same weights up to the order of the sums
  which = [2, 5, 6]
  keep = [i for i in range(11) if i not in which]
  code, weights, info = cc.host_weights(lib, _with_nan_rows(cc.exact_sqdist(rows), which), 11, mode, param, iters)
  code2, expect, _ = cc.host_weights(lib, cc.exact_sqdist(rows[keep]), len(keep), mode, param, iters)
  assert code == 0 and code2 == 0 and info[2] == len(keep)
  assert not weights[which].any()
  np.testing.assert_allclose(weights[keep], expect[:len(keep)], rtol=1e-12, atol=0)


@pytest.mark.parametrize("mode", ["geomed", "cclip"])
@pytest.mark.parametrize("finite_among_themselves", [False, True])
def test_a_majority_of_nan_rows_gives_nan_weights(lib, mode, finite_among_themselves):
  case = cc.cases()[0]
  rows, _ = cc.make_rows(case)
  param, iters = cc.params(case, mode)
  which = list(range(5, 11))  # 6 of 11
  sq = _with_nan_rows(cc.exact_sqdist(rows), which)
  if finite_among_themselves:  # aliased NaN rows to which the distance pass gave a mutual distance of 0
    for i in which:
      for j in which:
        sq[i, j] = 0.0
  code, weights, info = cc.host_weights(lib, sq, 11, mode, param, iters)
  assert code == 0
  # six of eleven: every row, honest or not, misses at least half of its ten distances
  assert np.isnan(weights[:11]).all() and not weights[11:].any()
  assert info[0] == 0 and info[2] == 0
  if finite_among_themselves:
    # eight of eleven copies that see each other are the usable ones (each misses 3 of 10), the three honest rows are
    # not: all the weight sits on NaN rows, so the weighted sum of the rows is NaN everywhere just the same
    which = list(range(3, 11))
    sq = _with_nan_rows(cc.exact_sqdist(rows), which)
    for i in which:
      for j in which:
        sq[i, j] = 0.0
    code, weights, info = cc.host_weights(lib, sq, 11, mode, param, iters)
    assert code == 0 and info[2] == 8 and not weights[:3].any() and abs(weights[3:11].sum() - 1.0) <= 1e-12


def test_a_nan_start_falls_back_to_the_uniform_start(lib):
  case = cc.cases()[0]
  rows, start = cc.make_rows(case)
  param, iters = cc.params(case, "cclip")
  points = np.concatenate([rows, start[None, :]])
  sq = _with_nan_rows(cc.exact_sqdist(points), [11])
  code, weights, info = cc.host_weights(lib, sq, 11, "cclip", param, iters, has_start=True)
  code2, expect, info2 = cc.host_weights(lib, cc.exact_sqdist(rows), 11, "cclip", param, iters)
  assert code == 0 and code2 == 0
  assert np.array_equal(weights, expect) and weights[11] == 0.0
  assert np.array_equal(info, info2)


def test_a_point_at_distance_zero_from_the_iterate(lib):
  # geomed: three copies of one point — every distance is 0, the weights are 1 / nu each, the iterate stays
  code, weights, info = cc.host_weights(lib, np.zeros((3, 3)), 3, "geomed", 1e-9, 4)
  assert code == 0 and np.allclose(weights[:3], 1 / 3, rtol=1e-15) and info[1] == 0.0
  # cclip from a start that IS row 0: r_0 = 0 counts as inside the ball (s_0 = 1), nothing divides by it
  rows = np.array([[0.0, 0.0], [3.0, 4.0]], dtype=np.float32)
  points = np.concatenate([rows, rows[:1]])
  code, weights, info = cc.host_weights(lib, cc.exact_sqdist(points), 2, "cclip", 1.0, 1, has_start=True)
  assert code == 0 and np.isfinite(weights).all()
  ref, _ = cc.vector_iteration(rows, "cclip", 1.0, 1, start=rows[0])
  np.testing.assert_allclose(cc.combine(weights, points), ref, rtol=1e-15, atol=1e-15)


def test_tol_stops_early_and_says_when(lib):
  case = cc.cases()[4]  # n = 25, k = 5, empire
  rows, _ = cc.make_rows(case)
  nu = 1e-6 * math.sqrt(case.d)
  sq = cc.exact_sqdist(rows)
  _, _, full = cc.host_weights(lib, sq, case.n, "geomed", nu, 32)
  assert full[0] == 32  # tol = 0: never early
  tol = 1e-3
  ref, done = cc.vector_iteration(rows, "geomed", nu, 32, tol=tol)
  assert 1 < done < 32
  code, weights, info = cc.host_weights(lib, sq, case.n, "geomed", nu, 32, tol=tol)
  assert code == 0 and info[0] == done and math.sqrt(info[1]) <= tol
  assert cc.relative_error(cc.combine(weights, rows), ref) <= BAR


def test_bad_arguments_are_refused(lib):
  from byzantinemomentum_amd import _lib
  sq = np.zeros((65, 65))
  ok = dict(n=11, mode="geomed", param=1e-6, iters=8, tol=0.0, has_start=False)

  def code(**change):
    a = dict(ok, **change)
    return cc.host_weights(lib, sq, a["n"], a["mode"], a["param"], a["iters"], a["tol"], a["has_start"])[0]

  assert code() == 0
  assert code(iters=0) == _lib.EINVAL and code(iters=65) == _lib.EINVAL and code(iters=64) == 0
  assert code(param=0.0) == _lib.EINVAL and code(param=-1.0) == _lib.EINVAL and code(param=math.nan) == _lib.EINVAL
  assert code(mode="cclip", param=0.0) == _lib.EINVAL and code(mode="cclip", param=-2.0) == _lib.EINVAL
  assert code(tol=-1e-9) == _lib.EINVAL and code(tol=math.nan) == _lib.EINVAL
  assert code(n=0) == _lib.EINVAL and code(n=65) == _lib.EINVAL and code(n=64) == 0
  assert code(n=64, has_start=True) == _lib.EINVAL and code(n=63, has_start=True) == 0  # N > 64
  buf = (ctypes.c_double * 64)()
  assert lib.bm_center_weights(buf, 11, 0, 2, 1.0, 8, 0.0, buf, buf) == _lib.EINVAL   # no such mode
  assert lib.bm_center_weights(buf, 11, 2, 0, 1.0, 8, 0.0, buf, buf) == _lib.EINVAL   # has_start is 0 or 1
  assert lib.bm_center_weights(None, 11, 0, 0, 1.0, 8, 0.0, buf, buf) == _lib.EINVAL
  # the device form and the weighted sum refuse before any HIP call (no GPU here)
  assert lib.bm_center_weights_device(buf, 11, 0, 0, 1.0, 0, 0.0, buf, buf, None) == _lib.EINVAL
  assert lib.bm_center_weights_device(buf, 64, 1, 1, 1.0, 3, 0.0, buf, buf, None) == _lib.EINVAL
  assert lib.bm_center_weights_device(buf, 11, 0, 0, -1.0, 3, 0.0, buf, buf, None) == _lib.EINVAL
  assert lib.bm_center_weights_device(buf, 11, 0, 0, 1.0, 3, -1.0, buf, buf, None) == _lib.EINVAL
  assert lib.bm_center_weights_device(None, 11, 0, 0, 1.0, 3, 0.0, buf, buf, None) == _lib.EINVAL
  rows = (ctypes.c_void_p * 64)()
  assert lib.bm_weighted_sum(rows, 0, buf, 10, buf, None) == _lib.EINVAL
  assert lib.bm_weighted_sum(rows, 65, buf, 10, buf, None) == _lib.EINVAL
  assert lib.bm_weighted_sum(rows, 3, None, 10, buf, None) == _lib.EINVAL
  assert lib.bm_weighted_sum(rows, 3, buf, -1, buf, None) == _lib.EINVAL
  assert lib.bm_weighted_sum(rows, 3, buf, 0, None, None) == 0   # empty vectors: nothing to do
