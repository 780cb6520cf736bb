"""bm_spectral_weights (csrc/spectral.cpp over csrc/spectral_core.h): CAF and DnC evaluated on the squared distances of
the rows alone — against the same rules run on the vectors in float64 numpy (tests/spectral_cases.py), and on crafted
matrices.  Host code only: no GPU."""

import ctypes
import math

import numpy as np
import pytest

from tests import spectral_cases as sc

# |w - w_ref| of every weight between the library on float64 distances and the definition on the vectors.  A numpy
# prototype of the evaluation on scalars gave 1.1e-15 at worst on these cases (the host form here: 1.1e-15 too): the bar
# leaves three orders of margin for other summation orders, as test_center_weights_cpu.py argues for its own.
BAR = 1e-12


@pytest.fixture(scope="module")
def lib():
  from byzantinemomentum_amd import build, _lib
  build.build()
  return _lib.load()


@pytest.mark.parametrize("T", sc.POWER_ITERS)
@pytest.mark.parametrize("mode", ["caf", "dnc"])
@pytest.mark.parametrize("case", sc.cases(), ids=sc.case_id)
def test_weights_reproduce_the_rule_on_the_vectors(lib, case, mode, T):
  rows, _ = sc.make_rows(case)
  count = sc.count_of(case, mode)
  code, weights, info = sc.host_weights(lib, sc.exact_sqdist(rows), case.n, mode, count, T)
  assert code == 0
  ref = sc.vector_spectral(rows, mode, count, T)
  err = float(np.abs(weights[:case.n] - ref.weights).max())
  print(f"{sc.case_id(case)} {mode} T={T}: weights differ by {err:.3e}; rounds {ref.rounds}, kept {ref.kept}")
  assert err <= BAR
  assert info[0] == ref.rounds and info[3] == ref.kept and info[2] == case.n == ref.usable
  assert abs(info[1] - ref.lam) <= 1e-10 * ref.lam
  assert abs(weights[:case.n].sum() - 1.0) <= 1e-12 and not weights[case.n:].any()
  assert (weights[:case.n] >= 0).all()


def _crafted(name):
  for item in sc.crafted():
    if item[0] == name:
      return item[1:]
  raise KeyError(name)


def _run(lib, name, T=16):
  sq, n, mode, count = _crafted(name)
  code, weights, info = sc.host_weights(lib, sq, n, mode, count, T)
  assert code == 0 and not weights[n:].any()
  return weights[:n], info


def test_one_two_and_three_rows(lib):
  for name in ("one-row", "one-row-dnc"):
    w, info = _run(lib, name)
    assert w[0] == 1.0 and list(info) == [0.0, math.inf, 1.0, -1.0]  # one row IS the weighted mean: degenerate
  w, info = _run(lib, "two-rows")                                    # f = 0: 2 > 2 - 0 is false, no round
  assert list(w) == [0.5, 0.5] and list(info) == [0.0, math.inf, 2.0, -1.0]
  w, info = _run(lib, "two-rows-dnc")   # both rows project 3 / 2 on the one direction: a tie, the higher index goes
  assert list(w) == [1.0, 0.0] and list(info) == [1.0, 2.25, 2.0, 0.0]
  w, info = _run(lib, "three-rows")
  assert abs(w.sum() - 1.0) <= 1e-12 and (w == 0).sum() == 1 and info[2] == 3
  w, info = _run(lib, "three-rows-dnc")
  assert sorted(w) == [0.0, 0.0, 1.0]


@pytest.mark.parametrize("name", ["sixty-four", "sixty-four-f31", "sixty-four-dnc"])
@pytest.mark.parametrize("T", sc.POWER_ITERS)
def test_sixty_four_rows(lib, name, T):
  sq, n, mode, count = _crafted(name)
  big = sc.sixty_four_rows()
  code, weights, info = sc.host_weights(lib, sq, n, mode, count, T)
  ref = sc.vector_spectral(big, mode, count, T)
  assert code == 0 and info[0] == ref.rounds and info[3] == ref.kept
  assert float(np.abs(weights - ref.weights).max()) <= BAR
  assert not weights[-9:].any()         # the nine far copies are gone
  if name == "sixty-four-f31":
    assert ref.rounds >= 8               # many rounds, each zeroing a row


def test_f_zero_and_k_zero_are_the_mean(lib):
  w, info = _run(lib, "f-zero")
  assert np.array_equal(w, np.full(11, 1.0 / 11)) and list(info) == [0.0, math.inf, 11.0, -1.0]
  w, info = _run(lib, "k-zero")         # DnC evaluates once and removes nothing
  assert np.array_equal(w, np.full(11, 1.0 / 11)) and info[0] == 1 and info[3] == 0 and info[1] > 0


def test_all_rows_equal_is_degenerate(lib):
  w, info = _run(lib, "all-equal")
  assert np.array_equal(w, np.full(7, 1.0 / 7)) and list(info) == [0.0, math.inf, 7.0, -1.0]
  w, info = _run(lib, "all-equal-dnc")  # every tau is 0: the k rows of highest index go
  assert np.array_equal(w, np.array([0.2] * 5 + [0.0] * 2)) and list(info) == [0.0, math.inf, 7.0, -1.0]


@pytest.mark.parametrize("T", sc.POWER_ITERS)
def test_copies_of_one_far_row_all_end_at_exactly_zero_after_round_one(lib, T):
  sq, n, mode, count = _crafted("far-copies")
  # the weights that are kept are those of a round >= 1: made by round one's filter, in which the three bit-identical
  # rows had one tau, the largest, and all got 1 - tau / tau_max = 0 exactly
  code, weights, info = sc.host_weights(lib, sq, n, mode, count, T)
  assert code == 0 and info[3] >= 1
  assert np.array_equal(weights[8:11], np.zeros(3)) and (weights[:8] > 0).all()
  w, _ = _run(lib, "far-copies-dnc", T)
  assert np.array_equal(w, np.array([0.125] * 8 + [0.0] * 3))


def test_nan_rows_are_unusable_and_count_as_filtered_mass(lib):
  sq, n, mode, count = _crafted("nan-rows")     # 2 NaN rows, f = 3: the threshold stays 11 - 6 = 5, U = 9
  code, weights, info = sc.host_weights(lib, sq, n, mode, count, 16)
  assert code == 0 and info[2] == 9 and weights[2] == 0 and weights[5] == 0 and info[0] >= 1
  assert abs(weights[:11].sum() - 1.0) <= 1e-12
  # the same as the rule on the nine rows with f chosen so that the threshold is the same: 9 - 2 f' = 5
  keep = [i for i in range(11) if i not in (2, 5)]
  clean = sq[np.ix_(keep, keep)]
  code2, expect, info2 = sc.host_weights(lib, clean, 9, mode, 2, 16)
  assert code2 == 0 and info2[0] == info[0] and info2[3] == info[3]
  np.testing.assert_allclose(weights[keep], expect[:9], rtol=1e-12, atol=1e-15)
  # U <= n - 2f: no round, the mean of the usable rows
  for name, usable in (("nan-rows-mean", 8), ("nan-rows-at-floor", 9)):
    w, info = _run(lib, name)
    assert np.array_equal(w, np.array([1.0 / usable] * usable + [0.0] * (11 - usable)))
    assert list(info) == [0.0, math.inf, float(usable), -1.0]


def test_no_usable_row_gives_nan_weights(lib):
  for name in ("no-usable-row", "no-usable-row-dnc"):
    sq, n, mode, count = _crafted(name)
    code, weights, info = sc.host_weights(lib, sq, n, mode, count, 16)
    assert code == 0 and np.isnan(weights[:n]).all() and not weights[n:].any()
    assert list(info) == [0.0, math.inf, 0.0, -1.0]


def test_dnc_ties_between_identical_rows_remove_the_higher_index(lib):
  sq, n, mode, count = _crafted("far-copies-dnc")   # rows 8, 9, 10 are bit-identical
  for k, gone in ((1, [10]), (2, [9, 10]), (3, [8, 9, 10])):
    code, weights, _ = sc.host_weights(lib, sq, n, "dnc", k, 16)
    assert code == 0
    assert [i for i in range(n) if weights[i] == 0] == gone
    assert np.array_equal(weights[[i for i in range(n) if i not in gone]], np.full(n - k, 1.0 / (n - k)))


def test_dnc_removes_fewer_rows_when_some_are_unusable(lib):
  sq, n, mode, count = _crafted("nan-rows-dnc")     # k = 3, two unusable rows: one more usable row goes
  code, weights, info = sc.host_weights(lib, sq, n, mode, count, 16)
  assert code == 0 and info[2] == 9
  assert [i for i in range(n) if weights[i] == 0] == [2, 5, 10]
  assert np.array_equal(weights[[0, 1, 3, 4, 6, 7, 8, 9]], np.full(8, 0.125))
  code, weights, _ = sc.host_weights(lib, sq, n, mode, 2, 16)   # k = n - U: nothing more to remove
  assert [i for i in range(n) if weights[i] == 0] == [2, 5]


def test_bad_arguments_are_refused(lib):
  from byzantinemomentum_amd import _lib
  sq = np.zeros((64, 64))
  ok = dict(n=11, mode="caf", count=2, T=16)

  def code(**change):
    a = dict(ok, **change)
    return sc.host_weights(lib, sq, a["n"], a["mode"], a["count"], a["T"])[0]

  assert code() == 0
  assert code(count=5) == 0 and code(count=6) == _lib.EINVAL and code(n=10, count=5) == _lib.EINVAL   # 2 f >= n
  assert code(count=-1) == _lib.EINVAL
  assert code(mode="dnc", count=10) == 0 and code(mode="dnc", count=11) == _lib.EINVAL              # k >= n
  assert code(mode="dnc", count=-1) == _lib.EINVAL
  assert code(T=0) == _lib.EINVAL and code(T=257) == _lib.EINVAL and code(T=256) == 0 and code(T=1) == 0
  assert code(n=0) == _lib.EINVAL and code(n=65) == _lib.EINVAL and code(n=64) == 0
  buf = (ctypes.c_double * (64 * 64))()
  assert lib.bm_spectral_weights(buf, 11, 2, 2, 16, buf, buf) == _lib.EINVAL    # no such mode
  assert lib.bm_spectral_weights(buf, 11, -1, 2, 16, buf, buf) == _lib.EINVAL
  assert lib.bm_spectral_weights(None, 11, 0, 2, 16, buf, buf) == _lib.EINVAL
  assert lib.bm_spectral_weights(buf, 11, 0, 2, 16, None, buf) == _lib.EINVAL
  assert lib.bm_spectral_weights(buf, 11, 0, 2, 16, buf, None) == _lib.EINVAL
  # the device form refuses before any HIP call (no GPU here)
  assert lib.bm_spectral_weights_device(buf, 11, 0, 6, 16, buf, buf, None) == _lib.EINVAL
  assert lib.bm_spectral_weights_device(buf, 11, 1, 11, 16, buf, buf, None) == _lib.EINVAL
  assert lib.bm_spectral_weights_device(buf, 11, 0, 2, 0, buf, buf, None) == _lib.EINVAL
  assert lib.bm_spectral_weights_device(buf, 11, 0, 2, 257, buf, buf, None) == _lib.EINVAL
  assert lib.bm_spectral_weights_device(buf, 11, 2, 2, 16, buf, buf, None) == _lib.EINVAL
  assert lib.bm_spectral_weights_device(buf, 65, 0, 2, 16, buf, buf, None) == _lib.EINVAL
  assert lib.bm_spectral_weights_device(None, 11, 0, 2, 16, buf, buf, None) == _lib.EINVAL
  assert lib.bm_spectral_weights_device(buf, 11, 0, 2, 16, None, buf, None) == _lib.EINVAL
  assert lib.bm_spectral_weights_device(buf, 11, 0, 2, 16, buf, None, None) == _lib.EINVAL


def test_one_lane_form_gives_the_same_rule(lib):
  """BM_SPECTRAL_LANES = 1 (the A/B knob of profiles/spectral_timings.txt) changes the order of the additions inside a
  row-dot and nothing else: the same decisions, the weights within the bar."""
  case = sc.cases()[5]
  rows, _ = sc.make_rows(case)
  sq = sc.exact_sqdist(rows)
  _, four, info4 = sc.host_weights(lib, sq, case.n, "caf", case.k, 16)
  assert lib.bm_tuning_set(b"BM_SPECTRAL_LANES", 1) == 0
  try:
    _, one, info1 = sc.host_weights(lib, sq, case.n, "caf", case.k, 16)
  finally:
    assert lib.bm_tuning_set(b"BM_SPECTRAL_LANES", 0) == 0
  assert info1[0] == info4[0] and info1[3] == info4[3]
  assert float(np.abs(one - four).max()) <= BAR


def test_header_exports_and_bindings():
  import pathlib
  import byzantinemomentum_amd as bm
  lib = bm._lib.load()
  header = (pathlib.Path(bm.__file__).resolve().parent.parent / "include" / "bm_gar.h").read_text()
  for name in ("bm_spectral_weights", "bm_spectral_weights_device"):
    assert f"int {name}(" in header and name in bm._lib.SIGNATURES and hasattr(lib, name), name
  assert "BM_SPECTRAL_CAF = 0" in header and "BM_SPECTRAL_DNC = 1" in header
  assert bm._lib.SPECTRAL_MODES == {"caf": 0, "dnc": 1} and bm._lib.SPECTRAL_MAX_POWER_ITERS == 256
  assert bm._lib.ABI_VERSION == 23 and lib.bm_abi_version() == 23
