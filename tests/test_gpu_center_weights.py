"""bm_center_weights_device against bm_center_weights, bit for bit (weights and info): the two run ONE definition of
the iteration (csrc/center_core.h) and the library is built without floating-point contraction — on the matrices of
test_center_weights_cpu.py, on matrices the device distance pass produced, at 1, 3 and 64 iterations, both modes,
with and without a start vector.  Needs an MI355X: `pytest -m gpu`."""

import math

import numpy as np
import pytest
import torch

from tests import center_cases as cc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ITERS = (1, 3, 64)


@pytest.fixture(scope="module")
def bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


def _same_bits(a, b):
  return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _compare(bm, sq, n, mode, param, iters, tol, has_start, tag):
  """sq: float64 numpy N x N.  Device form on a device copy, host form on the matrix itself."""
  lib = bm._lib.load()
  sq = np.ascontiguousarray(sq, dtype=np.float64)
  code, want, want_info = cc.host_weights(lib, sq, n, mode, param, iters, tol, has_start)
  assert code == 0, tag
  got, info = bm.gars.center_weights(torch.from_numpy(sq).to(DEV), n, mode, param, iters, tol, has_start)
  got, info = got.cpu().numpy(), info.cpu().numpy()
  assert _same_bits(got, want), (tag, got[:n + 1], want[:n + 1])
  assert _same_bits(info, want_info), (tag, info, want_info)
  # the host wrapper (a host matrix) is the host form
  again, again_info = bm.gars.center_weights(torch.from_numpy(sq), n, mode, param, iters, tol, has_start)
  assert _same_bits(again.numpy(), want) and _same_bits(again_info.numpy(), want_info)
  return want, want_info


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("mode", ["geomed", "cclip"])
@pytest.mark.parametrize("case", cc.cases(), ids=cc.case_id)
def test_exact_matrices_of_the_cpu_cases(bm, case, mode, iters):
  rows, start = cc.make_rows(case)
  param, _ = cc.params(case, mode)
  sq = cc.exact_sqdist(np.concatenate([rows, start[None, :]]))
  n = case.n
  _compare(bm, sq[:n, :n], n, mode, param, iters, 0.0, False, (cc.case_id(case), mode, iters, "no start"))
  _compare(bm, sq, n, mode, param, iters, 0.0, True, (cc.case_id(case), mode, iters, "start"))


@pytest.mark.parametrize("mode", ["geomed", "cclip"])
@pytest.mark.parametrize("case", cc.cases()[::3], ids=cc.case_id)
def test_matrices_of_the_device_distance_pass(bm, case, mode):
  rows, start = cc.make_rows(case)
  param, _ = cc.params(case, mode)
  byz = torch.from_numpy(rows[-1].copy()).to(DEV)
  dev = [torch.from_numpy(r.copy()).to(DEV) for r in rows[:case.n - case.k]] + [byz] * case.k
  nan_row = torch.full_like(byz, math.nan)
  for stack, tag in ((dev, "as is"), (dev[:case.n - case.k] + [nan_row] * case.k, "nan attack")):
    for has_start in (False, True):
      points = stack + ([torch.from_numpy(start).to(DEV)] if has_start else [])
      sq = bm.gars.pairwise_sqdist(points).cpu().numpy()
      for iters in ITERS:
        want, info = _compare(bm, sq, case.n, mode, param, iters, 0.0, has_start, (cc.case_id(case), mode, tag, has_start, iters))
        if tag == "nan attack" and 2 * case.k < case.n - 1:
          assert info[2] == case.n - case.k and not want[case.n - case.k:case.n].any() and np.isfinite(want).all()


@pytest.mark.parametrize("mode", ["geomed", "cclip"])
def test_crafted_matrices(bm, mode):
  param = 1e-6 if mode == "geomed" else 1.0
  for iters in ITERS:
    _compare(bm, np.zeros((1, 1)), 1, mode, param, iters, 0.0, False, "n = 1")
    _compare(bm, np.array([[0.0, 4.0], [4.0, 0.0]]), 1, mode, param, iters, 0.0, True, "n = 1 and a start")
    _compare(bm, np.array([[0.0, 9.0], [9.0, 0.0]]), 2, mode, param, iters, 0.0, False, "n = 2")
    _compare(bm, np.zeros((3, 3)), 3, mode, param, iters, 0.0, False, "distance zero")
  rng = np.random.default_rng(64)
  pts = rng.normal(size=(64, 37)).astype(np.float32)
  pts[-5:] = pts[-1] + 20.0
  sq = cc.exact_sqdist(pts)
  big = 4.0 if mode == "cclip" else 1e-6
  for iters in ITERS:
    _compare(bm, sq, 64, mode, big, iters, 0.0, False, "N = 64")
    _compare(bm, sq, 63, mode, big, iters, 0.0, True, "N = 64 with a start")
  # NaN rows: a minority (excluded), a majority (every weight NaN), a NaN start (the uniform start)
  case = cc.cases()[0]
  rows, start = cc.make_rows(case)
  p, _ = cc.params(case, mode)
  full = cc.exact_sqdist(np.concatenate([rows, start[None, :]]))
  for which, has_start in (([8, 9, 10], False), ([2, 5, 6], True), (list(range(5, 11)), False), ([11], True)):
    bad = full.copy()
    bad[which, :] = math.nan
    bad[:, which] = math.nan
    N = 12 if has_start else 11
    for iters in ITERS:
      want, info = _compare(bm, bad[:N, :N], 11, mode, p, iters, 0.0, has_start, ("nan rows", which, iters))
    if len(which) == 6:
      assert np.isnan(want[:11]).all()
  # early stop by tol: both sides stop at the same iteration
  case = cc.cases()[4]
  rows, _ = cc.make_rows(case)
  if mode == "geomed":
    _, info = _compare(bm, cc.exact_sqdist(rows), case.n, mode, 1e-6 * math.sqrt(case.d), 32, 1e-3, False, "tol")
    assert 1 < info[0] < 32


def test_bad_arguments_launch_nothing(bm):
  sq = torch.zeros((11, 11), dtype=torch.float64, device=DEV)
  for bad in (dict(iters=0), dict(iters=65), dict(param=0.0), dict(param=-1.0), dict(tol=-1.0)):
    args = dict(dict(param=1.0, iters=3, tol=0.0), **bad)
    with pytest.raises(ValueError):
      bm.gars.center_weights(sq, 11, "cclip", args["param"], args["iters"], args["tol"])
  with pytest.raises(bm.gars.GarInputError):
    bm.gars.center_weights(sq, 11, "cclip", 1.0, 3, 0.0, has_start=True)     # the matrix holds 11 x 11, not 12 x 12
  with pytest.raises(bm.gars.GarInputError):
    bm.gars.center_weights(torch.zeros((65, 65), dtype=torch.float64, device=DEV), 64, "cclip", 1.0, 3, 0.0, has_start=True)
