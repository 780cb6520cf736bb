"""Every compiled instance of the n x n squared-distance pass against float64 (tests/distance_matrix.py): the Gram
kernel at every row count, plane count, alignment and in both of its loops, the slices of its reduction, the direct
kernel at every geometry on the whole stack and on every size of gated sub-stack, the ranking inside those launches,
and rows with non-finite coordinates.

The bars are the suite's own (tests/pair_mode_check.py, test_gpu_parity.py::test_seeded_stack_100k): every off-diagonal
squared distance within 1e-5 of the float64 direct-difference value relative to itself (1e-6 for plain seeded stacks),
a bitwise symmetric matrix with a zero diagonal, exact zeros between aliased rows and bitwise-equal distances from them
to every third row.  Knobs the library reads once per process (BM_PAIR_MODE, BM_GRAM_STEADY) run in a child process
that holds its outputs to the same bars and prints a SHA-256 per output.  Needs an MI355X: `pytest -m gpu`.

With BM_DISTANCE_ERRORS=FILE in the environment the run also writes the worst relative error it saw per (form, K, NPL)
next to the bar it was held to — how profiles/distance_matrix_errors.txt is made.
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import gar_oracle as O
from tests import distance_matrix as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


@pytest.fixture(scope="module")
def cus():
  return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def checks():
  from tests import pair_mode_check
  return pair_mode_check


@pytest.fixture(scope="module", autouse=True)
def error_table():
  yield
  path = os.environ.get("BM_DISTANCE_ERRORS")
  if path:
    with open(path, "w") as out:
      out.write("\n".join(D.ERRORS.lines()) + "\n")


def _child(group, knobs, timeout):
  """The report of `group` from a fresh process with `knobs` set (one attempt; a crash or a timeout fails the test)."""
  env = dict(os.environ, PYTHONPATH=ROOT, **{k: str(v) for k, v in knobs})
  try:
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "distance_matrix.py"), group], cwd=ROOT,
                          env=env, capture_output=True, text=True, timeout=timeout)
  except subprocess.TimeoutExpired as err:
    pytest.fail(f"{group} child timed out after {timeout} s: {(err.stderr or b'')[-2000:]!r}")
  assert done.returncode == 0, (group, done.returncode, done.stderr[-3000:])
  res = json.loads(done.stdout.strip().splitlines()[-1])
  assert all(res["knobs"][k] == str(v) for k, v in knobs), res["knobs"]
  D.ERRORS.merge(res["worst"])
  return res


def _none(fails):
  assert not fails, (len(fails), fails[:6])


# ---------------------------------------------------------------------------------------------------------------------
# 1 + 4. Every row count, three planes, every alignment

@pytest.mark.parametrize("block", range(4))
def test_every_row_count_three_planes(bm, cus, block):
  """n = 1..64 (aliased Byzantine rows from n = 3) at the tails of a 64-coordinate Gram chunk and of the three direct
  tile widths, rows at byte offset 0 and 4 (the aligned and the unaligned Gram kernel), and at 8 and mixed at d = 257:
  the bars against float64, and the same bits at every offset — both forms read the same values in the same order."""
  todo = [c for c in D.cases("rows3", cus) if (c.n - 1) // 16 == block]
  digests = {}
  _none(D.sweep(todo, digests=digests))
  differ = D.differing_offsets(todo, digests)
  assert not differ, (len(differ), differ[:8])


# ---------------------------------------------------------------------------------------------------------------------
# 2. Two planes at short length

def test_two_planes_at_short_length(bm, cus):
  """d_total = 2^20 selects the two-plane split at d = 65 573 and 131 072, n = 4K and 4K - 3 for every K, aligned and
  unaligned.  The split keeps 16 bits and its error on a distance falls as 1 / sqrt(d) — gram_bf16.hip gives 2.8 * 2^-16
  (|x| / |x_i - x_j|) / sqrt(d); a CPU simulation of the split on iid and common-component stacks gave worst relative
  errors of 2.1e-6 at d = 256, 5e-7 at 4 096 and 1.4e-7 at 65 536 — so the 1e-6 bar holds from d = 65 536 on with about
  7x room and would fail a correct kernel at small d: no two-plane case may be shorter."""
  todo = D.cases("planes2", cus)
  assert all(D.planes(c.d_total) == 2 and c.d >= 65536 for c in todo)
  digests = {}
  _none(D.sweep(todo, digests=digests))
  differ = D.differing_offsets(todo, digests)
  assert not differ, (len(differ), differ[:8])


# ---------------------------------------------------------------------------------------------------------------------
# 3. The steady-state loop of every (K, NPL)

def test_steady_state_loop_every_instance(bm, cus):
  """n = 4K at the length at which every wave of the instance enters the condition-free loop, drains it, and some go on
  in the generic loop up to a ragged chunk (the mirror, for this device's CU count): the bars, and with
  BM_GRAM_STEADY=0 (the generic loop alone, in a child process) the same bits — "same chunks, same order per wave"."""
  todo = D.cases("steady", cus)
  for c in todo:
    npl = D.planes(c.d if c.d_total is None else c.d_total)
    in_steady, in_generic, nw = D.gram_loops(c.n, c.d, npl, True, cus)
    assert in_steady == nw and in_generic > 0, c
  digests = {}
  _none(D.sweep(todo, digests=digests))
  theirs = _child("knob_steady", (("BM_GRAM_STEADY", 0),), 300)
  _none(theirs["failures"])
  assert set(theirs["digests"]) == set(digests) and len(digests) == len(todo)
  differ = [k for k in digests if digests[k] != theirs["digests"][k]]
  assert not differ, (len(differ), differ[:8])


# ---------------------------------------------------------------------------------------------------------------------
# 4 + 5. The direct kernel on the whole stack

def test_direct_kernel_whole_stack(bm, cus):
  """BM_PAIR_MODE=1 in a child process: n = 1..64 at the lengths and offsets of the first test, plus one row count per
  tile width at a length that takes a workgroup three times through both tile buffers and ends ragged.  The child
  holds every matrix to the bars; here: the same bits at every offset (LDS-DMA against plain loads)."""
  todo = D.cases("direct_whole", cus)
  res = _child("direct_whole", (("BM_PAIR_MODE", 1),), 600)
  _none(res["failures"])
  assert len(res["digests"]) == len(todo)
  differ = D.differing_offsets(todo, res["digests"])
  assert not differ, (len(differ), differ[:8])


# ---------------------------------------------------------------------------------------------------------------------
# 6. The gated direct kernel at every sub-stack size

@pytest.mark.parametrize("n", D.GATED_N)
def test_gated_direct_kernel_every_substack_size(bm, cus, n):
  """k = 2..n rows of a hetero stack rewritten as base + 1e-4 noise, at the first k rows, the last k, spread with a
  stride, and on the rows that are no probe of the centre first; d = 2 051, and 70 001 for k = 2 and n; two aliased
  rows inside the clique; rows at byte offset 4; and stacks of near-duplicate PAIRS around unrelated bases, which list
  all n rows, or n - 1 with one row left alone, at both lengths (a clique reaches k = 2 .. n - 2 only).
  Every distance within 1e-5 of float64 relative to itself — a clique distance taken from the Gram form of rows centred
  elsewhere misses that by orders of magnitude.  The gate's row list is read back: exactly the clique where at most
  one probe row lies inside it, nothing where the centre itself falls inside the clique (the Gram form is then
  accurate for it: distance_matrix.expected_listed)."""
  fails = []
  for case in (c for c in D.cases("gated", cus) if c.n == n):
    sq, rows, rowmap = D.run_case(case)
    listed = D.listed_rows(rows)
    if listed != D.expected_listed(case):
      fails.append(f"{D.case_key(case)}: listed {listed}")
    fails += D.check_case(case, sq, rows, rowmap)
  _none(fails)


# ---------------------------------------------------------------------------------------------------------------------
# 7. Ranking inside the launches

def _rank_checks(bm, checks, case, fails, expect_listed):
  from byzantinemomentum_amd import _lib
  n = case.n
  rows, rowmap = D.device_rows(case)
  sq = bm.gars.pairwise_sqdist(rows)
  fails += D.check_case(case, sq, rows, rowmap)
  if D.rank_shape(n) is None:
    return
  f, m = D.rank_shape(n)
  dist = np.sqrt(D.sqdist_f64_on_gpu(rows))
  for mode in (_lib.RANK_KRUM, _lib.RANK_BULYAN):
    order, scores = bm.gars._rank(rows, f, m, mode)
    listed = D.listed_rows(rows)
    if bool(listed) != expect_listed:
      fails.append(f"{D.case_key(case)}: listed {listed}")
    # (rank_from_sqdist runs the same rank_body.h: it is itself anchored, against a Python float64 reference and bit
    #  for bit where the arithmetic is exact, by tests/test_gpu_selection_matrix.py)
    want_order, want_scores = bm.gars.rank_from_sqdist(sq, n, f, m, mode)
    if not torch.equal(order[:n], want_order[:n]) or not D.same_bits64(scores[:n], want_scores[:n]):
      fails.append(f"{D.case_key(case)} mode {mode}: not the ranking of the returned matrix")
    if mode == _lib.RANK_KRUM:
      s64 = O.krum_scores(dist, f)
    else:
      s64 = [O._sum_smallest([dist[i, j] for j in range(n) if j != i], m) for i in range(n)]
    if not checks.same_up_to_ties(order[:n].tolist(), O._stable_order(s64), s64):
      fails.append(f"{D.case_key(case)} mode {mode}: order {order[:n].tolist()} against float64")


def test_ranking_by_the_gram_reduction(bm, cus, checks):
  """Plain stacks of n = 1..64 list nothing, so the last workgroup of the Gram reduction ranks (Krum and Bulyan modes):
  order and scores bit-identical to bm_krum_rank on the matrix pairwise_sqdist returns for the same rows, and the order
  the float64 oracle's stable one wherever the score gap is decisive."""
  fails = []
  for case in D.cases("rank_plain", cus):
    _rank_checks(bm, checks, case, fails, expect_listed=False)
  _none(fails)


@pytest.mark.parametrize("n", D.GATED_N)
def test_ranking_by_the_gated_kernel(bm, cus, checks, n):
  """Clique stacks list rows, so the last workgroup of the gated direct kernel ranks after it has corrected them."""
  fails = []
  for case in (c for c in D.cases("rank_gated", cus) if c.n == n):
    _rank_checks(bm, checks, case, fails, expect_listed=bool(D.expected_listed(case)))
  _none(fails)


# ---------------------------------------------------------------------------------------------------------------------
# 8. Slices of the Gram reduction

def test_gram_reduction_slices(bm, cus):
  """(n, d) that the mirror says reduce in 1, 2 and 8 slices: the bars, and the matrix the ranking call returns is
  bit-identical to the plain call's."""
  from byzantinemomentum_amd import _lib
  todo = D.cases("slices", cus)
  got = [D.gram_slices(c.n, D.gram_blocks(c.n, c.d, 3, cus)) for c in todo]
  assert got == [1, 2, D.K_GRAM_SLICES_MAX], got
  fails = []
  for case in todo:
    sq, rows, rowmap = D.run_case(case)
    fails += D.check_case(case, sq, rows, rowmap)
    f, m = D.rank_shape(case.n)
    _, _, sq_rank = D.rank_with_sqdist(rows, f, m, _lib.RANK_KRUM)
    if not D.same_bits64(sq_rank, sq):
      fails.append(f"{D.case_key(case)}: the ranking call's matrix differs")
  _none(fails)


# ---------------------------------------------------------------------------------------------------------------------
# 9. Non-finite rows

def test_non_finite_rows(bm, cus):
  """One row carries NaN, +inf or -inf in every lane position of a chunk and in the ragged tail; it is in turn each
  probe row of the centre and row n - 1, the row the table repeats into the padding.  Distances among the other rows
  meet the bars, every entry with the bad row is non-finite, the matrix stays bitwise symmetric."""
  _none(D.sweep(D.cases("nonfinite", cus)))
