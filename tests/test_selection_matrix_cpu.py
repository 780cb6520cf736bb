"""The mirror of tests/selection_matrix.py against the sources, its references against what the project already trusts,
and every claim tests/test_gpu_selection_matrix.py makes about its inputs (no GPU needed): the exactness of the exact
ranking matrices in integers and fractions, tied scores where they are claimed, the order sensitivity of the
selected-mean inputs, the instances the mean cases reach, the paths of the device Brute search its cases reach (by the
phase-by-phase model of tests/test_brute_parallel_model.py) and its node counts, and that the case lists leave nothing
out."""

import math
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import gar_oracle as O
from tests import selection_matrix as S
from tests.test_brute_parallel_model import PATHS, search_paths
from tests.test_host_logic import _brute_select
from tests.test_instance_matrix_cpu import HEADER, _read, c_eval

RANK = _read("rank_body.h")
PAIR = _read("pairwise.hip")
REDUCE = _read("reduce.hip")
PLAN = _read("launch_plan.h")
BRUTE = _read("brute.hip")
API = _read("api.cpp")
CUS = (256, 304)


def _int(text, name):
  m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*([^;]+);", text)
  assert m, name
  return c_eval(m.group(1).replace("1 << 18", str(1 << 18)), {})


# ---------------------------------------------------------------------------------------------------------------------
# The mirror against the sources

def test_constants():
  assert int(re.search(r"#define\s+BM_MAX_ROWS\s+(\d+)", HEADER.read_text()).group(1)) == S.BM_MAX_ROWS
  ranks = dict(re.findall(r"\b(BM_RANK_[A-Z]+)\s*=\s*(\d+)", HEADER.read_text()))
  assert (int(ranks["BM_RANK_KRUM"]), int(ranks["BM_RANK_BULYAN"])) == (S.RANK_KRUM, S.RANK_BULYAN)
  assert _int(PAIR, "kRankThreads") == S.K_RANK_THREADS
  assert _int(REDUCE, "kRedBlock") == S.K_RED_BLOCK
  assert _int(REDUCE, "kMeanMaxBlocks") == S.K_MEAN_MAX_BLOCKS
  assert _int(REDUCE, "kMeanBurstThreads") == S.K_MEAN_BURST_THREADS
  assert _int(REDUCE, "kMeanBurstSlots") == S.K_MEAN_BURST_SLOTS
  assert _int(BRUTE, "kBruteWaves") == S.K_BRUTE_WAVES
  assert _int(BRUTE, "kBruteNodeBudgetPerWave") == S.K_BRUTE_NODE_BUDGET_PER_WAVE
  for knob, value in S.DEFAULT_KNOBS.items():
    assert int(re.search(r'env_int\("' + knob + r'", (\d+)\)', API).group(1)) == value, knob
    assert '{"' + knob + '", &t.' in API  # settable in-process
  # the launch of bm_krum_rank and of the selected mean, the caps and the tail mode the mirror assumes
  assert "dim3(1), dim3(kRankThreads), rank_lds_bytes(n)" in PAIR and "rank_bitonic(n) ? 1 : 0);" in PAIR
  assert "for_body_and_tail<4>(Tail::kRidesNarrowed, vec, d, kRedBlock, caps_of(kMeanMaxBlocks)" in REDUCE
  assert "const int vec = Alignment().of(rows, n).of(out).vec();" in REDUCE
  assert "while (mode == Tail::kRidesNarrowed && vec > 1 && d / vec == 0) vec /= 2;" in PLAN
  assert "dim3(cus), dim3(kMeanBurstThreads)" in REDUCE and "dim3(1), dim3(64 * kBruteWaves)" in BRUTE


def test_rank_dispatch_expression():
  expr = re.search(r"inline bool rank_bitonic\(int n\) \{\s*const int algo = tuning\(\)\.rank_algo;\s*return ([^;]+);",
                   RANK).group(1)
  for n in range(1, S.BM_MAX_ROWS + 1):
    for algo in S.RANK_ALGOS:
      assert bool(c_eval(expr, {"algo": algo, "n": n})) == S.rank_bitonic(n, algo), (n, algo)


def test_mean_burst_expression():
  body = re.search(r"if constexpr \(VEC == 4\) \{.*?if \((tuning\(\)\.mean_burst > 0.+?)\) \{\n", REDUCE, re.S)
  expr = re.sub(r"\s+", " ", body.group(1)).replace("(int64_t)", "").replace("tuning().mean_burst", "knob")
  expr = expr.replace("(1 << 30)", str(1 << 30))
  for cus in CUS + (64,):
    span = cus * S.K_MEAN_BURST_THREADS
    for knob in (0, 1, 8):
      for m in (1, 11, 12, 64):
        for nvec in (0, 1, span - 1, span, 8 * span - 1, 8 * span, (1 << 30) - 1, 1 << 30):
          env = {"knob": knob, "m": m, "nvec": nvec, "cus": cus, "kMeanBurstThreads": S.K_MEAN_BURST_THREADS}
          assert bool(c_eval(expr, env)) == S.mean_burst(4, m, nvec, cus, knob), env
  assert not S.mean_burst(2, 64, 1 << 29, 256, 1)


# ---------------------------------------------------------------------------------------------------------------------
# The ranking: reference, exactness, ties, completeness

@pytest.mark.parametrize("kind", ["hetero", "tight", "iid"])
def test_rank_reference_is_the_oracles(kind):
  """rank_reference on the squared float64 distances of a stack is O.krum_order / O.bulyan_order of that stack."""
  for n, f in ((5, 1), (11, 2), (25, 5), (40, 9)):
    rows, _ = O.make_stack(kind, n, f, 257, seed=3 * n + f)
    dist = O.pairwise_distances(rows, "f64")
    m = n - f - 2
    want_order, want_scores = O.krum_order(rows, f, "f64")
    got_order, got_scores = S.rank_reference(dist * dist, n, f, m, S.RANK_KRUM)
    # (sqrt(x * x) is x again for these magnitudes or off by rounding: the scores then agree to the last bits)
    assert got_order == want_order and np.allclose(got_scores, want_scores, rtol=1e-15, atol=0)
    want_order, want_scores = O.bulyan_order(rows, f, m, "f64")
    got_order, got_scores = S.rank_reference(dist * dist, n, f, m, S.RANK_BULYAN)
    assert got_order == want_order and np.allclose(got_scores, want_scores, rtol=1e-15, atol=0)


def test_exact_kind_is_exact():
  """Squares, square roots and sums of the exact matrices recomputed in integers and fractions: each square is the
  fraction k^2 / 2^20, its fp64 square root is k / 1024, and every score of the reference is the exact sum."""
  for kind, sub in S.RANK_KINDS:
    if kind != "exact":
      continue
    for n in range(1, S.BM_MAX_ROWS + 1):
      rng = np.random.default_rng([S.RANK_KINDS.index((kind, sub)), n])
      k = S.rank_integers(sub, n, rng)
      assert (k == k.T).all() and int(k.max(initial=0)) < (1 << 20) and not k.diagonal().any()
      sq = S.rank_matrix(kind, sub, n)
      off = ~np.eye(n, dtype=bool)
      assert (sq == sq.T)[off].all()
      assert all(math.isnan(sq[i, i]) if i % 2 == 0 else sq[i, i] == -1.0 for i in range(n))
      for i in range(n):
        for j in range(n):
          if i != j:
            assert Fraction(float(sq[i, j])) == Fraction(int(k[i, j]) ** 2, 1 << 20)
            assert Fraction(math.sqrt(sq[i, j])) == Fraction(int(k[i, j]), 1024)
      for c in (c for c in S.rank_cases(kind, sub) if c.n == n):
        take = S.rank_take(n, c.f, c.m, c.mode)
        _, scores = S.rank_reference(sq, n, c.f, c.m, c.mode)
        for i in range(n):
          smallest = sorted(int(k[i, j]) for j in range(n) if j != i)[:take]
          assert Fraction(scores[i]) == Fraction(sum(smallest), 1024), (sub, n, c, i)


def test_tied_scores_where_claimed():
  """The lattice and the block sub-kinds tie scores at every n >= 3, in every case; equal distances tie them all; the
  rows of the non-finite kinds reach +inf scores that tie."""
  inf_ties = 0
  for kind, sub in S.RANK_KINDS:
    for n in range(3, S.BM_MAX_ROWS + 1):
      sq = S.rank_matrix(kind, sub, n)
      for c in (c for c in S.rank_cases(kind, sub) if c.n == n):
        order, scores = S.rank_reference(sq, n, c.f, c.m, c.mode)
        if sub in S.TIED_SUBKINDS:
          assert len(set(scores)) < n, (sub, c)
        if sub == "equal":
          assert len(set(scores)) == 1 and order == list(range(n))
        if kind == "nonfinite":
          inf_ties += sum(1 for s in scores if s == math.inf) >= 2
        # ties go to the lower index
        assert all(scores[a] < scores[b] or (scores[a] == scores[b] and a < b) for a, b in zip(order, order[1:]))
  assert inf_ties > 3 * 62


def test_rank_cases_leave_nothing_out():
  cases = S.rank_cases()
  for kind, sub in S.RANK_KINDS:
    for mode in (S.RANK_KRUM, S.RANK_BULYAN):
      assert {c.n for c in cases if (c.kind, c.sub, c.mode) == (kind, sub, mode)} == set(range(1, 65))
  for n in range(1, 65):  # both sort forms at every n: every case runs under the three settings
    assert {S.rank_bitonic(n, a) for a in S.RANK_ALGOS} == {True, False}
    assert S.rank_bitonic(n) == (n > 32)
    fs, ms = S.rank_shapes(n)
    assert {n - 1, n} <= set(fs) and 0 in fs
    if n >= 3:
      assert {S.f_main(n), n - 3} <= set(fs) and all(1 <= m <= n - 2 for m in ms) and {1, n - 2} <= set(ms)
      assert all(any(m <= n - f - 2 for f in fs) for m in ms)
    else:
      assert ms == [1]
  # Krum's edge in the reference: nothing to add
  assert S.rank_reference(S.rank_matrix("exact", "continuous", 5), 5, 4, 0, S.RANK_KRUM) == (list(range(5)), [0.0] * 5)


def test_integer_stacks_hold_tied_scores():
  for n in S.LATTICE_STACK_N:
    vals, rowmap = S.lattice_stack(n)
    sq = S.integer_sqdist(vals, rowmap)
    assert int(np.abs(vals).max()) <= 2 and int(sq.max()) < (1 << 24) and len(rowmap) == n
    f = max(1, S.f_main(n))
    for mode in (S.RANK_KRUM, S.RANK_BULYAN):
      _, scores = S.rank_reference(sq.astype(np.float64), n, f, max(1, n - f - 2), mode)
      assert n < 4 or len(set(scores)) < n


# ---------------------------------------------------------------------------------------------------------------------
# The argsort

def test_argsort_inputs_hold_what_they_claim():
  for n in range(1, 65):
    for kind in S.ARGSORT_KINDS:
      keys = S.argsort_keys(kind, n)
      order = S.argsort_reference(keys)
      assert sorted(order) == list(range(n))
      k = [math.inf if math.isnan(v) else v for v in keys]
      assert all(k[a] < k[b] or (k[a] == k[b] and a < b) for a, b in zip(order, order[1:]))
    assert math.isnan(S.argsort_keys("nan_first", n)[0]) and math.isnan(S.argsort_keys("nan_last", n)[n - 1])
    assert math.isnan(S.argsort_keys("nan_middle", n)[n // 2])
    if n >= 8:
      assert len(set(S.argsort_keys("distinct", n))) == n and len(set(S.argsort_keys("equal", n))) == 1
      assert np.isnan(S.argsort_keys("nans", n)).sum() >= 2
      mixed = S.argsort_keys("inf_nan", n)
      assert np.isnan(mixed).any() and np.isposinf(mixed).any() and np.isfinite(mixed).any()
      assert np.isneginf(S.argsort_keys("neg_inf", n)).any()
  zeros = S.argsort_keys("zeros", 64)
  assert (np.signbit(zeros) & (zeros == 0)).any() and (~np.signbit(zeros) & (zeros == 0)).any()


# ---------------------------------------------------------------------------------------------------------------------
# The selected mean

def test_mean_reference_is_the_oracles_sequential_mean():
  rows, _ = O.make_stack("hetero", 9, 2, 515, seed=4)
  idx = [4, 0, 7, 2, 5]
  assert torch.equal(S.mean_reference(rows, idx + [-1], 5), O._seq_sum_div([rows[i] for i in idx], 5))
  assert bool(S.mean_reference(rows, [4, -1, 2], 3).isnan().all()) and not S.mean_reference(rows, [4, 1, -1], 2).isnan().any()


def _small(case):
  return case if case.d <= 4099 else case._replace(d=4099)


@pytest.mark.parametrize("group", S.MEAN_GROUPS)
def test_mean_inputs_are_order_sensitive(group):
  """For each table: summing in the reverse order (from three entries on — two commute) or without the last entry
  (from two on) changes the reference's bits in at least 10 % of the columns (long cases: on their first 4 099); the
  special columns give +0.0, +inf, NaN and a finite value."""
  for case in S.mean_cases(group):
    idx = list(case.table[:case.m])
    if any(i < 0 for i in idx) or case.d < 16:
      continue
    case = _small(case)
    rows = list(S.mean_values(case))
    want = S.mean_reference(rows, idx, case.m)
    c_zero, c_inf, c_both, c_nan = S.SPECIAL_COLUMNS
    assert want[c_zero] == 0 and not math.copysign(1, want[c_zero]) < 0 and want[c_inf] == math.inf
    assert want[case.d - 1] == 0 and not math.copysign(1, want[case.d - 1]) < 0
    if len(set(idx)) >= 2:
      assert math.isnan(want[c_both])
    assert math.isfinite(want[c_nan]) and (len(set(idx)) == case.n or any(r[c_nan].isnan() for r in rows))
    bits = want.view(torch.int32)
    if case.m >= 3 and idx[::-1] != idx:
      other = S.mean_reference(rows, idx[::-1], case.m).view(torch.int32)
      assert float((other != bits).float().mean()) >= 0.1, ("reversed", case.group, case.n, case.m)
    if case.m >= 2:
      acc = S.mean_reference(rows, idx[:-1], case.m - 1) * (case.m - 1) / case.m  # (the row dropped, the divisor kept)
      assert float((acc.view(torch.int32) != bits).float().mean()) >= 0.1, ("dropped", case.group, case.n, case.m)


def test_mean_cases_reach_the_instances_claimed():
  assert {c.m for c in S.mean_cases("every_m")} == set(range(1, 65))
  assert {c.m % 8 for c in S.mean_cases("every_m")} == set(range(8))
  assert {c.offset for c in S.mean_cases("every_m")} == {0, 4, 8, "mixed"}
  for c in S.mean_cases("every_m"):
    assert sorted(c.table[:c.m]) == sorted(set(c.table[:c.m])) and all(i == -1 for i in c.table[c.m:]) and len(c.table) == 64
  for cus in CUS:
    reached = set()
    for group in S.MEAN_GROUPS:
      for c in S.mean_cases(group, cus):
        reached |= S.mean_instances(c, cus)
        if group != "burst":
          assert all(form == "plain" for form, _ in S.mean_instances(c, cus))
    assert reached == {("plain", 4), ("plain", 2), ("plain", 1), ("burst", 4)}
    burst = S.mean_cases("burst", cus)
    assert all(S.mean_instances(c, cus) == {("burst", 4)} and c.m >= 12 and c.d % 4 == 3 for c in burst)
    assert sorted({S.burst_iterations(c, cus) for c in burst}) == [1, 2, 9, 10] and {c.m for c in burst} == {12, 37}
    assert any(-1 in c.table[:c.m] for c in burst)
    assert all(len(set(c.table[:c.m]) - {-1}) == 3 for c in burst)
  for c in S.mean_cases("trip"):
    assert S.mean_grid(c) == (S.K_MEAN_MAX_BLOCKS, 2) and c.d % 4 == 3
  assert [S.mean_width(c) for c in S.mean_cases("trip")] == [1, 4]
  negative = S.mean_cases("negative")
  assert {(S.mean_width(c), c.d) for c in negative} == {(4, 2051), (2, 2051), (1, 2051), (2, 3), (1, 3)}
  assert {tuple(i < 0 for i in c.table[:c.m]) for c in negative} == {
      (True, False, False, False), (False, False, False, True), (True,), (True,) * 4}
  repeated = S.mean_cases("repeated")
  assert {(c.n, c.m) for c in repeated} == {(3, 64), (11, 12), (1, 1)}
  assert all(c.table[11] == c.table[0] for c in repeated if c.n == 11)
  assert {(c.d, S.mean_width(c)) for c in S.mean_cases("short") if c.offset == 0} == {(1, 1), (2, 2), (3, 2), (5, 4), (7, 4)}


# ---------------------------------------------------------------------------------------------------------------------
# The Brute search

@pytest.fixture(scope="module")
def brute_paths():
  out = {}
  for case in S.all_brute_cases():
    dist = S.brute_distances(S.brute_matrix(case))
    out[case] = (dist,) + search_paths(dist, case.n, case.f)
  return out


def test_brute_model_is_the_host_search_on_every_case(brute_paths):
  for case, (dist, status, sel, _, nodes, _) in brute_paths.items():
    rc, want = _brute_select(dist, case.n, case.f)
    assert (status == 0) == (rc == 0), case
    if rc == 0:
      assert sel == want, case
      if case.n <= 12:
        assert sel == O.brute_selection_from_distances(dist, case.f), case
    # no case comes near the node budget
    assert nodes < S.K_BRUTE_NODE_BUDGET_PER_WAVE // 64, (case, nodes)


def test_brute_cases_reach_the_paths_claimed(brute_paths):
  reached = {g: set() for g in S.BRUTE_GROUPS}
  rounds = {g: 0 for g in S.BRUTE_GROUPS}
  for case, (_, _, _, paths, _, rounds3b) in brute_paths.items():
    assert paths <= set(PATHS)
    reached[case.group] |= paths
    rounds[case.group] = max(rounds[case.group], rounds3b)
  assert reached["ties"] == set(PATHS) and rounds["ties"] >= 2
  crafted = {c.kind: brute_paths[c] for c in S.brute_cases("ties") if c.kind in S.BRUTE_CRAFTED}
  assert {"skipped_then_accepted", "row63_chosen", "3b_rounds"} <= crafted["skip_then_63"][3]
  assert crafted["skip_then_63"][2] == list(range(59)) + [62, 63]
  assert "shortcut_after_chosen" in crafted["shortcut"][3] and crafted["shortcut"][2] == [0] + list(range(2, 20))
  assert crafted["last_round"][2] == list(range(62)) and crafted["last_round"][5] == 4
  lattice = [brute_paths[c] for c in S.brute_cases("ties") if c.kind == "lattice"]
  assert {n for c in S.brute_cases("ties") if c.kind == "lattice" for n in (c.n,)} == set(S.BRUTE_TIE_N)
  assert any(p[5] >= 2 for p in lattice) and any("shortcut_after_chosen" in p[3] for p in lattice)
  # all distances equal with f >= 1 at 64 rows: 16 rows per round, the 17th open row must not count as tried
  flat = {(c.n, c.f, c.kind): brute_paths[c] for c in S.brute_cases("flat")}
  assert flat[(64, 1, "equal")][2] == list(range(63)) and flat[(64, 1, "equal")][5] == 4
  assert flat[(64, 8, "zero")][2] == list(range(56))


def test_brute_cases_leave_nothing_out(brute_paths):
  every = S.brute_cases("every_n")
  for n in range(1, 65):
    assert {c.f for c in every if c.n == n} == {f for f in (0, 1, S.f_brute(n)) if n - f >= 1}
  assert S.f_brute(33) == 8 and S.f_brute(12) == 2
  assert {(c.n, c.f) for c in S.brute_cases("few_open")} == {(n, f) for n in (2, 3, 4) for f in range(n)}
  for case in S.brute_cases("nonfinite"):
    dist, status, sel = brute_paths[case][:3]
    bad = [i for i in range(case.n) if all(not math.isfinite(dist[i, j]) for j in range(case.n) if j != i)]
    if case.kind == "bad_f":
      assert len(bad) == case.f >= 1 and status == 0 and not set(sel) & set(bad)
    elif case.kind == "bad_f_plus_1":
      assert len(bad) == case.f + 1 and status == -1 and S.first_all_bad_row(dist) == bad[0]
    else:
      assert not bad and status == 0 and not math.isfinite(dist[1, case.n - 2])
  # what the kernel is given: nothing but the strict upper triangle
  given = S.brute_device_input(S.brute_matrix(every[-1]))
  assert all(math.isnan(given[i, j]) for i in range(64) for j in range(i + 1)) and np.isfinite(np.triu(given, 1)[np.triu_indices(64, 1)]).all()
