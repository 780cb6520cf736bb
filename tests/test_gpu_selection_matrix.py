"""The selection layer on crafted inputs (tests/selection_matrix.py): the ranking from a squared-distance matrix at
every n, in both sort forms, against a Python float64 reference bit for bit on matrices whose arithmetic is exact (ties
included: Python's stable sort decides); the ranking inside the distance pass on integer stacks; the stable argsort on
equal, NaN, infinite and signed-zero keys; the selected mean by index table, bit for bit against the sequential fp32
sum in table order; the device Brute search on the paths tests/test_selection_matrix_cpu.py proves its cases reach.
Needs an MI355X: `pytest -m gpu`."""

import numpy as np
import pytest
import torch

from oracle import gar_oracle as O
from tests import selection_matrix as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


@pytest.fixture(scope="module")
def lib():
  from byzantinemomentum_amd import _lib
  return _lib.load()


@pytest.fixture(scope="module")
def cus():
  return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def checks():
  from tests import pair_mode_check
  return pair_mode_check


def _none(fails):
  assert not fails, (len(fails), fails[:6])


def _knob(lib, name, value):
  assert lib.bm_tuning_set(name.encode(), value) == 0


# ---------------------------------------------------------------------------------------------------------------------
# a. bm_krum_rank at every n, both modes, the three BM_RANK_ALGO values

def _rank_all_algos(bm, lib, sq_dev, case):
  """[(order, scores)] of `case` under BM_RANK_ALGO 0, 1, 2 (device tensors)."""
  out = []
  try:
    for algo in S.RANK_ALGOS:
      _knob(lib, "BM_RANK_ALGO", algo)
      out.append(bm.gars.rank_from_sqdist(sq_dev, case.n, case.f, case.m, case.mode))
  finally:
    _knob(lib, "BM_RANK_ALGO", S.DEFAULT_KNOBS["BM_RANK_ALGO"])
  return out


@pytest.mark.parametrize("kind,sub", S.RANK_KINDS, ids=lambda v: v)
def test_rank_from_distances_every_row_count(bm, lib, checks, kind, sub):
  """n = 1..64, Krum (f in {0, (n-1)//4, n-3}, and n-f-1 <= 0: all-zero scores, the identity order) and Bulyan (m in
  {1, n-f-2, one between}) under BM_RANK_ALGO 0 / 1 / 2: order[:n] and scores[:n] against rank_reference — bit for bit
  on the exact and non-finite matrices (tied scores in the lattice and block sub-kinds, +inf scores in the non-finite
  ones: the lower index first), up to ties within 1e-5 and (take + 1) 2^-52 on the generic one — and the same bits from
  the three settings on every case."""
  fails, worst = [], 0.0
  for n in range(1, S.BM_MAX_ROWS + 1):
    sq = S.rank_matrix(kind, sub, n)
    sq_dev = torch.from_numpy(sq).to(DEV)
    todo = [c for c in S.rank_cases(kind, sub) if c.n == n]
    got = [_rank_all_algos(bm, lib, sq_dev, c) for c in todo]
    orders = torch.stack([o for per in got for o, _ in per]).cpu().numpy().reshape(len(todo), 3, -1)[:, :, :n]
    scores = torch.stack([s for per in got for _, s in per]).cpu().numpy().reshape(len(todo), 3, -1)[:, :, :n]
    for c, order, score in zip(todo, orders, scores):
      want_order, want_scores = S.rank_reference(sq, n, c.f, c.m, c.mode)
      tag = f"{kind}/{sub} n={n} f={c.f} m={c.m} mode={c.mode}"
      for algo in (1, 2):
        if not (np.array_equal(order[algo], order[0]) and np.array_equal(S.bits64(score[algo]), S.bits64(score[0]))):
          fails.append(f"{tag}: BM_RANK_ALGO {algo} differs from 0")
      if c.mode == S.RANK_KRUM and n - c.f - 1 <= 0:
        assert want_order == list(range(n)) and not any(want_scores)
      for algo in S.RANK_ALGOS:
        if kind == "generic":
          take = S.rank_take(n, c.f, c.m, c.mode)
          bar = (take + 1) * 2.0 ** -52
          worst = max([worst] + [abs(g - w) / w for g, w in zip(score[algo], want_scores) if w])
          if not all(abs(g - w) <= bar * abs(w) for g, w in zip(score[algo], want_scores)):
            fails.append(f"{tag} algo {algo}: scores beyond {bar:.2e}")
          if not checks.same_up_to_ties(order[algo].tolist(), want_order, want_scores):
            fails.append(f"{tag} algo {algo}: order {order[algo].tolist()} want {want_order}")
        else:
          if order[algo].tolist() != want_order:
            fails.append(f"{tag} algo {algo}: order {order[algo].tolist()} want {want_order}")
          if not np.array_equal(S.bits64(score[algo]), S.bits64(want_scores)):
            fails.append(f"{tag} algo {algo}: scores differ in bits")
  if kind == "generic":
    print("worst relative score error", worst)
  _none(fails)


# ---------------------------------------------------------------------------------------------------------------------
# b. The ranking inside the distance pass

def test_ranking_inside_the_distance_pass_on_integer_stacks(bm):
  """Stacks of integer rows (coordinates -2..2, d = 257; b aliased Byzantine rows and two equal honest rows: exact
  score ties) at n = 3, 11, 25, 32, 33, 51, 64: the matrix bm_pairwise_rank returns holds every squared distance
  exactly (against an integer computation), and its order and scores are rank_reference of that matrix bit for bit in
  both modes — the last workgroup of the distance pass runs rank_body.h on the distances it has just formed."""
  from tests import distance_matrix as D
  fails = []
  for n in S.LATTICE_STACK_N:
    vals, rowmap = S.lattice_stack(n)
    views = S.place(torch.from_numpy(vals).float().to(DEV), 0)
    rows = S.rows_of(views, rowmap)
    want_sq = S.integer_sqdist(vals, rowmap).astype(np.float64)
    f = max(1, S.f_main(n))
    m = max(1, n - f - 2)
    for mode in (S.RANK_KRUM, S.RANK_BULYAN):
      order, scores, sq = D.rank_with_sqdist(rows, f, m, mode)
      sq = sq.cpu().numpy()
      if not np.array_equal(sq, want_sq):
        fails.append(f"n={n} mode={mode}: the matrix is not the integers', worst {np.abs(sq - want_sq).max()}")
        continue
      want_order, want_scores = S.rank_reference(sq, n, f, m, mode)
      assert len(set(want_scores)) < n or n < 4
      if order[:n].tolist() != want_order:
        fails.append(f"n={n} mode={mode}: order {order[:n].tolist()} want {want_order}")
      if not np.array_equal(S.bits64(scores[:n].cpu().numpy()), S.bits64(want_scores)):
        fails.append(f"n={n} mode={mode}: scores differ in bits")
      o2, s2 = bm.gars._rank(rows, f, m, mode)
      if not (torch.equal(o2[:n], order[:n]) and torch.equal(s2[:n].view(torch.int64), scores[:n].view(torch.int64))):
        fails.append(f"n={n} mode={mode}: gars._rank differs from the same call with its matrix")
  _none(fails)


# ---------------------------------------------------------------------------------------------------------------------
# c. bm_stable_argsort

@pytest.mark.parametrize("kind", S.ARGSORT_KINDS)
def test_stable_argsort_every_row_count(bm, kind):
  """n = 1..64: the first n entries are Python's stable sort of the keys with NaN as +inf — equal keys (+inf and NaN,
  0.0 and -0.0, plain repeats) in index order."""
  fails = []
  got = [bm.gars.stable_argsort(torch.from_numpy(S.argsort_keys(kind, n)).to(DEV), n) for n in range(1, 65)]
  got = torch.stack(got).cpu().numpy()
  for n in range(1, 65):
    want = S.argsort_reference(S.argsort_keys(kind, n))
    if got[n - 1, :n].tolist() != want:
      fails.append(f"{kind} n={n}: {got[n - 1, :n].tolist()} want {want}")
  _none(fails)


# ---------------------------------------------------------------------------------------------------------------------
# d. bm_selected_mean by index table

def _mean_group(group, cus=256):
  """Runs the cases of `group`; returns (failures, {case: output})."""
  fails, outs = [], {}
  for case in S.mean_cases(group, cus):
    got, vals = S.run_mean(case)
    want = S.mean_reference(list(vals), case.table, case.m)
    if not S.same_bits_or_nan(got.cpu(), want):
      bad = ((got.cpu().view(torch.int32) != want.view(torch.int32)) & ~(got.cpu().isnan() & want.isnan())).nonzero().flatten()
      fails.append(f"{case.group} n={case.n} m={case.m} d={case.d} off={case.offset}: {len(bad)} columns, first {bad[:4].tolist()}")
    outs[case] = got
  return fails, outs


def test_selected_mean_every_m_every_offset():
  """n = 64, m = 1..64 (every remainder of the unrolled row loop), a seeded permutation as the table with -1 behind
  m, d = 2 051 at byte offsets 0 / 4 / 8 / mixed: bit for bit the sequential fp32 sum in table order divided by m
  (+0.0 from a column of -0.0, +inf, NaN from +inf and -inf, a NaN in an unselected row ignored), and the same bits at
  every offset."""
  fails, outs = _mean_group("every_m")
  assert {next(iter(S.mean_instances(c)))[1] for c in outs} == {4, 2, 1}
  for case, got in outs.items():
    if case.offset != 0 and not S.same_bits_strict(got, outs[case._replace(offset=0)]):
      fails.append(f"m={case.m} off={case.offset}: differs from offset 0")
  _none(fails)


def test_selected_mean_repeated_indices():
  """m = 64 > n = 3 (each row 21 or 22 times), the anticge table (its first entry again at the end), one row."""
  _none(_mean_group("repeated")[0])


def test_selected_mean_negative_index_is_nan_everywhere():
  """A -1 first, last, alone and everywhere, at VEC 4 / 2 / 1, d = 2 051 and d = 3: every coordinate NaN, the riding
  tail included."""
  fails, outs = _mean_group("negative")
  assert {next(iter(S.mean_instances(c)))[1] for c in outs} == {4, 2, 1}
  for case, got in outs.items():
    if not bool(got.isnan().all()):
      fails.append(f"m={case.m} d={case.d} off={case.offset}: {int((~got.isnan()).sum())} coordinates are not NaN")
  _none(fails)


def test_selected_mean_short_lengths():
  """d = 1, 2, 3, 5, 7 at offsets 0 and 8: the body narrows to the widest width with a whole vector, the rest rides."""
  cases = S.mean_cases("short")
  assert {(c.d, c.offset, S.mean_width(c)) for c in cases} == {
      (1, 0, 1), (2, 0, 2), (3, 0, 2), (5, 0, 4), (7, 0, 4), (1, 8, 1), (2, 8, 2), (3, 8, 2), (5, 8, 2), (7, 8, 2)}
  _none(_mean_group("short")[0])


def test_selected_mean_second_grid_stride_trip():
  """One block of 256 vectors more than the capped grid of 8 192 workgroups covers in one trip, and a 3-column tail, at
  VEC 1 and at VEC 4: the first workgroups take a second trip; every coordinate compared on the device."""
  fails = []
  for case in S.mean_cases("trip"):
    assert S.mean_grid(case) == (S.K_MEAN_MAX_BLOCKS, 2) and S.mean_instances(case) <= {("plain", 1), ("plain", 4)}
    got, vals = S.run_mean(case)
    want = S.mean_reference(list(vals), case.table, case.m).to(DEV)
    if not S.same_bits_or_nan(got, want):
      fails.append(f"d={case.d} off={case.offset}")
  _none(fails)


def test_selected_mean_burst_form_across_its_staging_group(lib, cus):
  """BM_MEAN_BURST = 1, three rows repeated to m = 12 and m = 37, lengths of 1, 2, 9 and 10 iterations per CU (the
  last ragged, 9 = one full staging group) plus a 3-column tail: the mirror says burst; bit-identical to the reference
  and to the plain form of the same call; with a -1 in the table all NaN."""
  from byzantinemomentum_amd import gars
  fails = []
  cases = S.mean_cases("burst", cus)
  assert sorted({S.burst_iterations(c, cus) for c in cases}) == [1, 2, S.K_MEAN_BURST_SLOTS, S.K_MEAN_BURST_SLOTS + 1]
  vals = None
  try:
    for case in cases:
      assert S.mean_instances(case, cus) == {("burst", 4)}
      assert S.mean_instances(case._replace(knobs=(("BM_MEAN_BURST", 0),)), cus) == {("plain", 4)}
      if vals is None or vals.shape[1] != case.d:
        vals = S.mean_values(case)
        rows = S.place(vals.to(DEV), case.offset)
      table = torch.tensor(case.table, dtype=torch.int32, device=DEV)
      _knob(lib, "BM_MEAN_BURST", 1)
      burst = gars.selected_mean(rows, table, case.m)
      _knob(lib, "BM_MEAN_BURST", 0)
      plain = gars.selected_mean(rows, table, case.m)
      want = S.mean_reference(list(vals), case.table, case.m).to(DEV)
      tag = f"m={case.m} d={case.d}"
      if not S.same_bits_or_nan(burst, want):
        fails.append(f"{tag}: burst form against the reference")
      if not S.same_bits_strict(burst, plain):
        fails.append(f"{tag}: burst form against the plain form")
      if -1 in case.table[:case.m] and not bool(burst.isnan().all()):
        fails.append(f"{tag}: a negative index and not all NaN")
  finally:
    _knob(lib, "BM_MEAN_BURST", S.DEFAULT_KNOBS["BM_MEAN_BURST"])
  _none(fails)


# ---------------------------------------------------------------------------------------------------------------------
# e. bm_brute_select_device

def _brute_check(bm, case, fails):
  n, f = case.n, case.f
  k = n - f
  sq = S.brute_matrix(case)
  dist = S.brute_distances(sq)
  sel, status = bm.gars.brute_select_device(torch.from_numpy(S.brute_device_input(sq)).to(DEV), n, f)
  sel, status = sel.cpu().tolist(), int(status.item())
  try:
    want = bm.gars.brute_select_host(torch.from_numpy(np.ascontiguousarray(dist)), n, f)
  except RuntimeError:
    want = None
  tag = f"{case.group}/{case.kind} n={n} f={f} seed={case.seed}"
  if any(sel[k:]):
    fails.append(f"{tag}: entries behind n - f are not zero")
  if want is None:
    if status != -1 or sel[:k] != [S.first_all_bad_row(dist)] * k:
      fails.append(f"{tag}: status {status}, table {sel[:k]} where no subset is finite")
    return
  if status != 0 or sel[:k] != want:
    fails.append(f"{tag}: status {status}, {sel[:k]} want {want}")
  elif not O.brute_selection_is_the_references(dist, f, sel[:k]):
    fails.append(f"{tag}: the oracle refuses {sel[:k]}")
  if n <= 12 and sel[:k] != O.brute_selection_from_distances(dist, f):
    fails.append(f"{tag}: not the enumeration's subset")


@pytest.mark.parametrize("block", range(4))
def test_brute_search_every_row_count(bm, block):
  """n = 1..64, f in {0, 1, min((n-1)//4, 8)}, unrelated distances and points of a line; the lower triangle and the
  diagonal are NaN (the kernel reads [x][y], x < y only): status and selection of the host search, accepted by the
  oracle's independent check, the enumeration's subset up to 12 rows, zeros behind the n - f entries."""
  fails = []
  for case in S.brute_cases("every_n"):
    if (case.n - 1) // 16 == block:
      _brute_check(bm, case, fails)
  _none(fails)


@pytest.mark.parametrize("group", ("ties", "few_open", "nonfinite", "flat"))
def test_brute_search_paths(bm, group):
  """ties: lattice points and crafted non-adjacency graphs that reach several rounds of phase 3b, a row skipped and a
  later one accepted, the "what is left is the rest" shortcut after a chosen row, and row 63 chosen in a round; few_open:
  n = 2, 3, 4 at every f (fewer open candidates than waves); nonfinite: exactly f rows at non-finite distance of
  everything (status 0, they are left out), f + 1 of them (status -1, n - f copies of the first all-bad row), one
  non-finite pair; flat: all distances zero, all equal (every subset ties: rows 0 .. n-f-1, 16 per round)."""
  fails = []
  for case in S.brute_cases(group):
    _brute_check(bm, case, fails)
  _none(fails)
