"""The host form of the attacks' factor search (csrc/linesearch.cpp over csrc/search_core.h, through
byzantinemomentum_amd.linesearch) against the float64 search on the vectors of tests/search_matrix.py, at every case of
its list and on exact distances; the conditions under which that comparison admits nothing; the proof that the cases
reach every path of the device kernel's merge; and the mirror's ties to the sources (no GPU needed).

Per case and per candidate (tests/search_matrix.py says what each piece is):
  a  the abscissae and the factor are what tools.line_maximize's restatement proposes from the objectives reported;
  b  the whole permutation in Krum and in Bulyan mode, at every abscissa of the trace and at FIXED_FACTORS, equals the
     float64 order up to rows of identical content — NO inversion is admitted, whatever the scores' distance;
  c  the objective is the float64 objective of the selection the form made, within exact_bar(kind);
  d  the trace's abscissae and the factor are the float64 vector search's;
  e  rule Average: c and d.
Conditions, recomputed here for every case this file and tests/test_gpu_search_matrix.py use (caps, not measurements):
the gap between a selected and an unselected row of different content is at least 4 G at every candidate looked at, and
the two best objectives of a search are equal or differ by at least 100 bars — 100 exact bars for every case, 100 device
bars for the cases that also run on the device's distances and for the steps.  A draw that misses is replaced by another
seed (search_matrix.RESEEDED) or by a neighbouring shape (the comments of search_matrix._cases say which and why).
What no draw can meet is named, not widened: the ties of search_matrix.structural_tie (take = 0, one honest row, two
honest rows around the candidate at t = 0), and the five (case, rule) pairs of search_matrix.ENDS_ON_START, whose Krum
search ends on its start: the cursor walks back to x = 0 in ever shorter steps and its objectives come as close as its
abscissae — d is asserted there all the same, and a test holds that each of them does miss the condition.
Mutations of search_core.h / linesearch.cpp that this file fails: CHANGELOG.md.
"""

import functools
import math
import re

import pytest
import torch

from byzantinemomentum_amd import linesearch
from oracle import gar_oracle as O
from tests import search_matrix as S
from tests.test_instance_matrix_cpu import HEADER, ROOT, _read, c_eval

DEVICE = _read("search_device.hip")
CORE = _read("search_core.h")
HOST = _read("linesearch.cpp")
COMMON = _read("bm_common.h")
STATS = (ROOT / "byzantinemomentum_amd" / "stats.py").read_text()

class HostForm:
  """byzantinemomentum_amd.linesearch on exact distances."""

  def __init__(self, case, ext):
    self.case, self.ext = case, ext
    self.args = (ext, case.h, case.k, case.f)

  def search(self, rule):
    c = self.case
    return linesearch.attack_line_search(*self.args, rule, evals=c.evals, negative=c.negative, m=c.m if rule == "krum" else None)

  def rankings(self, mode, m, ts):
    return [linesearch.attack_ranking(*self.args, mode, t, m) for t in ts]

  def objective(self, rule, t):
    return linesearch.attack_objective(*self.args, rule, t, self.case.m if rule == "krum" else None)


@functools.lru_cache(maxsize=None)
def study(case):
  """Everything this file asserts about one case; returns what it measured."""
  inputs = S.inputs_of(case)
  return S.examine(case, inputs, HostForm(case, S.exact_ext(inputs)), S.within_exact(case.kind))


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_host_form_against_the_float64_search_on_the_vectors(case):
  got = study(case)
  print("%-50s worst %.2e  gap %.2e  order gap %.2e  two best %s" % (S.case_id(case), got.worst, got.gap, got.order_gap,
                                                                      got.best_two))
  S.record("host", case, got, "%.2e*max(y64,floor)" % S.exact_bar(case.kind))
  assert got.gap >= 4 * S.G, got.gap
  assert not S.two_best_condition(case, got.best_two, S.exact_bar(case.kind)), got.best_two


def test_what_is_exempt_from_the_two_best_condition_misses_it():
  """ENDS_ON_START names (case, rule) pairs of the list, each of which does miss the condition — nothing else is waived."""
  keys = {tuple(c)[:-1]: c for c in S.CASES}
  for key, rule in S.ENDS_ON_START:
    got = study(keys[key])
    assert got.best_two[rule] < 100 * S.exact_bar(key[0]), (key, rule, got.best_two)
    assert S.vector_search(S.Reference(S.inputs_of(keys[key]), key[2]), keys[key], rule)[0] == 0.0


@pytest.mark.parametrize("case", S.DEVICE_CASES, ids=S.case_id)
def test_conditions_of_the_cases_on_device_distances(case):
  """The bar on the device's distances is 2e-5: the two best objectives of those cases differ by 100 of THOSE bars."""
  assert not S.two_best_condition(case, study(case).best_two, S.DEVICE_REL), study(case).best_two


def test_conditions_of_the_long_cases():
  """The two cases that also run at d = 20 011 are other draws there (make_stack draws d numbers per row)."""
  assert len(S.DEVICE_CASES) >= 140 and len(S.LONG_CASES) == 2
  for case in S.LONG_CASES:
    gap, best_two = S.conditions_at(case, S.inputs_of(case, S.D_PASS))
    assert gap >= 4 * S.G and not S.two_best_condition(case, best_two, S.DEVICE_REL), (S.case_id(case), gap, best_two)


@pytest.mark.parametrize("cfg", S.STEP_CASES, ids=lambda c: "%s-n%d-f%d" % (c.gar, c.n, c.f))
def test_conditions_of_the_step_cases(cfg):
  """The rows of tests/test_gpu_search_matrix.py's steps (the workers' momentum buffers after one step are the sampled
  rows times 1 - dampening: gaps and relative differences do not change with the scale)."""
  h, d = cfg.n - cfg.f, S.D_PASS
  rows = torch.stack(O.make_stack("hetero", cfg.n, cfg.f, d, cfg.seed)[0][:h])
  avg = rows.mean(dim=0)
  inputs = S.Inputs(rows, avg, S.direction_of(rows, avg, cfg.attack))
  case = S.Case("hetero", h, cfg.f, cfg.f, None, cfg.attack, cfg.negative, 16, cfg.seed)
  ref = S.Reference(inputs, cfg.f)
  if cfg.gar == "bulyan":
    want_factor, trace = S.bulyan_search(ref, case)
  else:
    want_factor, trace, seen = S.vector_search(ref, case, cfg.gar)
    assert all(c is None or c.gap >= 4 * S.G for c in seen)
  assert S.two_best_differ_by(trace) >= 100 * S.DEVICE_REL, (cfg, S.two_best_differ_by(trace))


def test_cursor_folds_a_negative_probe_only():
  """tools/misc.py:493-494 folds `while x < 0`: a probe that lands on 0 exactly stays there.  The attack's own call
  (start 0, delta 1, ratio 0.8) never lands on it — 0.8 is no dyadic number — so the cursor is driven with parameters
  that do: from 0.3125 with delta 1 and ratio 0.75 on a falling scape the probes are 1.3125, 0.5625 and 0.5625 - 0.5625."""
  scape = lambda x: -x  # noqa: E731
  got, trace = linesearch.line_maximize(scape, evals=8, start=0.3125, delta=1.0, ratio=0.75)
  want, want_trace = O.line_maximize(scape, evals=8, start=0.3125, delta=1.0, ratio=0.75)
  assert [x for x, _ in want_trace][:4] == [0.3125, 1.3125, 0.5625, 0.0]
  assert trace == want_trace and got == want == 0.0


def test_bars_come_from_the_measurement():
  for kind in S.KINDS:
    assert S.exact_bar(kind) == min(1e-6, 16 * S.EXACT_WORST[kind]) and S.exact_bar(kind) <= S.EXACT_BAR_CAP
  assert S.G == 1e-5 and S.DEVICE_REL == 2e-5


# ---------------------------------------------------------------------------------------------------------------------
# The case list

def test_case_list_holds_what_it_must():
  shapes = {(c.h, c.k, c.f, c.m) for c in S.CASES}
  for h, k, f in S.REFERENCE_GRID:
    for m in (None, 1, h + k):
      assert (h, k, f, m) in shapes
    for kind in S.KINDS:
      assert any((c.kind, c.h, c.k, c.f) == (kind, h, k, f) for c in S.CASES), (kind, h)
    for kind in ("hetero", "tight", "momentum"):
      signs = {(c.attack, c.negative) for c in S.CASES if (c.kind, c.h, c.k, c.f, c.m) == (kind, h, k, f, None)}
      assert signs == {(a, s) for a in ("empire", "little") for s in (False, True)}
  for h in S.STRUCTURE_H:
    assert {c.k for c in S.CASES if c.h == h} >= {1, S.BM_MAX_ROWS - h}, h
  hk = {(c.h, c.k) for c in S.CASES}
  assert {(63, 1), (64, 0), (14, 0)} <= hk
  assert {(20, 3, 5), (20, 5, 3)} <= {(c.h, c.k, c.f) for c in S.CASES}
  takes = {S.krum_take(c.h + c.k, c.f) for c in S.CASES}
  assert {0, 1, 7, 8, 9, 16} <= takes
  assert any(S.krum_take(c.h + c.k, c.f) == c.h + c.k - 1 for c in S.CASES)
  assert any(0 < S.krum_take(c.h + c.k, c.f) <= c.k - 1 for c in S.CASES)
  assert {c.evals for c in S.CASES} == set(S.EVALS)
  assert all(c.h + c.k <= S.BM_MAX_ROWS and 1 <= (c.m or S.default_m(c.h, c.k, c.f)) <= c.h + c.k for c in S.CASES)
  assert len(set(S.CASES)) == len(S.CASES)


def test_cases_reach_every_path_of_the_merge():
  reached = set()
  for case in S.CASES:
    reached |= study(case).reach
  assert reached >= set(S.REACH), set(S.REACH) - reached
  # both sides of each boundary in h: where a wave's sorted rows wrap, where the row span grows, where LDS needs the opt-in
  hs = {c.h for c in S.CASES if c.k >= 1}
  for edge in range(S.K_SEARCH_WAVES, S.BM_MAX_ROWS, S.K_SEARCH_WAVES):
    assert {edge, edge + 1} <= hs and -(-edge // S.K_SEARCH_WAVES) + 1 == -(-(edge + 1) // S.K_SEARCH_WAVES)
  assert {8, 9} <= hs and S.row_span(8) == 8 and S.row_span(9) == 16
  assert {48, 49} <= hs and S.search_lds_bytes(48) <= S.LDS_OPT_IN_BYTES < S.search_lds_bytes(49)
  assert 62 in hs and {63, 64} <= {c.h for c in S.CASES}


def test_merge_model_adds_what_the_reference_adds():
  """The stretches of the model, added up, are the float64 scores: b1 of the row's sorted distances, c2 copies of the
  distance to the candidate, c3 more of the row; k - 1 zeros and `rest` sorted dq for the Byzantine row."""
  import numpy as np
  for case in [c for c in S.CASES if c.kind in ("hetero", "duplicates") and c.k >= 1][::5]:
    ref = S.Reference(S.inputs_of(case), case.k)
    take = S.krum_take(case.h + case.k, case.f)
    for t in (0.0, 0.3, 1.1, -2.5, 17.0):
      merge = S.merge_model(ref, t, take, case.m or S.default_m(case.h, case.k, case.f))
      dist, dq = ref.distances(t)
      scores = ref.scores(dist, take)
      for i in range(case.h):
        others = np.sort(np.delete(ref.hh[i], i))
        parts = list(others[:merge.b1[i]]) + [dq[i]] * merge.c2[i] + list(others[merge.b1[i]:merge.b1[i] + merge.c3[i]])
        assert len(parts) == take and math.isclose(sum(parts), scores[i], rel_tol=1e-13, abs_tol=0.0), (case, t, i)
      byz = [0.0] * merge.zeros + list(np.sort(dq)[:merge.rest])
      assert len(byz) == take and math.isclose(sum(byz), scores[case.h], rel_tol=1e-13, abs_tol=0.0), (case, t)


# ---------------------------------------------------------------------------------------------------------------------
# The mirror against the sources

def _constexpr(text, name):
  found = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*([^;]+);", text)
  assert found, name
  return found.group(1).strip()


def test_constants_and_layout_of_the_device_kernel():
  max_rows = int(re.search(r"#define\s+BM_MAX_ROWS\s+(\d+)", HEADER.read_text()).group(1))
  assert max_rows == S.BM_MAX_ROWS
  block = int(_constexpr(DEVICE, "kSearchBlock"))
  env = {"BM_MAX_ROWS": max_rows, "kSearchBlock": block}
  env["kSearchWaves"] = c_eval(_constexpr(DEVICE, "kSearchWaves"), env)
  assert env["kSearchWaves"] == S.K_SEARCH_WAVES
  assert c_eval(_constexpr(DEVICE, "kSortRowsPerWave"), env) == S.K_SORT_ROWS_PER_WAVE
  assert c_eval(_constexpr(DEVICE, "kRankChunk"), env) == S.K_RANK_CHUNK
  assert "const int i = wave + r * kSearchWaves;" in DEVICE  # row i is sorted by wave i % 16
  assert "inline int attack_row_span(int h) { return (h + 7) & ~7; }" in CORE
  assert "inline int search_ld(int h) { return attack_row_span(h) + 1; }" in DEVICE
  lds = re.search(r"inline size_t search_lds_bytes\(int h\) \{\s*return \(size_t\)\((.+?)\) \* sizeof\(double\) \+\s*"
                  r"\(size_t\)(.+?) \* sizeof\(int\);", DEVICE, re.S)
  assert lds
  for h in range(1, max_rows + 1):
    names = dict(env, h=h)
    doubles = c_eval(lds.group(1).replace("search_ld(h)", str(S.search_ld(h))), names)
    ints = c_eval(lds.group(2), names)
    assert doubles * 8 + ints * 4 == S.search_lds_bytes(h), h
  assert "if (dynamic_bytes + static_bytes <= 48u * 1024u) return 0;" in COMMON
  assert DEVICE.count("lds_opt_in(reinterpret_cast<const void*>(kernel), lds, 0)") == 2
  assert S.search_lds_bytes(48) <= S.LDS_OPT_IN_BYTES < S.search_lds_bytes(49)
  assert "for (int q = 0; q < 8; ++q) g[q] = hs[u0 + q];" in DEVICE and "for (int u0 = 0; u0 < most1; u0 += 8)" in DEVICE
  assert "for (int u0 = 0; u0 < most3; u0 += 8)" in DEVICE and S.GROUP == 8


def test_merge_model_is_the_kernels():
  for line in ("const bool right = len > 0 && v < dq;",
               "const int b1 = below < take ? below : take;",
               "const int c2 = (take - b1 < k) ? take - b1 : k;",
               "const int c3 = take - b1 - c2;",
               "const int most1 = longest(b1, take), most3 = longest(c3, take);",
               "if (__builtin_amdgcn_ballot_w64(v >= limit) != 0ull) return limit;",
               "const int zeros = (k - 1 < take) ? k - 1 : take;",
               "const int rest = take - zeros;",
               "int take = take_arg >= 0 ? take_arg : n - f - 1;  // krum.py:59-60",
               "take = take > n - 1 ? n - 1 : take;",
               "take = take < 0 ? 0 : take;",
               "const int kb = __builtin_popcountll(h >= 64 ? 0ull : (selected >> h));",
               "selected = __builtin_amdgcn_ballot_w64(lane < n && rank < m);"):
    assert line in DEVICE, line
  assert "const int take = mode == BM_RANK_KRUM ? n - f - 1 : m;" in DEVICE
  # the host form's counts
  assert "rank_order(sq, n, n - f - 1, order);" in HOST and "rank_order(sq, n, mode == BM_RANK_KRUM ? n - f - 1 : m, order);" in HOST
  assert "take = std::max(0, std::min(take, n - 1));" in HOST and "if (m <= 0) m = n - f - 2;" in HOST


def test_trace_room_and_trace_switch_use_one_predicate():
  """The kernel writes its phase clocks behind the results when BM_SEARCH_TRACE starts with '1'; the caller must make
  room on the same predicate (a value such as "10" once made the kernel write behind the buffer)."""
  assert "const bool trace = trace_env != nullptr && trace_env[0] == '1';" in DEVICE
  assert 'extra = 24 * evals if os.environ.get("BM_SEARCH_TRACE", "")[:1] == "1" else 0' in STATS
  assert int(_constexpr(DEVICE, "kTraceSlots")) * 2 == 24


def test_reference_is_vectorised():
  """A case at n = 64, d = 2 003: the reference's set-up and a sixteen-evaluation search in well under a second."""
  import time
  case = next(c for c in S.CASES if (c.h, c.k) == (33, 31))
  inputs = S.inputs_of(case)
  S.Reference(inputs, case.k)  # (first use of the thread pool)
  start = time.perf_counter()
  S.vector_search(S.Reference(inputs, case.k), case, "krum")
  assert time.perf_counter() - start < 5.0  # (0.05 s on an idle machine: a loop over pairs in Python takes minutes)
