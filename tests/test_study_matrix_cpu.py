"""The mirror of tests/study_matrix.py against the sources, its case lists against every instance the sources can
instantiate, the structure its derived lengths were chosen for, the sensitivity of its inputs and its expected values
against what the project already trusts (no GPU needed).

Parsed out of csrc/study.hip, reduce.hip, launch_plan.h, bm_common.h, api.cpp and include/bm_gar.h: the block sizes and grid caps, the
fold of the plain form, U and the staged iterations of the burst form, the burst condition and its knob, the pointers
the entry point drops, the order of its Alignment, the tiers and the narrowing of dispatch_stack_stats, and every
instantiation of the three kernels.  An instance added to the sources without a case that runs it fails here."""

import itertools
import re

import pytest
import torch

from tests import first_pass_matrix as F
from tests import study_matrix as S
from tests.sharded_backend import OracleBackend
from tests.test_instance_matrix_cpu import HEADER, _function, _read, c_eval

STUDY = _read("study.hip")
REDUCE = _read("reduce.hip")
PLAN = _read("launch_plan.h")
COMMON = _read("bm_common.h")
CUS = (256, 304, 64)


def _int(text, name):
  m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*([^;]+);", text)
  assert m, name
  return c_eval(m.group(1), {})


def _squash(text):
  return re.sub(r"\s+", " ", text)


# ---------------------------------------------------------------------------------------------------------------------
# The mirror against the sources

def test_constants():
  assert _int(STUDY, "kStudyBlock") == S.K_STUDY_BLOCK
  assert _int(STUDY, "kStudyMaxBlocks") == S.K_STUDY_MAX_BLOCKS
  assert _int(STUDY, "kStudyBurstThreads") == S.K_STUDY_BURST_THREADS
  assert _int(STUDY, "kStudySlotBudget") == S.K_STUDY_SLOT_BUDGET
  assert _int(REDUCE, "kRedBlock") == S.K_RED_BLOCK
  assert _int(REDUCE, "kMaxPartialBlocks") == S.K_MAX_PARTIAL_BLOCKS
  assert "constexpr Caps kStudyCaps = caps_of(kStudyMaxBlocks);" in STUDY and S.STUDY_CAPS == (2048, 2048)
  assert "constexpr Caps kStatsCaps{kMaxPartialBlocks - 1, kMaxPartialBlocks};" in REDUCE and S.STATS_CAPS == (2047, 2048)
  assert "constexpr Caps caps_of(int both) { return Caps{both, both}; }" in PLAN
  header = HEADER.read_text()
  assert int(re.search(r"#define\s+BM_MAX_ROWS\s+(\d+)", header).group(1)) == S.BM_MAX_ROWS
  assert int(re.search(r"#define\s+BM_STUDY_SLOTS\s+(\d+)", header).group(1)) == S.STUDY_SLOTS
  assert int(re.search(r'env_int\("BM_STUDY_BURST", (\d+)\)', _read("api.cpp")).group(1)) == S.DEFAULT_KNOBS["BM_STUDY_BURST"]
  assert "int study_burst;     // BM_STUDY_BURST: iterations per CU from which bm_study_stats takes its burst form" in COMMON
  # the Byzantine vector of the stack statistics: `empire` two fp32 operations, BM_ATTACK_DIRECTION the product alone
  assert "const float dir = ((attack_kind & 15) == BM_ATTACK_LITTLE) ? __builtin_sqrtf(q / (fk - 1.0f)) : -avg;" in COMMON
  assert "return (attack_kind & BM_ATTACK_DIRECTION) ? att : avg + att;" in COMMON
  # the fold of the plain form
  assert f"if (++since == {S.K_STUDY_FOLD}) {{" in STUDY
  assert "const int64_t stride = (int64_t)gridDim.x * kStudyBlock;" in STUDY


def test_burst_shape_and_condition():
  assert "constexpr int kStudySlots = MOM ? kStudySlotBudget / 2 : kStudySlotBudget;" in STUDY
  assert "constexpr int U = ((L2 && CM >= 2) || MOM) ? 1 : 2;" in STUDY
  for cm, l2, mom in itertools.product((1, 2, 3), (False, True), (False, True)):
    u = c_eval("((L2 && CM >= 2) || MOM) ? 1 : 2", {"L2": l2, "CM": cm, "MOM": mom})
    slots = c_eval("MOM ? kStudySlotBudget / 2 : kStudySlotBudget", {"MOM": mom, "kStudySlotBudget": S.K_STUDY_SLOT_BUDGET})
    assert S.burst_shape(cm, l2, mom) == (u, slots)
  assert {S.burst_shape(cm, l2, mom) for cm, l2, mom in itertools.product((1, 2, 3), (False, True), (False, True))} == \
      set(S.BURST_CLASSES)
  for cls, (f, cm, l2, mom) in S.CLASS_INSTANCE.items():
    assert S.burst_shape(cm, l2, mom) == cls
  text = _squash(STUDY)
  assert ("if (threshold <= 0 || cm < 1 || vec != 4 || a.a_out != nullptr || nvec >= ((int64_t)1 << 30)) return false; "
          "return nvec >= (int64_t)threshold * compute_units() * kStudyBurstThreads;") in text
  assert "const int threshold = tuning().study_burst;" in text
  assert "sp.grid = compute_units();" in text and "if (sp.grid > kStudyMaxBlocks) sp.grid = kStudyMaxBlocks;" in text
  assert "const uint32_t span = gridDim.x * kStudyBurstThreads;" in text
  assert "const uint32_t iters = (nvec + span - 1) / span;" in text
  assert "const uint32_t p1 = (p0 + kStudySlots < iters) ? p0 + kStudySlots : iters;" in text
  assert "live[u] = (it + u) < p1 && v < nvec;" in text
  base = S._case("x", cm=1, d=4 * 256 * 1024)
  one = base._replace(knobs=S.BURST_ONLY)
  assert S.study_burst_eligible(one, 4, 256 * 1024, 256) and not S.study_burst_eligible(one, 4, 256 * 1024 - 1, 256)
  assert not S.study_burst_eligible(one, 2, 1 << 24, 256) and not S.study_burst_eligible(one._replace(cm=0), 4, 1 << 24, 256)
  assert not S.study_burst_eligible(one._replace(f=3, a_out=True), 4, 1 << 24, 256)
  assert S.study_burst_eligible(one._replace(f=0, a_out=True), 4, 1 << 24, 256)  # (the entry dropped the output)
  assert S.study_burst_eligible(base, 4, 8 * 256 * 1024, 256) and not S.study_burst_eligible(base, 4, 8 * 256 * 1024 - 1, 256)
  assert not S.study_burst_eligible(base._replace(knobs=(("BM_STUDY_BURST", 0),)), 4, 1 << 28, 256)


def test_pointers_the_entry_drops_and_its_alignment():
  text = _squash(STUDY)
  assert "const bool att = f_real > 0, l2 = params != nullptr && origin != nullptr;" in text
  assert ("StudyArgs a{sampled_avg, honest_avg, defense, att ? byz : nullptr, curv_mode >= 2 ? past_newest : nullptr, "
          "curv_mode == 3 ? past_oldest : nullptr, l2 ? params : nullptr, l2 ? origin : nullptr, "
          "curv_mode >= 1 ? curv : nullptr, att ? attack_avg_out : nullptr, update_momentum, momentum_mu, "
          "one_minus_damp};") in text
  order = re.search(r"const int vec = Alignment\(\)((?:\s*\.of\(a\.\w+\))+)\s*\.vec\(\);", STUDY).group(1)
  assert tuple(re.findall(r"a\.(\w+)", order)) == S.ROLES
  assert "for_body_and_tail<4>(Tail::kOwnLaunch, vec, d, kStudyBlock, kStudyCaps," in text
  assert "partial + sp.part, s);" in text
  assert "int vec() const { return (bits_ & 15u) == 0 ? 4 : ((bits_ & 7u) == 0 ? 2 : 1); }" in PLAN
  full = S._case("x", **S.FULL)
  assert S.live_roles(full) == list(S.ROLES) and S.study_vec(full) == 4
  for role in S.ROLES:
    assert S.study_vec(full._replace(mis=(role, 4))) == 1 and S.study_vec(full._replace(mis=(role, 8))) == 2
  # a dropped pointer does not narrow the call
  assert S.study_vec(full._replace(f=0, mis=("byz", 4))) == 4 and S.study_vec(full._replace(f=0, mis=("a_out", 4))) == 4
  assert S.study_vec(full._replace(cm=0, mis=("curv", 4))) == 4 and S.study_vec(full._replace(cm=1, mis=("past", 8))) == 4
  assert S.study_vec(full._replace(cm=2, mis=("oldest", 4))) == 4 and S.study_vec(full._replace(l2=False, mis=("origin", 4))) == 4
  for arg in ("a_out_f0", "byz_f0", "curv_mode0"):
    c = [c for c in S.cases("args") if c.arg == arg][0]
    assert set(S.given_roles(c)) - set(S.live_roles(c)) == {{"a_out_f0": "a_out", "byz_f0": "byz", "curv_mode0": "curv"}[arg]}


def test_the_cut():
  text = _squash(PLAN)
  assert "if (mode == Tail::kOwnLaunch && d / vec == 0) vec = 1;" in text
  assert "Span span{0, nvec, body + rides, rides, stream_grid(nvec, block, caps.body), parts};" in text
  assert "Span span{body, rest, d, 0, body == 0 ? stream_grid(rest, block, caps.tail) : 1, parts};" in text
  assert "parts += span.grid;" in text
  assert S.cut(4, 0, 256, S.STUDY_CAPS) == [] and S.cut(4, 3, 256, S.STUDY_CAPS) == [(1, 0, 3, 1)]
  assert S.cut(4, S.D_SHORT, 256, S.STUDY_CAPS) == [(4, 0, 293, 2), (1, 1172, 3, 1)]
  assert S.cut(2, 1027, 256, S.STUDY_CAPS) == [(2, 0, 513, 3), (1, 1026, 1, 1)]
  assert S.cut(1, 1 << 24, 256, S.STUDY_CAPS) == [(1, 0, 1 << 24, 2048)]
  assert S.cut(4, 1 << 24, 256, S.STATS_CAPS)[0][3] == 2047 and S.cut(1, 1 << 24, 256, S.STATS_CAPS)[0][3] == 2048
  assert S.cut(4, 3, 256, S.STATS_CAPS) == [(1, 0, 3, 1)]


def test_stack_dispatch():
  body = _function(REDUCE, "dispatch_stack_stats")
  tiers = [(int(a), int(b)) for a, b in re.findall(r"if \(k <= (\d+)\) return launch_stack_stats<(\d+), VEC>", body)]
  assert [a for a, _ in tiers] == [b for _, b in tiers] == list(S.STACK_TIERS)
  text = _squash(body)
  assert ("if (k <= 32) return launch_stack_stats<32, (VEC > 2 ? 2 : VEC)>(tab, k, nvec * (VEC > 2 ? VEC / 2 : 1), avg, "
          "scaled,") in text
  assert "return launch_stack_stats<64, 1>(tab, k, nvec * VEC, avg, scaled, scale, kind, partial, grid, s);" in text
  assert "const int vec = Alignment().of(rows, k).of(avg_out).of(scaled_out).vec();" in REDUCE
  assert "for_body_and_tail<4>(Tail::kOwnLaunch, vec, d, kRedBlock, kStatsCaps," in REDUCE
  for k, vec in itertools.product(range(1, 65), (4, 2, 1)):
    kmax, v, n = S.dispatch_stack_stats(k, vec, 100)
    assert kmax >= k and v * n == vec * 100
    assert (kmax, v) == ((8 if k <= 8 else 16 if k <= 16 else 24, vec) if k <= 24 else (32, min(vec, 2)) if k <= 32 else (64, 1))


def _launched(text, kernel):
  return re.findall(r"hipLaunchKernelGGL\(\(?" + kernel + r"<([^>]+)>", text)


def test_source_instances():
  """The instantiations the sources hold: study_stats_kernel through launch_study / _cm / _vec, the burst kernel
  through launch_study_burst / _mom, stack_stats_kernel through dispatch_stack_stats at the three widths."""
  assert _launched(STUDY, "study_stats_kernel") == ["ATT, CM, L2, 4", "ATT, CM, L2, 2", "ATT, CM, L2, 1"]
  cm = _function(STUDY, "launch_study_cm")
  assert re.findall(r"launch_study_vec<ATT, (\d), L2>", cm) == ["0", "1", "2", "3"]
  assert sorted(re.findall(r"launch_study_cm<(\w+), (\w+)>", _function(STUDY, "launch_study"))) == \
      sorted((a, b) for a in ("true", "false") for b in ("true", "false"))
  assert _launched(STUDY, "study_stats_burst_kernel") == ["ATT, 1, L2, MOM", "ATT, 2, L2, MOM", "ATT, 3, L2, MOM"]
  assert re.findall(r"launch_study_burst_mom<ATT, L2, (\w+)>", _function(STUDY, "launch_study_burst")) == ["true", "false"]
  assert sorted(re.findall(r"launch_study_burst<(\w+), (\w+)>", _function(STUDY, "bm_study_stats_update"))) == \
      sorted((a, b) for a in ("true", "false") for b in ("true", "false"))
  assert _launched(REDUCE, "stack_stats_kernel") == ["KMAX, VEC"]
  want = S.source_instances()
  assert len([i for i in want if i[0] == "study"]) == 48 and len([i for i in want if i[0] == "study_burst"]) == 24
  assert len([i for i in want if i[0] == "stack"]) == 12 and len(want) == 84
  stack = {S.dispatch_stack_stats(k, vec, 1)[:2] for k in range(1, 65) for vec in (4, 2, 1)}
  assert {("stack",) + i for i in stack} == {i for i in want if i[0] == "stack"}


# ---------------------------------------------------------------------------------------------------------------------
# The case lists against the instances

def test_case_lists_reach_every_instance():
  want = S.source_instances()
  for cus in CUS:
    reached = {g: set() for g in S.GROUPS}
    for g in S.GROUPS:
      for c in S.cases(g, cus):
        reached[g] |= S.instances(c, cus)[0]
    union = set().union(*reached.values())
    assert union == want, (cus, sorted(want - union, key=str), sorted(union - want, key=str))
    assert {i for i in reached["plain"]} == {i for i in want if i[0] == "study"}
    assert {i for i in reached["knob_burst"] if i[0] == "study_burst"} == {i for i in want if i[0] == "study_burst"}
    assert reached["stack"] == {i for i in want if i[0] == "stack"}
  print(f"{len(want)} source instances, all reached by a case")
  # the 48 plain instances with the momentum stream on and off, the attack average on and off where there is an attack
  seen = {}
  for c in S.cases("plain"):
    for i in S.instances(c)[0]:
      seen.setdefault(i, set()).add((c.mom, c.a_out))
  for i in (i for i in want if i[0] == "study"):
    assert {m for m, _ in seen[i]} == {False, True}, i
    assert {a for _, a in seen[i]} == ({False, True} if i[1] else {False}), i
  # every tier edge of the stack, every output combination, every attack with and without the direction flag
  stack = S.cases("stack")
  assert {c.f for c in stack} >= {1, 8, 9, 16, 17, 24, 25, 32, 33, 64}
  for k in (1, 8, 9, 16, 17, 24, 25, 32, 33, 64):
    mine = [c for c in stack if c.f == k]
    assert {(c.avg, c.scaled) for c in mine} == set(itertools.product((False, True), repeat=2))
    assert {(c.attack, c.direction) for c in mine if c.scaled} >= ({("empire", False), ("empire", True)} if k == 1 else
                                                                   set(itertools.product(("empire", "little"), (False, True))))
    assert {(c.offset, c.d) for c in mine} >= set(itertools.product(S.STACK_OFFSETS, S.D_STACK[1:]))
  # the narrowed widths together with a tail launch
  for k, inst in ((25, ("stack", 32, 2)), (32, ("stack", 32, 2)), (33, ("stack", 64, 1)), (64, ("stack", 64, 1))):
    assert any(c.f == k and c.offset == 0 and len(S.instances(c)[1]) == 2 and S.instances(c)[1][0].inst == inst and
               S.instances(c)[1][0].count * S.instances(c)[1][0].vec == c.d // 4 * 4 for c in stack), k


def test_parts_cover_their_groups():
  for group in S.GROUPS:
    whole = S.cases(group)
    keys = [S.case_key(c) for c in whole]
    assert len(keys) == len(set(keys)), group
    if group in S.PARTS:
      split = [c for p in S.PARTS[group] for c in S.cases(group, 256, p)]
      assert sorted(keys) == sorted(map(S.case_key, split)), group


@pytest.mark.parametrize("cus", CUS)
def test_derived_lengths_have_the_structure_they_were_chosen_for(cus):
  span = S.span_of(cus)
  # plain_long: the fold, the grid cap and one workgroup more, nparts 2048 / 64 / 65
  fold, cap, p2048, p64, p65 = S.cases("plain_long", cus)
  inst, launches, nparts = S.instances(fold, cus)
  assert inst == {("study", True, 2, False, 1)} and len(launches) == 1 and launches[0].grid == S.K_STUDY_MAX_BLOCKS
  assert S.plain_iterations(launches[0].count, launches[0].grid) == S.K_STUDY_FOLD + 1
  assert S.plain_iterations(launches[0].count - 1, launches[0].grid) == S.K_STUDY_FOLD  # the smallest such d
  inst, launches, nparts = S.instances(cap, cus)
  assert nparts == 2049 and cap.d % 4 == 3 and [l.vec for l in launches] == [4, 1]
  assert launches[0].grid == 2048 and launches[0].count == 2049 * 256 and launches[1].part == 2048
  assert [S.instances(c, cus)[2] for c in (p2048, p64, p65)] == [2048, 64, 65]
  assert all(l.form == "plain" for c in (fold, cap, p2048, p64, p65) for l in S.instances(c, cus)[1])
  assert S.instances(S.cases("args")[0], cus)[2] == 3 and S.instances([c for c in S.cases("args") if c.arg == "d0"][0], cus)[2] == 0
  assert S.instances(S._case("x", d=1024), cus)[2] == 1
  # knob_burst
  todo = S.cases("knob_burst", cus)
  for c in S.cases("knob_burst", cus, 0) + S.cases("knob_burst", cus, 1):  # two iterations, the second partly live, a tail of 3
    inst, launches, nparts = S.instances(c, cus)
    body, tail = launches
    assert body.form == "burst" and body.grid == min(cus, 2048) and S.burst_iterations(body.count, cus) == 2
    assert 0 < body.count - span < span and (body.count - span) % S.K_STUDY_BURST_THREADS != 0
    assert tail.vec == 1 and tail.count == 3 and tail.part == body.grid and nparts == body.grid + 1
    plain = S.instances(c._replace(knobs=()), cus)[1]
    assert all(l.form == "plain" for l in plain)  # the parent's digests are the plain form's
  classes = S.cases("knob_burst", cus, 2)
  for i, cls in enumerate(S.BURST_CLASSES):
    one, three = classes[2 * i], classes[2 * i + 1]
    assert S.burst_shape(one.cm, one.l2, one.mom) == cls
    b1, b3 = S.instances(one, cus)[1][0], S.instances(three, cus)[1][0]
    assert b1.form == b3.form == "burst" and b1.count == span and S.burst_iterations(b1.count, cus) == 1
    assert S.burst_iterations(b3.count, cus) == 3 and b3.count % span != 0 and three.d % 4 == 2
    # an odd number of iterations inside one burst: with U = 2 the second group of the last step is not live
    assert 3 < cls[1]
    past = S.cases("knob_burst", cus, 3 + i)[0]
    bp = S.instances(past, cus)[1][0]
    assert S.burst_shape(past.cm, past.l2, past.mom) == cls and bp.form == "burst"
    assert S.burst_iterations(bp.count, cus) == cls[1] + 1 and bp.count % span != 0 and len(S.instances(past, cus)[1]) == 2
    e = S.edges(past, cus)
    assert cls[1] * span * 4 - 1 in e and cls[1] * span * 4 in e  # either side of the burst boundary
  misc = S.cases("knob_burst", cus, 6)
  assert all(l.form == "plain" for l in S.instances(misc[0], cus)[1]) and misc[0].a_out  # an output: the plain form
  for c in misc[1:]:
    body = S.instances(c, cus)[1][0]
    assert body.form == "burst" and c.bad is not None
    col = S.bad_column(c, c.bad[2], cus)
    assert col // 4 >= span and col // 4 < body.count  # in the last, partly live iteration
    if c.bad[2] == "lane1023":
      assert (col // 4) % S.K_STUDY_BURST_THREADS == 1023
  # every long case: at most MAX_EDGES edge coordinates, inside the vector
  for c in S.all_cases(cus):
    e = S.edges(c, cus)
    assert len(e) <= S.MAX_EDGES and all(0 <= x < c.d for x in e), c
    assert c.spiked == (c.d >= S.LONG)
  # the stack's cap: 2047 workgroups, one vector more than they hold in one trip, and a tail
  capped = [c for c in S.cases("stack", cus) if c.d >= S.LONG]
  assert len(capped) == 1
  body, tail = S.instances(capped[0], cus)[1]
  assert body.grid == 2047 and body.count == 2047 * 256 + 1 and tail.count == 3 and tail.part == 2047


def test_the_largest_spike_rotates():
  tops = set()
  for c in S.cases("knob_burst", 256, 0):
    v = S.values(c, 256)
    tops.add(int(v["def"].abs().argmax()))
    assert int(v["def"].abs().argmax()) in S.edges(c, 256)
  assert len(tops) >= 6, tops


# ---------------------------------------------------------------------------------------------------------------------
# Sensitivity

def test_every_edge_coordinate_counts():
  """For every case of the lists (256 compute units) and every non-zero sum slot: dropping or doubling one edge
  coordinate moves the float64 expected value by at least ten of the slot's bars.  Exempt: slot 19 (the deviation of
  the attack copies from their mean) at long cases only, where a power-of-two spike has deviation 0."""
  exempt = []
  for c in S.all_cases(256):
    for slot, col in S.insensitive(c, 256):
      assert c.kernel != "stack", (S.case_key(c), slot, col)
      assert slot == 19 and c.spiked, (S.case_key(c), slot, col)  # no Gram, dot or l2 slot, and no short case
      exempt.append((S.case_key(c), slot))
  for key, slot in sorted(set(exempt)):
    print(f"exempt: slot {slot} of {key}")
  short = [c for c in S.all_cases(256) if c.kernel != "stack" and not c.spiked and c.f >= 3 and c.d >= 4 and c.bad is None]
  assert len(short) > 50
  for c in short:  # slot 19 is a non-zero slot there, and sensitive (see above)
    terms = {slot: t for slot, t, _ in S.study_terms(c, S.values(c, 256))}
    assert float(terms[19].sum()) > 0, S.case_key(c)


def test_the_maxima_sit_on_edge_coordinates_of_long_cases():
  for c in S.all_cases(256):
    if c.spiked and c.kernel != "stack" and c.bad is None:
      v = S.values(c, 256)
      e = S.edges(c, 256)
      assert int(v["def"].abs().argmax()) in e and (c.f == 0 or int(v["byz"].abs().argmax()) in e)


# ---------------------------------------------------------------------------------------------------------------------
# The expected values against what the project already trusts

def _short_study_cases():
  return [c for c in S.all_cases(256) if c.kernel == "study" and c.d <= S.SHORT_FULL]


def test_expected_slots_are_the_restatements():
  """tests/sharded_backend.py restates bm_study_stats_update on the CPU: same slots (float64), C and M within the
  rounding of its two-operation forms, the attack average bit for bit."""
  backend = OracleBackend()
  checked = 0
  for c in _short_study_cases():
    if c.bad is not None or c.arg == "curv_nan_mode1" or c.d == 0:
      continue
    v = S.values(c, 256)
    e = S.study_expected(c, v)
    w = {r: t.clone() for r, t in v.items()}
    a_out = torch.zeros(c.d) if c.f > 0 else None
    out = backend.study_stats(w["s"], w["h"], w["def"], w.get("byz") if c.f > 0 else None, c.f,
                              past_newest=w.get("past"), curv=w.get("curv") if c.cm >= 1 else None,
                              past_oldest=w.get("oldest"), curv_mode=c.cm, mu=S.MU, oldest_weight=S.W_OLDEST,
                              params=w.get("params"), origin=w.get("origin"), attack_avg_out=a_out,
                              update_momentum=w.get("mom"), update_mu=S.MOM_MU, update_omd=S.MOM_OMD).tolist()
    for slot in range(S.STUDY_SLOTS):
      assert abs(out[slot] - e.out[slot]) <= 1e-12 * abs(e.out[slot]), (S.case_key(c), slot, out[slot], e.out[slot])
    if c.f > 0:
      assert not bool(F.bits_differ(a_out, e.a).any())
    if c.cm >= 1:
      assert float((w["curv"] - e.curv).abs().max()) <= 2e-7 * float(e.curv.abs().max()), S.case_key(c)
    if c.mom:
      assert float((w["mom"] - e.mom).abs().max()) <= 2e-7 * float(e.mom.abs().max()), S.case_key(c)
    checked += 1
  assert checked > 150


def test_expected_stack_values_are_the_oracles():
  from oracle import gar_oracle as O
  checked = 0
  for c in S.cases("stack"):
    if c.d not in (3, 1027) or c.bad is not None:
      continue
    rows = S.stack_values(c)
    want, _, _, wmax = O.compute_avg_dev_max(list(rows))
    avg = F.seq_avg(rows)
    assert not bool(F.bits_differ(avg, want).any()) and F.abs_max(avg) == wmax
    terms = {slot: float(t.sum()) for slot, t, _ in S.stack_terms(c, rows)}
    n2, dev = F.sums64(rows, avg)
    assert abs(terms[0] - n2) <= 1e-12 * n2 and abs(terms[1] - dev) <= 1e-12 * dev + 1e-300
    checked += 1
  assert checked > 100


def test_midpoint_counts_are_within_the_cap():
  """The two emulated fmas (the leading one of mode 3, the momentum) of every study case up to 2^22 coordinates: at most
  MIDPOINT_CAP of the elements are fp32 midpoints of the float64 sum.  Longer cases are counted where they run."""
  total = elements = 0
  for c in S.all_cases(256):
    if c.kernel != "stack" and c.d <= (1 << 22) and (c.cm == 3 or c.mom):
      n, el = S.midpoints(c, 256)
      assert n <= S.MIDPOINT_CAP * el, (S.case_key(c), n, el)
      total, elements = total + n, elements + el
  print(f"midpoint elements: {total} of {elements}")


def test_neighbours_of_a_float():
  t = torch.tensor([1.0, -1.0, 0.0, 2.0 ** -126], dtype=torch.float32)
  up, down = S.next_up_down(t)
  assert up.tolist() == [1.0 + 2.0 ** -23, -1.0 + 2.0 ** -24, 2.0 ** -149, 2.0 ** -126 + 2.0 ** -149]
  assert down.tolist() == [1.0 - 2.0 ** -24, -1.0 - 2.0 ** -23, -(2.0 ** -149), 2.0 ** -126 - 2.0 ** -149]
