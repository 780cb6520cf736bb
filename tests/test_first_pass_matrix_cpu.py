"""The first-pass mirror of tests/first_pass_matrix.py against the sources, its case lists against every instance the
sources can instantiate, and its expected values against what the project already trusts (no GPU needed).

Parsed out of csrc/step.hip, launch_plan.h, api.cpp and include/bm_gar.h: the block sizes and the grid cap, the tiers of
dispatch_momentum_stats, fused_rule_shape / nomom_shape / shape_ok, the burst condition, the fused conditions of the
five entry points and the body / tail cut.  An instance added to the sources without a case that runs it fails here."""

import math
import re
from fractions import Fraction

import pytest
import torch

from oracle import gar_oracle as O
from tests import first_pass_matrix as F
from tests import instance_matrix as M
from tests.test_instance_matrix_cpu import CSRC, HEADER, _function, _read, c_eval

STEP = _read("step.hip")
PLAN = _read("launch_plan.h")


def _int(text, name):
  m = re.search(r"constexpr\s+(?:int|int64_t)\s+" + name + r"\s*=\s*([^;]+);", text)
  assert m, name
  return c_eval(m.group(1).replace("(int64_t)", ""), {}) if "<<" not in m.group(1) else m.group(1)


def _squash(text):
  return re.sub(r"\s+", " ", text)


# ---------------------------------------------------------------------------------------------------------------------
# The mirror against the sources

def test_constants():
  assert _int(STEP, "kStepBlock") == F.K_STEP_BLOCK
  assert _int(STEP, "kStepBurstBlock") == F.K_STEP_BURST_BLOCK
  assert _int(STEP, "kStepPieceCap") == F.K_STEP_PIECE_CAP
  assert re.search(r"constexpr int64_t kMaxColsPerLaunch = \(int64_t\)1 << 29;", PLAN) and F.K_MAX_COLS_PER_LAUNCH == 1 << 29
  assert int(re.search(r"#define\s+BM_MAX_ROWS\s+(\d+)", HEADER.read_text()).group(1)) == F.BM_MAX_ROWS
  api = _read("api.cpp")
  for knob, value in F.DEFAULT_KNOBS.items():
    assert int(re.search(r'env_int\("' + knob + r'", (\d+)\)', api).group(1)) == value, knob
  assert F.RULES == M.RULES


def test_dispatch_tiers():
  body = _function(STEP, "dispatch_momentum_stats")
  assert "if (tuning().step_stream != 1) {" in body
  reg = [(int(a), int(b)) for a, b in re.findall(r"if \(t <= (\d+)\) return launch_momentum_stats<(\d+), VEC>", body)]
  assert [a for a, _ in reg] == [b for _, b in reg] == list(F.REGISTER_TIERS)
  exact = re.findall(r"if \(ks == (\d+) && h == (\d+)\) return launch_momentum_stats<(\d+), VEC>", body)
  assert [tuple(map(int, e)) for e in exact] == [(t, t, t) for t in F.EXACT_TIERS]
  stream = re.findall(r"if \(t <= (\d+)\) return launch_momentum_stats_stream<(\d+), VEC>", body)
  last = re.search(r"return launch_momentum_stats_stream<(\d+), VEC>\(a\);\n}", body).group(1)
  assert [int(b) for _, b in stream] + [int(last)] == list(F.STREAM_TIERS) and all(a == b for a, b in stream)
  assert int(last) == F.BM_MAX_ROWS
  # row predicates only up to T = 12: above, EXACT alone is instantiated
  launch = _function(STEP, "launch_momentum_stats")
  assert "if constexpr (T > 12) {" in launch and "if (!exact) return BM_EINVAL;" in launch
  assert max(F.REGISTER_TIERS) == 12 and min(F.EXACT_TIERS) > 12
  assert "const bool exact = (a.ks == T && a.h == T);" in launch


def test_burst_condition():
  ready = _function(STEP.replace("static bool burst_ready", "static int burst_ready"), "burst_ready")
  assert "return tuning().step_burst > 0 && nvec / ((int64_t)cus * kStepBurstBlock) >= tuning().step_burst;" in ready
  form = _function(STEP, "launch_momentum_stats_form")
  assert "if (burst_ready(a.nvec, cus) && cus < *a.grid_io) {" in form
  knobs = dict(F.DEFAULT_KNOBS, BM_STEP_BURST=1)
  assert F.burst_form(256 * 512, 512, 256, knobs) and not F.burst_form(256 * 512 - 1, 512, 256, knobs)
  assert not F.burst_form(256 * 512, 256, 256, knobs)                    # the plain grid is no larger than the CUs
  assert not F.burst_form(1 << 28, 2047, 256, dict(knobs, BM_STEP_BURST=0))


def _shape_set(expr, names, ranges):
  out = set()
  for a in ranges[0]:
    for b in ranges[1]:
      if c_eval(expr, dict(zip(names, (a, b)))):
        out.add((a, b))
  return out


def test_fused_shapes():
  rows, copies = range(1, 65), range(0, 64)
  expr = re.search(r"static bool fused_rule_shape\(int h, int nb\) \{ return ([^;]+); \}", STEP).group(1)
  assert _shape_set(expr, ("h", "nb"), (rows, copies)) == set(F.FUSED_RULE_SHAPES)
  expr = re.search(r"static bool nomom_shape\(int k, int nb\) \{ return ([^;]+); \}", STEP).group(1)
  assert _shape_set(expr, ("k", "nb"), (rows, copies)) == set(F.NOMOM_SHAPES)
  expr = re.search(r"const bool shape_ok = ks == h && \((.+)\);\s*//", STEP).group(1)
  # n_byz >= 1 is checked by the entry point before
  assert "n_byz < 1" in _function(STEP, "bm_momentum_stats_sqdist")
  assert {s for s in _shape_set(expr, ("h", "n_byz"), (rows, copies)) if s[1] >= 1} == set(F.SQDIST_SHAPES)
  # the rule fusion: 1..6 copies is true of the distance fusion only
  assert set(F.FUSED_RULE_SHAPES) == {(20, 5), (14, 11)} and (20, 1) in F.SQDIST_SHAPES and (20, 6) in F.NOMOM_SHAPES
  cases = re.search(r"BM_FUSED_CASE\((\d+), (\d+)\) BM_FUSED_CASE\((\d+), (\d+)\)\n#undef", STEP).groups()
  assert {(int(cases[0]), int(cases[1])), (int(cases[2]), int(cases[3]))} == set(F.FUSED_RULE_SHAPES)


def test_fused_conditions_of_the_entry_points():
  text = _squash(STEP)
  assert ("return is_column_rule(op) && tuning().step_stream != 1 && ks == h && fused_rule_shape(h, nb);") in text
  assert ("const bool fused = fused_rule_shape(k, n_byz) && vec == 4 && d % 4 == 0 && d > 0 && d <= kMaxColsPerLaunch && "
          "tuning().step_stream != 1;") in text
  assert ("const bool fused = shape_ok && vec == 4 && honest_avg != nullptr && d <= kMaxColsPerLaunch && "
          "tuning().step_stream != 1 && tuning().pair_mode == 0 && tuning().pair_planes != 3 && burst_ready(d / 4, cus);") in text
  assert ("const bool fused = nomom_shape(k, n_byz) && vec == 4 && d % 4 == 0 && d <= kMaxColsPerLaunch && "
          "tuning().step_stream != 1 && tuning().pair_mode == 0 && tuning().pair_planes != 3 && burst_ready(d / 4, cus);") in text
  # all five cut their pass the same way
  assert len(re.findall(r"for_body_and_tail<4>\(Tail::kOwnLaunch, vec, (?:d|dp), kStepBlock, caps_of\((?:cap|kStepPieceCap)\)",
                        text)) == 4  # (bm_momentum_stats and _colwise share momentum_stats_impl)
  # the rule rides in the 16-byte body only; the scalar tail of the fused distance pass adds tail_gram_kernel
  assert "if constexpr (VEC == 4) { if (fusable) {" in text
  assert "return launch_momentum_stats_form<T, 4, true, CLIP, RULE, NB, NOMOM>(a);" in text


def test_alignment_and_cut():
  assert "int vec() const { return (bits_ & 15u) == 0 ? 4 : ((bits_ & 7u) == 0 ? 2 : 1); }" in PLAN
  assert [M.vec_width([o]) for o in (0, 4, 8, 12)] == [4, 1, 2, 1] and M.vec_width(M.row_offsets("mixed", 3)) == 1
  text = _squash(PLAN)
  assert "if (mode == Tail::kOwnLaunch && d / vec == 0) vec = 1;" in text
  assert "if (d > 0 && (vec > 1 || mode != Tail::kOwnLaunch)) {" in text
  assert "Span span{body, rest, d, 0, body == 0 ? stream_grid(rest, block, caps.tail) : 1, parts};" in text
  assert "int64_t g = (work_items + block - 1) / block; if (g < 1) g = 1; if (g > max_blocks) g = max_blocks;" in text
  assert F.plan(4, 0) == [] and F.plan(4, 3) == [(1, 3, 1)] and F.plan(4, 4) == [(4, 1, 1)]
  assert F.plan(4, 1027) == [(4, 256, 1), (1, 3, 1)] and F.plan(2, 1027) == [(2, 513, 3), (1, 1, 1)]
  assert F.plan(1, 1027) == [(1, 1027, 5)] and F.plan(4, 4 * 256 * 3 + 2) == [(4, 768, 3), (1, 2, 1)]
  assert F.plan(4, 1 << 28)[0][2] == F.K_STEP_PIECE_CAP


# ---------------------------------------------------------------------------------------------------------------------
# The case lists against the instances

def _reached(group, cus=256):
  out = set()
  for c in F.cases(group, cus):
    out |= F.instances(c, cus)
  return out


def test_case_lists_reach_every_instance():
  want = F.source_instances()
  assert len(want) == 144
  assert len([i for i in want if i[0] == "stats" and i[6] is None]) == 72
  assert len([i for i in want if i[0] == "stream"]) == 18
  assert len([i for i in want if i[0] == "stats" and i[6] is not None]) == 48
  assert len([i for i in want if i[0] == "gram"]) == 6
  reached = {g: _reached(g) for g in F.GROUPS}
  union = set().union(*reached.values())
  family = {i for i in union if i[0] != "tail_gram"}
  assert family == want, (sorted(want - family, key=str), sorted(family - want, key=str))
  assert {i[1] for i in union if i[0] == "tail_gram"} == {1, 2, 3}
  # each group reaches exactly the family it exists for
  plain = {i for i in want if i[0] == "stats" and i[6] is None and not i[5]}
  assert reached["register"] == plain
  assert reached["stream"] == {i for i in want if i[0] == "stream"}
  assert reached["knob_stream"] == {i for i in want if i[0] == "stream" and i[1] == 20}
  assert reached["knob_burst"] | {i for i in plain if i[2] == 1} >= {i for i in want if i[0] == "stats" and i[6] is None and i[5]}
  assert {i for i in reached["knob_burst"] if i[5]} == {i for i in want if i[0] == "stats" and i[6] is None and i[5]}
  assert {i for i in reached["rule"] if i[6]} == {i for i in want if i[6] is not None and not i[5]}
  assert {i for i in reached["knob_burst_rule"] if i[6] and i[5]} == {i for i in want if i[6] is not None and i[5]}
  assert {i for i in reached["knob_burst_sqdist"] if i[0] == "gram"} == {i for i in want if i[0] == "gram"}
  # the neighbours take the two kernels
  for c in F.cases("rule"):
    fused = c.ks == c.h and (c.h, c.nb) in F.FUSED_RULE_SHAPES and c.offset == 0 and \
        (c.entry == "ms_colwise" or c.d % 4 == 0)
    assert F.is_fused(c, 256) == fused, c
  for c in F.cases("knob_burst_sqdist"):
    fused = (c.h, c.nb) in F.SQDIST_SHAPES and c.offset == 0 and c.d >= 256 * 2048 and \
        (c.entry == "ms_sqdist" or c.d % 4 == 0)
    assert F.is_fused(c, 256) == fused, c
  # at the defaults none of the knob cases would take its form: the parent's digests are the other form's
  for g in ("knob_burst", "knob_burst_rule", "knob_burst_sqdist", "knob_stream"):
    assert not {i for c in F.cases(g) for i in F.instances(c._replace(knobs=()), 256)} & \
        {i for i in reached[g] if i[5] or i[0] in ("gram", "stream")} or g == "knob_stream"


def test_parts_cover_their_groups():
  for group, parts in F.PARTS.items():
    whole = F.cases(group)
    split = [c for p in parts for c in F.cases(group, 256, p)]
    assert sorted(map(F.case_key, whole)) == sorted(map(F.case_key, split)), group
  keys = [F.case_key(c) for g in F.GROUPS for c in F.cases(g)]
  for g in F.GROUPS:
    ks = [F.case_key(c) for c in F.cases(g)]
    assert len(ks) == len(set(ks)), g


def test_burst_lengths_follow_the_cu_count():
  for cus in (256, 304, 64):
    for vec in (4, 2, 1):
      one, ragged = F.burst_lengths(vec, cus)
      knobs = dict(F.DEFAULT_KNOBS, BM_STEP_BURST=1)
      (v, nvec, grid), = F.plan(vec, one)
      assert v == vec and nvec == cus * 512 and F.burst_form(nvec, grid, cus, knobs)
      launches = F.plan(vec, ragged)
      assert launches[0][1] == cus * 512 + 512 * 3 + 70 and (len(launches) == 2) == (vec > 1)


# ---------------------------------------------------------------------------------------------------------------------
# The expected values against what the project already trusts

def _small_cases():
  seen, out = set(), []
  for c in F.all_cases():
    key = (c.entry.startswith("ss"), c.ks, c.h, c.kind, c.d, c.clip, c.bad)
    if c.d <= (1 << 16) and key not in seen:
      seen.add(key)
      out.append(c)
  return out


def test_averages_are_the_oracles():
  """Both averages bit for bit oracle.gar_oracle.compute_avg_dev_max in f32 mode (tools/pytorch.py:97-125), max|avg| its
  fourth result; the `empire` vector torch's own avg.add(avg.neg().mul_(factor))."""
  checked = 0
  for c in _small_cases():
    if c.d == 0 or (c.d not in (5, 1027) and c.bad is None):
      continue
    e = F.expected(c)
    for rows, avg, top in ((e.g, e.s_avg, e.max_s), (e.buffers, e.h_avg, e.max_h)):
      want, _, _, wmax = O.compute_avg_dev_max(list(rows))
      assert not bool(F.bits_differ(avg, want).any())
      assert (math.isnan(top) and math.isnan(wmax)) or top == wmax
    for scale in (1.1, -1.5):
      byz, exact = F.byzantine(e.h_avg, e.buffers, "empire", scale, False)
      assert exact and not bool(F.bits_differ(byz, e.h_avg.add(e.h_avg.neg().mul_(scale))).any())
      att, _ = F.byzantine(e.h_avg, e.buffers, "empire", scale, True)
      assert not bool(F.bits_differ(att, e.h_avg.neg().mul_(scale)).any())
    checked += 1
  assert checked > 100
  # the sequential sum and the true division, in plain Python on a few columns
  c = F._case("x", "ms", 12, 7, d=5)
  e = F.expected(c)
  import numpy as np
  for col in range(5):
    acc = np.float32(e.buffers[0, col].item())
    for i in range(1, 7):
      acc = np.float32(acc + np.float32(e.buffers[i, col].item()))
    assert np.float32(acc / np.float32(7)) == np.float32(e.h_avg[col].item())


def _fma_exact(a, x, y):
  """float32(a * x + y) with ONE rounding, in exact rational arithmetic."""
  exact = Fraction(a) * Fraction(x) + Fraction(y)
  if exact == 0:
    return 0.0
  lo = float(exact)  # float64 nearest: a starting point only
  cand = torch.tensor([lo], dtype=torch.float64).float()
  best = None
  for step in (-1, 0, 1):
    v = (cand.view(torch.int32) + step).view(torch.float32).item()
    err = abs(Fraction(v) - exact)
    even = (torch.tensor([v], dtype=torch.float32).view(torch.int32).item() & 1) == 0
    if best is None or err < best[0] or (err == best[0] and even):
      best = (err, v)
  return best[1]


def _bits(x):
  return torch.tensor([x], dtype=torch.float32).view(torch.int32).item()


def _check_fma(omd, mu, g, b):
  """(masked and equal, masked and 1 ulp apart) over the elements; asserts what the mask promises."""
  omd32 = torch.tensor(omd, dtype=torch.float32).item()
  got, mid = F.fma_emulated(omd, g[None], mu, b[None])
  got, mid = got[0], mid[0]
  mub = b * torch.tensor(mu, dtype=torch.float32)
  masked_same = masked_differ = 0
  for i in range(g.numel()):
    gi, yi = g[i].item(), mub[i].item()
    want = _fma_exact(omd32, gi, yi)
    same = _bits(want) == _bits(got[i].item())
    if not bool(mid[i]):
      assert same, (i, gi, b[i].item())  # mask clear: the emulation IS the fma
      continue
    assert abs(_bits(want) - _bits(got[i].item())) <= 1
    masked_same += same
    masked_differ += not same
    # mask set: the float64 sum is exactly halfway between its two fp32 neighbours
    v = omd32 * gi + yi  # Python floats: the float64 product (exact) and sum
    near = torch.tensor([v], dtype=torch.float64).float()
    away = (near.view(torch.int32) + (1 if (v > near.item()) == (v > 0) else -1)).view(torch.float32).item()
    assert abs(Fraction(v) - Fraction(near.item())) == abs(Fraction(away) - Fraction(v)), (i, v)
  return masked_same, masked_differ


def test_fma_emulation_and_its_midpoint_mask():
  """float32(float64(omd) * float64(g) + float64(fl32(mu * b))) against an exact-rational fma.  Where the mask is clear
  the emulation IS the fma; where it is set the float64 sum is exactly halfway between two fp32 numbers and the two
  differ by at most 1 ulp.  On random elements with the suite's coefficients, and on constructed near-midpoints:
  omd = 1 + 2^-23, mu = 1, b = y in [2^q, 2^(q+1)) and g = 2^(q-24) (1 - 2^-23), so that omd * g = 2^(q-24) (1 - 2^-46):
  the exact sum lies 2^(q-70) BELOW the midpoint y + ulp / 2 and an fma returns y, the float64 sum IS the midpoint and
  rounds to even — y when its last bit is clear, y + ulp when it is set.  The mask holds all of them, half of them
  differ: it is exactly the set where the two MAY differ."""
  gen = torch.Generator().manual_seed(5)
  g = torch.randn(3000, generator=gen)
  b = torch.randn(3000, generator=gen)
  g[:500] = (g[:500] * 256).round() / 256  # short mantissas: their products end in zeros, exact ties are frequent
  b[:500] = (b[:500] * 256).round() / 256
  same, differ = _check_fma(0.1, 0.9, g, b)
  print(f"random elements: {same + differ} masked of 3000, {differ} of them 1 ulp apart")
  built_g, built_b = [], []
  for k in range(400):
    q = k % 9 - 4
    y = torch.tensor([2.0 ** q * (1 + ((k * 7919) % 8388608) / 8388608)], dtype=torch.float32).item()
    built_b.append(y)
    built_g.append(2.0 ** (q - 24) * (1 - 2.0 ** -23))
  g, b = torch.tensor(built_g, dtype=torch.float32), torch.tensor(built_b, dtype=torch.float32)
  assert g.double().tolist() == built_g and b.double().tolist() == built_b
  same, differ = _check_fma(1 + 2.0 ** -23, 1.0, g, b)
  assert same + differ == 400 and differ >= 150 and same >= 150, (same, differ)


def test_midpoint_counts_are_within_the_cap():
  """Every case of up to 2^16 columns: at most MIDPOINT_CAP of its elements are fp32 midpoints of the float64 sum (for
  these sizes: none).  Longer cases are counted where they run."""
  total = elements = 0
  for c in _small_cases():
    n, el = F.midpoints(c)
    assert n <= F.MIDPOINT_CAP * el, (F.case_key(c), n, el)
    total += n
    elements += el
  print(f"midpoint elements: {total} of {elements} in {len(_small_cases())} distinct inputs")
  assert total == 0


@pytest.mark.parametrize("kind", ["iid", "momentum"])
def test_centring_at_the_fp32_average_is_not_what_the_bar_measures(kind):
  """The float64 deviation sums centred at the expected fp32 average and at the float64 average agree to 1e-6 relative:
  the 1e-5 bar measures the kernel, not the centring."""
  for ks, h in ((3, 3), (8, 5), (20, 20), (64, 50), (19, 1)):
    for clip in (False, True):
      c = F._case("x", "ms", ks, h, clip=clip, d=4 * 256 * 3 + 2, kind=kind)
      e = F.expected(c)
      for rows, (n2, dev) in ((e.g, e.sums_s), (e.buffers, e.sums_h)):
        if rows.shape[0] < 2:
          continue
        r64 = rows.double()
        mean = r64.mean(dim=0)
        dev64 = float(((r64 - mean) ** 2).sum())
        n64 = float((mean * mean).sum())
        assert abs(dev - dev64) <= 1e-6 * dev64, (ks, h, clip, dev, dev64)
        assert abs(n2 - n64) <= 1e-6 * n64, (ks, h, clip, n2, n64)
