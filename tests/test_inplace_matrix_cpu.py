"""The mirror of tests/inplace_matrix.py against the sources and the code object, its case lists against the launch
forms they claim to reach, its references against exact arithmetic, and numpy twins of five plausible defects against the
references on the cases' own inputs (no GPU needed).

Read out of csrc/ by pattern: block sizes and grid caps of the seven launch sites, Tail::kOwnLaunch at each, the pointers
whose alignment decides the width, the two folds and their period, the slot map of bm_multi_dot.  Where libbm_gar.so and
the LLVM tools are present every <1,2,4> instance must be in the code object."""

import importlib.util
import math
import pathlib
import re

import numpy as np
import pytest

from tests import inplace_matrix as X

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "byzantinemomentum_amd" / "csrc"
HEADER = ROOT / "include" / "bm_gar.h"
F32 = np.float32


def _read(name):
  return (CSRC / name).read_text()


def _int(pattern, text):
  m = re.search(pattern, text)
  assert m, pattern
  return int(m.group(1))


# ---------------------------------------------------------------------------------------------------------------------
# The mirror against the sources

def test_mirror_constants_match_the_sources():
  assert _int(r"#define\s+BM_MAX_ROWS\s+(\d+)", HEADER.read_text()) == X.BM_MAX_ROWS
  reduce, step, acg, search = _read("reduce.hip"), _read("step.hip"), _read("anticge.hip"), _read("search_eval.hip")
  colwise, plan = _read("colwise_kernels.h"), _read("launch_plan.h")
  red_block = _int(r"constexpr int kRedBlock = (\d+);", reduce)
  step_block = _int(r"constexpr int kStepBlock = (\d+);", step)
  acg_block = _int(r"constexpr int kAcgScaleBlock = (\d+);", acg)
  col_block = _int(r"constexpr int kColBlock = (\d+);", colwise)
  acg_cap = _int(r"constexpr int kAcgScaleBlocks = (\d+);", acg)
  norm_blocks = _int(r"constexpr int kNormBlocks = (\d+);", reduce)
  eval_cap = _int(r"constexpr int kEvalMaxBlocks = (\d+);", colwise)
  dot_cap = _int(r"constexpr Caps kDotCaps = caps_of\((\d+)\);", reduce)
  assert "constexpr Caps kEvalCaps = caps_of(kEvalMaxBlocks);" in colwise
  assert "constexpr Caps caps_of(int both) { return Caps{both, both}; }" in plan
  # every site: for_body_and_tail<4>(Tail::kOwnLaunch, vec, d, <block>, <caps>
  sites = {
    X.AXPBY: (reduce, r"multi_axpby_kernel<decltype", "kRedBlock, caps_of(2048)", red_block, 2048),
    X.FMA3: (step, r"multi_fma3_kernel<decltype", "kStepBlock, caps_of(2048)", step_block, 2048),
    X.SCALE: (step, r"multi_scale_kernel<decltype", "kStepBlock, caps_of(2048)", step_block, 2048),
    X.ANTICGE: (acg, r"anticge_scale_kernel<decltype", "kAcgScaleBlock, caps_of(kAcgScaleBlocks)", acg_block, acg_cap),
    X.SQNORMS: (reduce, r"row_sqnorms_kernel<VEC>", "kRedBlock, caps_of(kNormBlocks)", red_block, norm_blocks),
    X.SQDIST2: (search, r"sqdist2_kernel<decltype", "kColBlock, kEvalCaps", col_block, eval_cap),
    X.DOT: (reduce, r"multi_dot_kernel<decltype", "kRedBlock, kDotCaps", red_block, dot_cap),
  }
  assert set(sites) == set(X.SITES)
  for entry, (text, launch, args, block, cap) in sites.items():
    site = X.SITES[entry]
    assert (site.block, site.cap_body, site.cap_tail) == (block, cap, cap), entry
    assert (CSRC / site.source).read_text() is not None and site.kernel in text
    # the launch of this kernel follows a cut with exactly these arguments
    cut = re.compile(r"for_body_and_tail<4>\(Tail::kOwnLaunch, [^\n]*?d, " + re.escape(args) + r"[^\n]*\n(?:[^\n]*\n){0,3}?[^\n]*" + launch)
    assert cut.search(text), entry
  assert X.MAX_VEC == 4 and X.TAIL_OWN_LAUNCH
  # the plan itself
  assert "return (bits_ & 15u) == 0 ? 4 : ((bits_ & 7u) == 0 ? 2 : 1);" in plan
  assert [X.vec_of([o]) for o in (0, 4, 8, 12)] == [4, 1, 2, 1] and X.vec_of([0, 8]) == 2 and X.vec_of([]) == 4
  assert "if (mode == Tail::kOwnLaunch && d / vec == 0) vec = 1;" in plan
  assert "if (d > 0 && (vec > 1 || mode != Tail::kOwnLaunch)) {" in plan
  assert "Span span{body, rest, d, 0, body == 0 ? stream_grid(rest, block, caps.tail) : 1, parts};" in plan
  assert "Span span{0, nvec, body + rides, rides, stream_grid(nvec, block, caps.body), parts};" in plan
  assert "int64_t g = (work_items + block - 1) / block;" in plan and "if (g < 1) g = 1;" in plan
  # the pointers that decide the width
  assert "Alignment().of(y, k).of(x, k).vec()" in reduce
  assert "Alignment().of(out, k).of(p, k).of(q, k).vec()" in step
  assert "Alignment().of(y, k).vec()" in step
  assert "Alignment().of(vec).vec()" in acg
  assert "Alignment().of(rows, k).vec()" in reduce
  assert "Alignment().of(a).of(b).vec()" in search
  assert "Alignment().of(core, nc).of(extra, ne).vec()" in reduce
  # the grid-stride loops and the folds
  for text, block in ((reduce, "kRedBlock"), (step, "kStepBlock"), (acg, "kAcgScaleBlock"), (search, "kColBlock")):
    assert f"const int64_t stride = (int64_t)gridDim.x * {block};" in text
  assert "for (; v + stride < nvec; v += 2 * stride) {  // two loads in flight per lane" in reduce and X.K_NORM_LOADS == 2
  assert reduce.count("if (++since == 16) {") == 1 and search.count("if (++since == 16) {") >= 1 and X.K_FOLD_EVERY == 16
  assert "(VEC == 1 ? ntail : nbody) = sp.grid;" in reduce
  assert "double* tail_part = body_part + (int64_t)BM_MAX_ROWS * kNormBlocks;" in reduce
  # bm_multi_dot's slots
  assert _int(r"constexpr int kMaxCore = (\d+);", reduce) == X.K_MAX_CORE
  assert _int(r"constexpr int kMaxExtra = (\d+);", reduce) == X.K_MAX_EXTRA
  assert "constexpr int kDotSlots = kMaxCore * (kMaxCore + 1) / 2 + kMaxExtra;" in reduce and X.K_DOT_SLOTS == 42
  assert [X.dot_slot(a, b) for a in range(4) for b in range(a, 4)] == list(range(10))
  # the arithmetic the references restate
  assert "yy[c] = __builtin_fmaf(b, xx[c], a * yy[c]);" in reduce
  assert "const float x = pscale != nullptr ? pp[e] * c : pp[e];" in step and "pp[e] = __builtin_fmaf(b, qq[e], a * x);" in step
  assert "const float b = b_dev != nullptr ? (float)b_dev[0] : b_host;" in step
  assert "if (c == 1.0f) return;" in step and "yy[e] *= c;" in step
  assert "factors[i] = (norm > (double)clip) ? (float)((double)clip / norm) : 1.0f;" in step
  assert "*mult = (float)(-nextafter(norm, 0.0) / (double)attnorm);" in acg and "if (!(attnorm > 0.0f)) return false;" in acg


def test_code_object_holds_every_instance():
  spec = importlib.util.spec_from_file_location("kernel_meta", ROOT / "scripts" / "kernel_meta.py")
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  if not mod.LIB.exists() or not (mod.LLVM / "llvm-objdump").exists():
    pytest.skip("libbm_gar.so or the LLVM tools are not here")
  names = {s.kernel for s in X.SITES.values()}
  found = set()
  for k in mod.kernels():
    m = re.search(r"\b(\w+_kernel)<(\d+)>", k["demangled"])
    if m and m.group(1) in names:
      found.add((m.group(1), int(m.group(2))))
  assert found == X.universe() and len(found) == 21
  assert any("clip_factors_kernel" in k["demangled"] for k in mod.kernels())


# ---------------------------------------------------------------------------------------------------------------------
# Reach

def _writer_forms(entry):
  out = {}
  for c in X.all_writer_cases():
    if c.entry == entry:
      for f in X.forms(entry, X.writer_pointers(c), c.d):
        out.setdefault(f, []).append(c)
  return out


def test_case_lists_reach_every_instance():
  reached = set()
  for c in X.all_writer_cases():
    reached |= X.instances(c.entry, X.writer_pointers(c), c.d)
  for c in X.all_reduction_cases():
    reached |= X.instances(c.entry, X.reduction_offsets(c), c.d)
  assert reached == X.universe()
  # the short list alone reaches them, at every row count
  for entry in X.WRITERS:
    for k in ((1,) if entry == X.ANTICGE else X.K_SHORT):
      got = set()
      for c in X.writer_cases("short", entry, None if entry == X.ANTICGE else k):
        got |= X.instances(entry, X.writer_pointers(c), c.d)
      assert got == {(X.SITES[entry].kernel, w) for w in (1, 2, 4)}, (entry, k)


@pytest.mark.parametrize("entry", X.WRITERS)
def test_writer_lists_reach_every_launch_form(entry):
  forms = _writer_forms(entry)
  assert set(forms) == {"tail_alone", "scalar", "body", "tail_behind_body", "second_trip"}
  # the tail alone at both wide widths: d = 1 at 8 bytes; d = 1, 2, 3 at 16 bytes
  alone = {(X.vec_of(X.writer_pointers(c)), c.d) for c in forms["tail_alone"]}
  assert alone >= {(2, 1), (4, 1), (4, 2), (4, 3)}
  # a body without a tail, and a tail of 1, 2 and 3 columns behind a body, one workgroup against several
  shapes = set()
  for c in X.writer_cases("short", entry, None if entry == X.ANTICGE else 20):
    ls = X.writer_launches(c)
    if ls[0].width > 1:
      shapes.add((ls[0].width, ls[1].count if len(ls) > 1 else 0, ls[0].grid > 1))
  assert shapes >= {(4, 0, False), (4, 1, False), (4, 2, False), (4, 3, False), (4, 3, True), (4, 0, True),
                    (2, 0, False), (2, 1, False), (2, 1, True), (2, 0, True)}
  # the second trip: at every width exactly one whole workgroup loops twice (width 1: and three lanes of a second one),
  # the widest tail behind it; no other case loops
  second = [c for c in X.all_writer_cases() if c.entry == entry and c.group == "second_trip"]
  assert sorted(c.d for c in second) == [524547, 1049089, 2098179]
  seen = set()
  for c in second:
    ls = X.writer_launches(c)
    seen.add(ls[0].width)
    assert ls[0].grid == X.SITES[entry].cap_body and ls[0].trips == 2 and c.d == X.second_trip_d(entry, ls[0].width)
    assert ls[0].second == (2 if ls[0].width == 1 else 1)
    assert ls[0].count - ls[0].grid * 256 == (259 if ls[0].width == 1 else 256)
    assert (len(ls) == 1) if ls[0].width == 1 else (ls[1].count == ls[0].width - 1 and ls[1].grid == 1)
    # one vector shorter and no workgroup is whole on its second trip
    assert X.for_body_and_tail(ls[0].width, c.d - ls[0].width * (4 if ls[0].width == 1 else 1), 256, 2048, 2048)[0].count \
        - 2048 * 256 < 256
    # the special elements of the row's end lie on the second trip
    assert c.d - X.END >= ls[0].width * ls[0].grid * 256
  assert seen == {1, 2, 4}
  for c in X.all_writer_cases():
    if c.entry == entry and c.group != "second_trip":
      assert all(l.trips == 1 for l in X.writer_launches(c)), c
  # the existing length, 300 007 at 4-byte rows, never loops: 1172 workgroups
  (l,) = X.launches(entry, [4], 300007)
  assert (l.grid, l.trips) == (1172, 1)


def test_writer_lists_cover_the_forced_widths_and_the_row_counts():
  for entry in (X.AXPBY, X.FMA3):
    forced = X.writer_cases("forced", entry)
    assert {(c.out_off, c.in_off) for c in forced} == {(4, 0), (8, 0), (0, 4), (0, 8)}
    for c in forced:
      outs, ins = X.writer_offsets(c)
      off = max(c.out_off, c.in_off)
      assert X.vec_of(outs + ins) == {4: 1, 8: 2}[off] and max(X.vec_of(outs), X.vec_of(ins)) == 4
      assert X.vec_of(outs) != X.vec_of(ins) and X.vec_of(outs + ins) == min(X.vec_of(outs), X.vec_of(ins))
  for entry in (X.AXPBY, X.FMA3, X.SCALE):
    assert {c.k for c in X.writer_cases("short", entry)} == {1, 2, 20, 63, 64}
    assert {c.d for c in X.writer_cases("short", entry)} >= {1, 2, 3, 4, 5, 7, 255, 256, 259, 1027, 4100}
    assert {c.out_off for c in X.writer_cases("short", entry)} == {0, 4, 8, "mixed"}
  forms = X.writer_cases("fma3_forms", X.FMA3)
  assert {(c.form, c.bdev, c.pscale) for c in forms} == {(f, b, p) for f in ("inplace", "fresh", "shared_q", "nesterov")
                                                         for b in (False, True) for p in (False, True)}
  for c in forms:
    if c.form == "nesterov":
      assert c.k == 1 and X.coef_of(c)[0] == 1.0
    if c.pscale:
      f = X.factors_for(c.k)[:c.k]
      assert f[0] == 1 and (c.k == 1 or ((f == 1).sum() >= 2 and (f != 1).sum() >= 2))
  assert {c.special for c in X.writer_cases("scale_special", X.SCALE)} == {"pow2", "arbitrary", "one_on_snan", "zero"}
  assert {c.special for c in X.writer_cases("anticge_special", X.ANTICGE)} == {"ordinary", "zero_norm", "nan_norm", "inf_byz"}


def test_reduction_lists_reach_the_folds_and_both_partial_areas():
  sq = X.reduction_cases(X.SQNORMS)
  # no short case folds; the fold cases do, with lanes that then take the single-load remainder
  for c in sq:
    walks = [X.sqnorm_walk(l.count, l.grid) for l in X.reduction_launches(c)]
    if c.group == "fold":
      w = walks[0]
      assert w.iterations > X.K_FOLD_EVERY and w.folds == 128 * 256 and 0 < w.remainder_after_fold < w.folds, (c, w)
    else:
      assert all(w.folds == 0 for w in walks), c
  fold = [c for c in sq if c.group == "fold"]
  assert [c.d for c in fold] == [1146885, 4 * 1146885 + 3]
  assert [[(l.width, l.count) for l in X.reduction_launches(c)] for c in fold] == [[(1, 1146885)], [(4, 1146885), (1, 3)]]
  assert any(X.sqnorm_walk(l.count, l.grid).plain_remainder for c in sq if c.group == "short" for l in X.reduction_launches(c))
  # the existing length never folds
  assert X.sqnorm_walk(300007, 128).folds == 0 and X.sqdist_walk(300007, 1172)[1] == 0
  # both partial areas in use at k = 64; each alone with several workgroups
  areas = {(c.d, c.offs): X.sqnorm_areas(X.reduction_offsets(c), c.d) for c in sq if c.group == "areas"}
  assert areas == {(1027, 0): (1, 1), (4103, 0): (5, 1), (1027, 4): (0, 5), (4100, 8): (9, 0)}
  assert all(c.k == 64 for c in sq if c.group == "areas")
  assert {c.k for c in sq if c.group == "short"} == {1, 2, 20, 63, 64}
  # sqdist2: the shortest length that folds, and only there
  sd = X.reduction_cases(X.SQDIST2)
  (fold,) = [c for c in sd if c.group == "fold"]
  (l,) = X.reduction_launches(fold)
  assert fold.d == 7864321 and (l.width, l.grid) == (1, 2048) and X.sqdist_walk(l.count, l.grid) == (16, 1)
  assert X.sqdist_walk(l.count - 1, l.grid) == (15, 0)
  for width in (2, 4):     # a wider row folds no earlier
    assert X.sqdist_walk((fold.d - 1) // width, 2048)[1] == 0
  stride = 2048 * 256
  v = X.reduction_input(fold._replace(d=stride * 2 + 1))
  assert (np.abs(v[0, ::stride]) > 3000).all()
  for c in sd:
    if c.group != "fold":
      assert all(X.sqdist_walk(l.count, l.grid)[1] == 0 for l in X.reduction_launches(c))
  assert {c.group for c in sd} == {"short", "fold", "equal", "empty"}
  # multi_dot: every nc with every ne, every slot of the finish kernel's map
  dots = X.reduction_cases(X.DOT)
  assert {(c.nc, c.ne) for c in dots} == {(nc, ne) for nc in (1, 2, 3, 4) for ne in (0, 1, 31, 32)}
  assert {c.d for c in dots} == {3, 1027} and {c.offs for c in dots} == {0, 4, 8, "mixed"}
  slots = {X.dot_slot(a, b) for c in dots for a in range(c.nc) for b in range(a, c.nc)} | \
      {10 + e for c in dots for e in range(c.ne)}
  assert slots == set(range(X.K_DOT_SLOTS))


# ---------------------------------------------------------------------------------------------------------------------
# Layout and values

def test_layout_keeps_guard_gaps_and_offsets():
  for offs in ([0, 0, 0], [4, 8, 12], X.row_offsets("mixed", 7), [12]):
    for d in (1, 3, 4, 255, 1027):
      total, starts = X.layout([(d, o) for o in offs])
      assert total % 4 == 0
      prev_end = 0
      for s, o in zip(starts, offs):
        assert (4 * s) % 16 == o and s - prev_end >= X.GUARD
        prev_end = s + d
      assert total - prev_end >= X.GUARD
  flat = X.Flat([np.ones(5, dtype=F32), np.zeros(3, dtype=F32)], [4, 8])
  assert (flat.bits == X.SENTINEL).sum() == flat.total - 8
  want, loose = flat.expected({0: (np.full(5, np.nan, dtype=F32), False)})
  got = want.copy()
  got[flat.starts[0]] = 0xFFC00001                      # another NaN in an output: the same
  assert X.first_mismatch(got, want, loose) is None
  got[flat.starts[1] + 3] = 0                           # one float behind the second vector
  assert X.first_mismatch(got, want, loose) == flat.starts[1] + 3 and flat.where(flat.starts[1] + 3) == (None, flat.starts[1] + 3)
  assert X.row_offsets("mixed", 4) == [4, 0, 12, 8]


def test_special_elements_land_where_they_are_claimed():
  for k in (20, 63, 64):
    for d in (1027, 259, 4100):
      kinds = X.kind_map(k, d)
      for kind in range(X.NK):
        rows, cols = np.nonzero(kinds == kind)
        # every kind in every lane position of a 16-byte group: at the start, in the middle of the first wave, at the end
        assert {c % 4 for c in cols if c < 128} == {0, 1, 2, 3}
        if d > 256 + X.END:
          assert {c % 4 for c in cols if 128 <= c < 256} == {0, 1, 2, 3}
        assert {c % 4 for c in cols if c >= d - X.END} == {0, 1, 2, 3}
        # and in every trailing column (the tail launches of both wide widths)
        for c in (d - 1, d - 2, d - 3):
          assert kind in kinds[:, c]
      assert (kinds[:, 300:d - X.END] == -1).all() if d > 400 else True
  # the tail alone: every column of d = 1, 2, 3 holds every kind over the rows
  for d in (1, 2, 3):
    assert all(set(X.kind_map(20, d)[:, c]) == set(range(X.NK)) for c in range(d))


def test_special_values_are_what_they_are_called():
  for flip in (False, True):
    x, y, kinds = X.values(20, 1027, flip)
    at = lambda name: kinds == X.KINDS.index(name)  # noqa: E731
    assert np.isnan(x[at("nan_x")]).all() and not np.isnan(y[at("nan_x")]).any()
    assert np.isnan(y[at("nan_y")]).all() and not np.isnan(x[at("nan_y")]).any()
    assert np.isinf(x[at("inf")]).all() and {1.0, -1.0} == set(np.sign(x[at("inf")]))
    assert (x[at("inf_minus_inf")] == np.inf).all() and (y[at("inf_minus_inf")] == (np.inf if flip else -np.inf)).all()
    z = at("zeros")
    assert not x[z].any() and not y[z].any()
    assert {(bool(a), bool(b)) for a, b in zip(np.signbit(x[z]), np.signbit(y[z]))} == {(False, False), (True, False),
                                                                                      (False, True), (True, True)}
    s = at("subnormal_in")
    assert (np.abs(x[s]) < 2.0 ** -126).all() and (x[s] != 0).all() and (np.abs(y[s]) < 2.0 ** -126).all()
    h = at("huge")
    assert np.isfinite(x[h]).all() and (np.abs(y[h]) >= 2.3e38).all() and (np.abs(x[h]) >= 3.2e38).all()
    ordinary = kinds == -1
    assert np.isfinite(x[ordinary]).all() and np.isfinite(y[ordinary]).all()
    # scales differ by row
    stds = x[:, 300:900].std(axis=1)
    assert (np.diff(stds) > 0).sum() >= 17
  # per coefficient pair the references show what the kinds are for
  for a, b in X.COEFS + (X.NESTEROV,):
    x, y, kinds = X.values(20, 1027, a * b < 0)
    out, counts = X.axpby_reference(y, x, a, b)
    at = lambda name: kinds == X.KINDS.index(name)  # noqa: E731
    assert np.isnan(out[at("nan_x")]).all() and np.isnan(out[at("nan_y")]).all() and np.isnan(out[at("inf_minus_inf")]).all()
    assert np.isinf(out[at("inf")]).all()
    assert (np.abs(out[at("subnormal_in")]) < 2.0 ** -126).all() and counts.subnormal >= at("subnormal_in").sum()
    if abs(a) > 1:
      assert np.isinf(out[at("huge")]).all()            # fl32(a y) overflows although the exact sum does not
      exact = np.float64(F32(b)) * x[at("huge")].astype(np.float64) + np.float64(F32(a)) * y[at("huge")].astype(np.float64)
      assert (np.abs(exact) < 3.4e38).all()
    elif abs(a) < 1:
      assert np.isfinite(out[at("huge")]).all()
    if abs(a) < 1 and abs(b) < 1:
      assert (np.abs(out[at("subnormal_out")]) < 2.0 ** -126).any()
  assert any(abs(a) > 1 for a, _ in X.COEFS) and any(a * b < 0 for a, b in X.COEFS)


# ---------------------------------------------------------------------------------------------------------------------
# The references

def test_round_f32_is_one_correct_rounding():
  from fractions import Fraction
  rng = np.random.default_rng(5)
  for v in rng.standard_normal(300) * 10.0 ** rng.integers(-44, 38, size=300):
    assert X.round_f32(Fraction(float(v))) == float(F32(v)), v              # numpy's own double -> float rounding
  tie = Fraction(2 ** 24 + 1)                                               # halfway between 2^24 and 2^24 + 2
  assert X.round_f32(tie) == 2.0 ** 24 and X.round_f32(tie + Fraction(1, 10 ** 30)) == 2.0 ** 24 + 2
  assert X.round_f32(Fraction(3, 2) * Fraction(2) ** -149) == 2 * 2.0 ** -149     # a subnormal tie goes to even
  assert X.round_f32(Fraction(1, 2) * Fraction(2) ** -149) == 0.0
  top = Fraction(2) ** 128 - Fraction(2) ** 103
  assert X.round_f32(top) == math.inf and X.round_f32(-top) == -math.inf and X.round_f32(top - 1) == float(np.finfo(F32).max)
  assert math.copysign(1.0, X.fma_exact(F32(-1.0), F32(0.0), F32(-0.0))) == -1.0
  assert math.copysign(1.0, X.fma_exact(F32(1.0), F32(0.0), F32(-0.0))) == 1.0
  assert math.copysign(1.0, X.fma_exact(F32(2.0), F32(1.0), F32(-2.0))) == 1.0


def test_fused_reference_equals_exact_arithmetic():
  """fma_emulated with the flagged and the small coordinates redone exactly, against Fraction on EVERY coordinate: the
  special elements of a case, random ones, and crafted fp32 midpoints of the float64 sum."""
  total = 0
  for (a, b), factors in ((X.COEFS[0], None), (X.COEFS[1], X.factors_for(20)), (X.COEFS[2], None), (X.NESTEROV, None)):
    x, y, _ = X.values(20, 259, a * b < 0)
    got, counts = X.fma3_reference(y, x, a, b, factors)
    assert X.first_mismatch(got.view(np.uint32).ravel(), X.fma3_all_exact(y, x, a, b, factors).view(np.uint32).ravel(),
                            np.ones(got.size, dtype=bool)) is None
    total += got.size
    print(f"a={a} b={b} factors={factors is not None}: {counts.midpoints} midpoints, {counts.subnormal} small, of {counts.total}")
  # crafted midpoints: b = 1, q = 2^-24 (1 + 2 j) times the ulp of t: the float64 sum is exactly halfway
  t = (1.0 + np.arange(1, 65, dtype=np.float64) * 2.0 ** -23).astype(F32).reshape(1, -1)
  q = np.full_like(t, 2.0 ** -24)
  got, counts = X.fma3_reference(t, q, 1.0, 1.0)
  assert counts.midpoints == t.size
  assert (got.view(np.uint32) == X.fma3_all_exact(t, q, 1.0, 1.0).view(np.uint32)).all()
  assert (got.view(np.uint32) & 1 == 0).all()                               # ties went to even
  # a sum of three terms that double rounding would get wrong: b q = 2^-24 + 2^-60 above a midpoint that float64 loses
  q2 = np.full_like(t, 2.0 ** -24 * (1 + 2.0 ** -20))
  b2 = F32(1 + 2.0 ** -20)
  got, _ = X.fma3_reference(t, q2, 1.0, b2)
  assert (got.view(np.uint32) == X.fma3_all_exact(t, q2, 1.0, b2).view(np.uint32)).all()
  assert total > 15000


def test_axpby_reference_is_the_fused_reference_in_place():
  x, y, _ = X.values(20, 1027)
  for a, b in X.COEFS:
    one, _ = X.axpby_reference(y, x, a, b)
    two, _ = X.fma3_reference(y, x, a, b, None)
    assert (one.view(np.uint32) == two.view(np.uint32)).all()
  ones = np.ones(64, dtype=F32)
  with_ones, _ = X.fma3_reference(y, x, 0.9, 0.1, ones)
  assert X.first_mismatch(with_ones.view(np.uint32).ravel(), X.axpby_reference(y, x, 0.9, 0.1)[0].view(np.uint32).ravel(),
                          np.ones(y.size, dtype=bool)) is None


def test_no_coordinate_is_left_out():
  """Per case: how many coordinates were resolved exactly — printed (`pytest -s`); the expected image covers every element
  of every output, and every other float of the allocation keeps its bits.  (The long rows of the second trip are
  prepared where the GPU tests run; the probe counts theirs.)"""
  mid = small = total = 0
  for c in X.all_writer_cases():
    if c.group == "second_trip":
      continue
    pre = X.prepare(c)
    want, loose = pre.flat.expected(pre.outputs)
    covered = np.zeros(pre.flat.total, dtype=bool)
    for i in pre.outputs:
      covered[pre.flat.starts[i]:pre.flat.starts[i] + c.d] = True
    assert covered.sum() == c.k * c.d and (want[~covered] == pre.flat.bits[~covered]).all()
    assert (loose <= covered).all()
    print(f"{c.entry} {c.group} k={c.k} d={c.d} off={c.out_off}/{c.in_off} {c.form}: {pre.counts.midpoints} midpoints, "
          f"{pre.counts.subnormal} small, of {c.k * c.d}; 0 skipped")
    mid, small, total = mid + pre.counts.midpoints, small + pre.counts.subnormal, total + c.k * c.d
  print(f"{mid} midpoint-flagged and {small} subnormal-path coordinates resolved exactly, of {total}; none skipped")
  assert small > 0


def test_scalar_references():
  clip = 2.5
  c2 = float(np.float64(F32(clip)) ** 2)
  sq = np.array([0.0, c2 * 0.99, c2, np.nextafter(c2, np.inf), 4 * c2, np.inf, np.nan, 1e-300], dtype=np.float64)
  got = X.clip_factors_reference(sq, clip)
  assert got.dtype == F32 and got[:3].tolist() == [1.0, 1.0, 1.0] and got[4] == 0.5 and got[5] == 0.0 and got[6] == 1.0
  assert got[3] == 1.0 or got[3] == np.nextafter(F32(1.0), F32(0.0))
  assert X.anticge_multiplier((0.0, 4.0)) is None and X.anticge_multiplier((math.nan, 4.0)) is None
  assert X.anticge_multiplier((4.0, 9.0)) == F32(-np.nextafter(3.0, 0.0) / 2.0)
  assert X.anticge_multiplier((4.0, math.inf)) == -np.inf
  y = X.scale_input(X.writer_cases("scale_special", X.SCALE)[2])
  assert X.writer_cases("scale_special", X.SCALE)[2].special == "one_on_snan"
  bits = y.view(np.uint32)[0]
  assert set(bits.tolist()) == set(X.SNAN_BITS) and np.isnan(y[0]).sum() >= y.shape[1] // 2


# ---------------------------------------------------------------------------------------------------------------------
# Five plausible defects as numpy twins: the case lists tell each from the reference

def _bits_differ(a, b):
  return X.first_mismatch(np.ascontiguousarray(a, dtype=F32).view(np.uint32).ravel(),
                          np.ascontiguousarray(b, dtype=F32).view(np.uint32).ravel(), np.ones(a.size, dtype=bool)) is not None


def _fma_cases():
  seen = set()
  for c in X.all_writer_cases():
    key = (c.k, c.d, c.coef, c.pscale)
    if c.entry in (X.AXPBY, X.FMA3) and c.group != "second_trip" and c.k in (20, 64) and c.d >= 255 and key not in seen:
      seen.add(key)
      yield c


def test_twin_unfused_shows():
  n = 0
  for c in _fma_cases():
    a, b = X.coef_of(c)
    x, y, _ = X.values(c.k, c.d, a * b < 0)
    f = X.factors_for(c.k) if c.pscale else None
    assert _bits_differ(X.twin_unfused(y, x, a, b, f), X.fma3_reference(y, x, a, b, f)[0]), c
    n += 1
  assert n >= 8


def test_twin_factor_after_a_shows():
  n = 0
  for c in _fma_cases():
    if c.pscale:
      a, b = X.coef_of(c)
      x, y, _ = X.values(c.k, c.d, a * b < 0)
      f = X.factors_for(c.k)
      assert _bits_differ(X.twin_factor_after_a(y, x, a, b, f), X.fma3_reference(y, x, a, b, f)[0]), c
      n += 1
  assert n >= 2


def test_twin_b_rounded_twice_shows():
  n = 0
  for c in X.writer_cases("fma3_forms", X.FMA3):
    if c.bdev and c.d >= 255 and not c.pscale:
      a, b = X.coef_of(c)
      wrong = X.twin_b_rounded_twice(b)
      if wrong == F32(b):
        continue
      x, y, _ = X.values(c.k, c.d, a * b < 0)
      assert _bits_differ(X.fma3_reference(y, x, a, wrong)[0], X.fma3_reference(y, x, a, F32(b))[0]), c
      n += 1
  assert n >= 1


def test_twin_tail_at_body_width_shows():
  """A tail stored as a whole vector overwrites the guard gap behind the row (or the next row's gap): the comparison of
  the whole allocation sees it at every case with a tail."""
  n = 0
  for c in X.writer_cases("short", X.SCALE, 20) + X.writer_cases("short", X.AXPBY, 2):
    ls = X.writer_launches(c)
    if len(ls) == 2:
      pre = X.prepare(c)
      want, loose = pre.flat.expected(pre.outputs)
      width = ls[0].width
      got = want.copy()
      for i in pre.outputs:
        s = pre.flat.starts[i]
        body = c.d // width * width
        got = X.twin_tail_at_body_width(got, s, c.d, width, np.resize(want[s + body:s + c.d], width))
      at = X.first_mismatch(got, want, loose)
      assert at is not None and pre.flat.where(at)[0] is None, c
      n += 1
  assert n >= 10


def test_twin_scale_all_rows_shows():
  n = 0
  for c in X.writer_cases("scale_special", X.SCALE):
    if c.special == "one_on_snan":
      y, f = X.scale_input(c), X.scale_factors(c)
      want, same = X.scale_reference(y, f)
      assert same[0] and (want[0].view(np.uint32) == y[0].view(np.uint32)).all()
      wrong = X.twin_scale_all_rows(y, f)
      assert (wrong[0].view(np.uint32) != want[0].view(np.uint32)).any(), c
      n += 1
  assert n >= 4
