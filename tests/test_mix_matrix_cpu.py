"""The mirror of tests/mix_matrix.py against the sources and the code object, its case lists against the 300 compiled
instances of the mixing kernels, and the conditions its inputs and mask sets must meet, computed with the numpy
reference alone (no GPU needed).

Read out of csrc/ by pattern: the row limit of the 16-byte instances of mix_rows_kernel, kMixedMaxRows, kMixedMaxVec,
Tail::kRides at both launch sites, the pointers whose alignment decides the width, kColBlock, kColMaxBlocks and the piece
length.  Where libbm_gar.so and the LLVM tools are present the kernels of the code object must be exactly the mirror's
universe.  The last tests run numpy twins of three deliberate defects of mix_one against the reference on the cases'
own inputs: each must show in the case lists."""

import importlib.util
import pathlib
import re

import numpy as np
import pytest

from tests import instance_matrix as M
from tests import mix_matrix as X
from tests import nnm_cases as nc

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "byzantinemomentum_amd" / "csrc"
HEADER = ROOT / "include" / "bm_gar.h"


def _read(name):
  return (CSRC / name).read_text()


def _product(expr):
  out = 1
  for factor in expr.split("*"):
    out *= int(factor)
  return out


# ---------------------------------------------------------------------------------------------------------------------
# The mirror against the sources

def test_mirror_constants_match_the_sources():
  header = HEADER.read_text()
  assert int(re.search(r"#define\s+BM_MAX_ROWS\s+(\d+)", header).group(1)) == X.BM_MAX_ROWS
  rows = _read("mix_rows.hip")
  m = re.search(r"constexpr int mix_max_vec\(\) \{\s*return N <= (\d+) \? (\d+) : (\d+);", rows)
  assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (X.K_MIX_WIDE_ROWS, 4, 2)
  assert [X.mix_max_vec(n) for n in (1, 28, 29, 64)] == [4, 4, 2, 2]
  assert "std::make_integer_sequence<int, BM_MAX_ROWS>" in rows and "n == Ns + 1" in rows        # N = 1 .. 64
  fused = _read("colwise_mixed_dispatch.h")
  assert int(re.search(r"constexpr int kMixedMaxRows\s*=\s*(\d+);", fused).group(1)) == X.K_MIXED_MAX_ROWS
  assert int(re.search(r"constexpr int kMixedMaxVec\s*=\s*(\d+);", fused).group(1)) == X.K_MIXED_MAX_VEC
  for rule, op in ((X.MEDIAN, "BM_OP_MEDIAN"), (X.TRMEAN, "BM_OP_TRMEAN")):
    assert f"colwise_mixed_dispatch<{op}, 1, kMixedMaxRows>" in _read(f"colwise_mixed_{rule}.hip")  # N = 1 .. 36
  # the d % VEC trailing columns ride in the body's launch at the pointers' width, capped per kernel
  assert "for_body_and_tail<mix_max_vec<N>()>(Tail::kRides, vec, d, kColBlock, caps_of(kColMaxBlocks)" in rows
  assert "for_body_and_tail<kMixedMaxVec>(Tail::kRides, vec, d, kColBlock, caps_of(kColMaxBlocks)" in fused
  assert X.TAIL_RIDES
  plan = _read("launch_plan.h")
  assert re.search(r"kRides,\s*// the last workgroup of the body's launch takes them, at the pointers' width whatever d is", plan)
  assert "while (mode == Tail::kRidesNarrowed && vec > 1 && d / vec == 0) vec /= 2;" in plan     # only that mode narrows
  # the width: every input AND every output pointer of the piece
  assert "Alignment().of(t.p, N).of(o.p, n_out).vec()" in rows
  assert "Alignment().of(t.p, N).of(o).vec()" in fused
  assert "return (bits_ & 15u) == 0 ? 4 : ((bits_ & 7u) == 0 ? 2 : 1);" in plan
  assert [M.vec_width([o]) for o in (0, 4, 8, 12)] == [4, 1, 2, 1]
  for text in (rows, fused):
    assert "tuning().wsum_piece > 0 ? (int64_t)tuning().wsum_piece : kMaxColsPerLaunch" in text
  assert re.search(r"kMaxColsPerLaunch = \(int64_t\)1 << 29;", plan) and X.K_MAX_COLS_PER_LAUNCH == 1 << 29
  assert int(re.search(r"constexpr int kColBlock\s*=\s*(\d+);", _read("colwise_kernels.h")).group(1)) == X.K_COL_BLOCK
  blocks = re.search(r"constexpr int kColMaxBlocks\s*=\s*([\d *]+);", _read("bm_common.h")).group(1)
  assert _product(blocks) == X.K_COL_MAX_BLOCKS and X.TRIP == X.K_COL_BLOCK * X.K_COL_MAX_BLOCKS
  # the kernels' loop: groups = nvec + (tail > 0), stride = grid * kColBlock, one workgroup per kColBlock body groups
  kernels = _read("mix_kernels.h")
  assert kernels.count("groups = nv + (tail > 0 ? 1u : 0u);") == 2
  assert kernels.count("g < groups; g += stride") == 2
  assert "Span span{0, nvec, body + rides, rides, stream_grid(nvec, block, caps.body), parts};" in plan


def test_universe_size():
  u = X.universe()
  assert len([i for i in u if i[0] == X.MIX_ROWS]) == 156 and len([i for i in u if i[0] == X.FUSED]) == 144


def test_code_object_holds_exactly_the_universe():
  spec = importlib.util.spec_from_file_location("kernel_meta", ROOT / "scripts" / "kernel_meta.py")
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  if not mod.LIB.exists() or not (mod.LLVM / "llvm-objdump").exists():
    pytest.skip("libbm_gar.so or the LLVM tools are not here")
  ops = {int(v): k.lower() for k, v in re.findall(r"\bBM_OP_(MEDIAN|TRMEAN)\s*=\s*(\d+)", HEADER.read_text())}
  found = []
  for k in mod.kernels():
    m = re.search(r"mix_rows_kernel<(\d+), (\d+)>", k["demangled"])
    if m:
      found.append((X.MIX_ROWS, int(m.group(1)), int(m.group(2))))
    m = re.search(r"colwise_mixed_kernel<(\d+), (\d+), (\d+)>", k["demangled"])
    if m:
      found.append((X.FUSED, int(m.group(1)), ops[int(m.group(2))], int(m.group(3))))
  assert len(found) == len(set(found)) == 300
  assert set(found) == X.universe()


# ---------------------------------------------------------------------------------------------------------------------
# Coverage

def test_case_lists_reach_every_instance():
  universe = X.universe()
  reached = set()
  for case in X.all_cases():
    got = X.instances(case)
    assert got <= universe, (case, got - universe)
    reached |= got
  missing = sorted(map(str, universe - reached))
  assert not missing, f"{len(missing)} instances no case runs, e.g. {missing[:8]}"


def test_every_row_count_group_alone_reaches_every_instance():
  """(the other groups add launch shapes, not instances)"""
  assert {i for c in X.cases("every_n") for i in X.instances(c)} == X.universe()
  by_n = {}
  for c in X.cases("every_n"):
    by_n.setdefault((c.kernel, c.rule, c.n), set()).add((c.masks, c.f))
  for n in range(1, X.BM_MAX_ROWS + 1):
    assert {s for s, _ in by_n[(X.MIX_ROWS, None, n)]} == set(X.mask_sets(X.MIX_ROWS, n))
    if n <= X.K_MIXED_MAX_ROWS:
      assert {s for s, _ in by_n[(X.FUSED, X.MEDIAN, n)]} == set(X.mask_sets(X.FUSED, n))
      # the rule's f on the masks of each mixing f: 0, 1 and (n - 1) // 2 wherever the rule admits them
      for mf in nc.f_values(n):
        fs = {f for s, f in by_n[(X.FUSED, X.TRMEAN, n)] if s == f"nnm-f{mf}"}
        assert {f for f in (0, 1, (n - 1) // 2) if n >= 2 * f + 1} <= fs, (n, mf, fs)
        if n >= 4:
          assert fs - {mf}, (n, mf)
      assert any(s == "random" for s, _ in by_n[(X.FUSED, X.TRMEAN, n)])
  assert X.BM_MAX_ROWS not in [c.n for c in X.cases("every_n") if c.kernel == X.FUSED]


def test_launch_shapes_of_the_short_lengths():
  def one(kernel, n, d, off):
    (l,) = X.launches(X.Case("t", kernel, X.MEDIAN if kernel == X.FUSED else None, n, d, off, 0, 0, "onehot", 0))
    return l
  # d = 3 and d = 1 at 16-byte pointers: the VEC 4 instance, the tail group alone (Tail::kRides never narrows)
  for d in (1, 3):
    l = one(X.MIX_ROWS, 11, d, 0)
    assert (l.vec, l.nvec, l.tail, l.groups, l.grid, l.tail_shares_wave) == (4, 0, d, 1, 1, False)
    l = one(X.FUSED, 11, d, 0)
    assert (l.vec, l.nvec, l.tail, l.groups) == (2, d // 2, d % 2, d // 2 + 1)
  # d = 1027: at VEC 4 the body is exactly one workgroup and the tail group is lane 0's second trip; at VEC 2 the tail
  # group shares a wave with body groups; at VEC 1 there is no tail
  l = one(X.MIX_ROWS, 11, 1027, 0)
  assert (l.vec, l.nvec, l.tail, l.grid, l.groups, l.tail_shares_wave) == (4, 256, 3, 1, 257, False)
  assert l.groups > l.grid * X.K_COL_BLOCK
  for kernel, off in ((X.MIX_ROWS, 8), (X.FUSED, 0), (X.MIX_ROWS, 0)):
    l = one(kernel, 29, 1027, off)
    assert (l.vec, l.nvec, l.tail, l.grid, l.tail_shares_wave) == (2, 513, 1, 3, True)
  l = one(X.MIX_ROWS, 11, 1027, 4)
  assert (l.vec, l.nvec, l.tail, l.groups) == (1, 1027, 0, 1027)
  # 259 and 3074: a tail in a wave with body groups at VEC 4; several workgroups
  l = one(X.MIX_ROWS, 11, 259, 0)
  assert (l.vec, l.nvec, l.tail, l.tail_shares_wave) == (4, 64, 3, False)
  l = one(X.MIX_ROWS, 11, 3074, 0)
  assert (l.vec, l.nvec, l.tail, l.grid, l.tail_shares_wave) == (4, 768, 2, 3, False)
  l = one(X.MIX_ROWS, 11, 3074, 4)
  assert (l.vec, l.grid) == (1, 13)


def test_every_group_reaches_what_it_promises():
  flagship = X.cases("flagship")
  assert {c.n for c in flagship if c.kernel == X.MIX_ROWS} == set(X.FLAGSHIP)
  assert {c.n for c in flagship if c.kernel == X.FUSED} == set(X.FLAGSHIP) - {64}
  assert {c.d for c in flagship} == {1, 259, 3074} and {c.d for c in X.cases("every_n")} == {3, 1027}
  # output-forced: the width follows the outputs, below what the inputs allow
  forced = X.cases("out_forced")
  assert {(c.kernel, c.n) for c in forced} == {(X.MIX_ROWS, 11), (X.MIX_ROWS, 29), (X.FUSED, 11)}
  for c in forced:
    (l,) = X.launches(c)
    assert c.offset == 0 and l.vec == {4: 1, 8: 2}[c.out_offset], c
    # 4 bytes off: narrower than the inputs allow everywhere; 8 bytes off: where the instance has a 16-byte width
    assert l.vec < X.input_width(c) or (c.out_offset == 8 and X.input_width(c) == 2), c
  narrowed = {(c.kernel, c.n, X.launches(c)[0].vec) for c in forced if X.launches(c)[0].vec < X.input_width(c)}
  assert narrowed == {(X.MIX_ROWS, 11, 1), (X.MIX_ROWS, 11, 2), (X.MIX_ROWS, 29, 1), (X.FUSED, 11, 1)}
  # pieces: VEC 2 and VEC 1 pieces from a call whose pointers are all 16-byte aligned
  pieces = X.cases("pieces")
  assert {(c.kernel, c.rule) for c in pieces} == {(X.MIX_ROWS, None), (X.FUSED, X.MEDIAN), (X.FUSED, X.TRMEAN)}
  for c in pieces:
    assert c.n == 11 and c.offset == 0 and c.out_offset == 0
    ls = X.launches(c)
    if c.piece == 1002:
      assert [(l.lo, l.vec) for l in ls] == [(0, min(4, X.input_width(c))), (1002, 2), (2004, min(4, X.input_width(c))),
                                             (3006, 2)]
      assert ls[-1].count == 68
    else:
      assert c.piece == 7 and len(ls) == 9 and ls[1].vec == 1 and ls[2].vec == 2
      assert {l.vec for l in ls[1:]} >= {1, 2}
  # the long case: VEC 1, a lane with two body trips, every special column of the trip boundary inside
  long = X.cases("long")
  assert {(c.kernel, c.rule) for c in long} == {(X.MIX_ROWS, None), (X.FUSED, X.MEDIAN), (X.FUSED, X.TRMEAN)}
  for c in long:
    (l,) = X.launches(c)
    assert (c.n, c.offset, c.d) == (3, 4, 16384 * 256 + 259) and l.vec == 1 and l.tail == 0
    assert l.grid == X.K_COL_MAX_BLOCKS and l.body_trips == 2 and l.nvec > l.grid * X.K_COL_BLOCK
  for c in X.all_cases():
    if c.group != "long":
      assert all(l.body_trips <= 1 for l in X.launches(c))


# ---------------------------------------------------------------------------------------------------------------------
# The inputs

def _lane_positions(cols):
  return {c % 4 for c in cols}


@pytest.mark.parametrize("d", [1027, 3074, X.D_LONG])
def test_special_columns_land_where_they_are_claimed(d):
  for n in ((3,) if d == X.D_LONG else (2, 3, 11, 29, 36, 64)):
    special = X.special_columns(n, d)
    for kind in X.KINDS:
      cols = X.columns_of_kind(n, d, kind)
      k = X.KINDS.index(kind)
      # column 0 (the first kind) and the start of the row
      assert special[0] == 0 and k * 16 in cols
      # each kind in every lane position of a 16-byte group: at the start, in the middle of the first wave of 16-byte
      # groups (lanes 32 ..) and over the last columns
      assert _lane_positions(c for c in cols if c < 128) == {0, 1, 2, 3}, (n, d, kind)
      mid = [c for c in cols if 128 <= c < 256]
      assert _lane_positions(mid) == {0, 1, 2, 3} and all(32 <= c // 4 < 64 for c in mid), (n, d, kind)
      assert _lane_positions(c for c in cols if c >= d - X.END) == {0, 1, 2, 3}, (n, d, kind)
    # the trailing columns, and special columns in the last body group at VEC 4 and at VEC 2
    assert {d - 1, d - 2, d - 3} <= set(special)
    for vec in (4, 2):
      body_end = d - d % vec
      assert any(c in special for c in range(body_end - vec, body_end)), (n, d, vec)
    # at 8-byte columns the tail group of d = 1027 sits in a wave whose body groups hold special columns too
    if d == 1027:
      (l,) = X.launches(X.Case("t", X.MIX_ROWS, None, n, d, 8, 0, 0, "onehot", 0))
      wave_first = l.nvec // X.WAVE * X.WAVE * l.vec
      assert l.tail_shares_wave and d - 1 in special and any(c in special for c in range(wave_first, l.nvec * l.vec))
    # at least one whole wave, at every width, holds no special value: columns 256 .. 511
    assert X.SITE <= 128 and X.site_starts(d)[:2] == [0, 128]
    assert X.ordinary_mask(n, d)[256:512].all()
    assert np.isfinite(X.values(n, d)[:, 256:512]).all()
    assert (np.abs(X.values(n, d)[:, 256:512]) > 2.0 ** -100).all()
  if d == X.D_LONG:
    special = X.special_columns(3, d)
    assert any(c < X.TRIP for c in special if c > 256) and any(X.TRIP <= c < X.TRIP + 64 for c in special)
    assert all(c >= X.TRIP for c in range(d - X.END, d))          # the end of the row is on the second trip


def test_trailing_columns_hold_the_kinds():
  """The trailing d % 4 columns of d = 3 and d = 1027 (the tail group of the VEC 4 instance) hold six kinds between
  them at every n, the one trailing column of the VEC 2 instances two, and every kind over seven consecutive n."""
  seen4, seen2 = set(), set()
  for n in range(1, X.BM_MAX_ROWS + 1):
    tails = {X.special_columns(n, d)[c] for d in (3, 1027) for c in range(d - 3, d)}
    assert len(tails) == 6, n
    two = {X.special_columns(n, d)[d - 1] for d in (3, 1027)}
    assert len(two) == 2
    seen4 |= tails
    seen2 |= two
    if n >= 7:
      assert len(seen2) == X.NK
  assert len(seen4) == X.NK
  # d = 3 is the tail group alone: all three columns special; d = 1: one
  assert len(X.special_columns(11, 3)) == 3 and len(X.special_columns(11, 1)) == 1


def test_special_values_are_what_they_are_called():
  for n, d in ((2, 1027), (11, 1027), (36, 3074), (64, 1027)):
    vals = X.values(n, d)
    for c in X.columns_of_kind(n, d, "nan"):
      assert np.isnan(vals[:, c]).sum() == 1 and np.isnan(vals[c % n, c])
    for c in X.columns_of_kind(n, d, "inf"):
      assert vals[c % n, c] == np.inf and vals[(c + 1) % n, c] == -np.inf and np.isinf(vals[:, c]).sum() == 2
    for c in X.columns_of_kind(n, d, "zeros"):
      assert not vals[:, c].any() and np.signbit(vals[1::2, c]).all() and not np.signbit(vals[::2, c]).any()
    for c in X.columns_of_kind(n, d, "cancel"):
      a, b = c % n, (c + 1) % n
      assert vals[a, c] == -vals[b, c] != 0 and np.count_nonzero(vals[:, c]) == 2 and not np.signbit(vals[:, c]).all()
    for c in X.columns_of_kind(n, d, "tiny"):
      assert (np.abs(vals[:, c]) < 2.0 ** -120).all() and (np.abs(vals[:, c]) > 0).all()
    for c in X.columns_of_kind(n, d, "ties"):
      k = vals[:, c].astype(np.float64) * 2.0 ** 149
      assert (k == np.round(k)).all() and (k >= 1).all() and (k <= 12).all()
    for c in X.columns_of_kind(n, d, "huge"):
      assert np.isfinite(vals[:, c]).all() and (vals[:, c] >= 2.7e38).all()
      with np.errstate(over="ignore"):
        assert np.isinf(vals[0, c] + vals[1, c])                  # finite on entry, inf in the accumulator


def test_mask_sets_include_and_exclude_every_bit_position():
  for kernel in (X.MIX_ROWS, X.FUSED):
    for n in range(1, (X.BM_MAX_ROWS if kernel == X.MIX_ROWS else X.K_MIXED_MAX_ROWS) + 1):
      sets = X.mask_sets(kernel, n)
      for j in range(n):
        for name in ("onehot", "complement"):
          words = sets[name]
          assert any((w >> j) & 1 for w in words) and any(not (w >> j) & 1 for w in words) or n == 1, (n, name, j)
        assert any((w >> j) & 1 for w in sets["onehot"]) and any(not (w >> j) & 1 for w in sets["complement"])
      assert all(w < 1 << n for name in ("onehot", "complement") for w in sets[name])
      assert sets["random"][-1] & ((1 << n) - 1) == 0 and (n == 64 or sets["random"][0] >> n)   # an empty mask; bits >= n set
      if kernel == X.FUSED:
        assert all(len(words) == n for words in sets.values())
        counts = {bin(w & ((1 << n) - 1)).count("1") for w in sets["random"]}
        assert n < 4 or len(counts) >= 3                                             # the counts differ per row
      else:
        assert n < 2 or len(sets["buckets"]) == (n + 1) // 2 < n or n == 2
      for f in nc.f_values(n):
        assert all(bin(w).count("1") == n - f for w in sets[f"nnm-f{f}"])
  assert len(X.mask_sets(X.MIX_ROWS, 3)["wide"]) == 64 and len(X.mask_sets(X.MIX_ROWS, 64)["single"]) == 1
  # across the word boundary: bits 31 and 32 each included and excluded at every N > 32
  for n in range(33, 65):
    for name in ("onehot", "complement"):
      words = X.mask_sets(X.MIX_ROWS, n)[name]
      assert {(w >> 31) & 3 for w in words} >= {1, 2} if name == "onehot" else {(w >> 31) & 3 for w in words} >= {1, 2, 3}


@pytest.mark.parametrize("n", [1, 2, 3, 11, 25, 28, 29, 36, 64])
def test_reference_properties_of_the_inputs(n):
  """On the numpy reference alone: one-hot masks give x + 0; no mixed value is a negative zero (so the median needs no
  zero-sign exemption); the empty mask gives NaN everywhere; the float32 loop stays within the float64 bound on the
  ordinary columns; a NaN row outside a mask does not reach the output."""
  d = 1027
  vals = X.values(n, d)
  ordinary = X.ordinary_mask(n, d)
  for kernel in ((X.MIX_ROWS, X.FUSED) if n <= X.K_MIXED_MAX_ROWS else (X.MIX_ROWS,)):
    for name, words in X.mask_sets(kernel, n).items():
      mixed = X.mixed_reference(kernel, n, d, name)
      assert not (np.signbit(mixed) & (mixed == 0)).any(), (n, name)
      y64, bound = nc.mix_reference64(list(vals[:, ordinary]), [w & ((1 << n) - 1) for w in words])
      for r, w in enumerate(words):
        if w & ((1 << n) - 1):
          assert (np.abs(mixed[r, ordinary].astype(np.float64) - y64[r]) <= bound[r]).all(), (n, name, r)
        else:
          assert np.isnan(mixed[r]).all()
      if name == "onehot":
        assert nc.same_bits(mixed, vals + np.float32(0))
  nan_cols = X.columns_of_kind(n, d, "nan")
  onehot = X.mixed_reference(X.MIX_ROWS, n, d, "onehot")
  for c in nan_cols:
    assert np.isnan(onehot[:, c]).sum() == 1                       # included by one mask, excluded by the others


def test_no_mixed_value_is_a_negative_zero_at_any_row_count():
  for kernel, top in ((X.MIX_ROWS, X.BM_MAX_ROWS), (X.FUSED, X.K_MIXED_MAX_ROWS)):
    for n in range(1, top + 1):
      for d in X.D_EVERY:
        for name in X.mask_sets(kernel, n):
          mixed = X.mixed_reference(kernel, n, d, name)
          assert not (np.signbit(mixed) & (mixed == 0)).any(), (kernel, n, d, name)


# ---------------------------------------------------------------------------------------------------------------------
# Three deliberate defects of mix_one, as numpy twins: the case lists tell each from the reference

def _differs(a, b):
  return X.first_difference(a.ravel(), b.ravel()) is not None


@pytest.mark.parametrize("n", [2, 3, 11, 29, 36, 64])
def test_twin_keep_dropped_in_the_non_finite_path(n):
  """Every row count >= 2 at d = 1027 (at d = 3 only where one of the three columns holds a NaN or an infinity): a
  one-hot mask that excludes the NaN row gives NaN."""
  d = 1027
  vals = X.values(n, d)
  for vec in (1, 2, 4):
    for name in ("onehot", "complement", "nnm-f1"):
      words = X.mask_sets(X.MIX_ROWS, n)[name]
      want = X.mixed_reference(X.MIX_ROWS, n, d, name)
      assert _differs(X.broken_keep_dropped(vals, words, vec), want), (n, d, vec, name)


@pytest.mark.parametrize("n", [1, 11, 32, 33, 36, 64])
def test_twin_high_word_read_for_the_low_rows(n):
  """Every row count: up to 32 rows nothing is added any more; beyond, rows j < 32 follow bit 32 + j."""
  d = 1027
  vals = X.values(n, d)
  for name in ("onehot", "complement", "nnm-f1" if n > 32 else "nnm-f0"):
    if n == 1 and name == "complement":                       # (the empty mask: NaN either way)
      continue
    words = X.mask_sets(X.MIX_ROWS, n)[name]
    assert _differs(X.broken_hi_word(vals, words), X.mixed_reference(X.MIX_ROWS, n, d, name)), (n, name)


@pytest.mark.parametrize("n", [11, 25, 36, 64])
def test_twin_division_always_by_the_reciprocal(n):
  """div_small_int taken unconditionally shows in the subnormal quotients of the tiny and the tie columns (for one: a
  mask of 6, 10, 12, ... rows whose sum is an odd multiple of half the count, in units of 2^-149), for bm_mix_rows'
  mask sets and for the fused kernels' alike."""
  d = 1027
  vals = X.values(n, d)
  cols = X.columns_of_kind(n, d, "ties") + X.columns_of_kind(n, d, "tiny")
  hits = 0
  for kernel in ((X.MIX_ROWS, X.FUSED) if n <= X.K_MIXED_MAX_ROWS else (X.MIX_ROWS,)):
    per_kernel = 0
    for name, words in X.mask_sets(kernel, n).items():
      want = X.mixed_reference(kernel, n, d, name)[:, cols]
      got = X.broken_division(vals, words, cols)
      per_kernel += int((~np.isnan(want) & (got.view(np.uint32) != want.view(np.uint32))).sum())
    assert per_kernel > 0, (n, kernel)
    hits += per_kernel
  assert hits > 0


def test_exact_twin_of_the_corrected_quotient():
  """div_small_int_exact is the division itself in the normal range, and rounds 9 / 6 units of 2^-149 down to 1 where
  the division's tie goes to the even 2."""
  rng = np.random.default_rng(1)
  for x in rng.standard_normal(200).astype(np.float32):
    for m in (3, 6, 7, 11, 25, 64):
      assert np.float32(X.div_small_int_exact(x, m)) == x / np.float32(m)
  unit = 2.0 ** -149
  assert np.float32(9 * unit) / np.float32(6) == np.float32(2 * unit)
  assert X.div_small_int_exact(np.float32(9 * unit), 6) == 1 * unit


def _ascending_sum(mixed, f=0):
  """The float32 sum of the ranks f .. n - f - 1 of every column in ascending order: the trimmed mean's numerator, whose
  bits the comparison with the plain rule on the numpy-mixed rows sees."""
  with np.errstate(all="ignore"):
    srt = np.sort(mixed, axis=0)
    acc = np.zeros(mixed.shape[1], dtype=np.float32)
    for r in range(f, mixed.shape[0] - f):
      acc = acc + srt[r]
  return acc


def test_twins_show_in_the_fused_rules():
  """The fused tests see mixed values only through a rule: each defect still moves the lower median or the ascending
  sum of the mixed values of some case."""
  d = 1027
  vals = X.values(11, d)
  for name in ("onehot", "complement", "nnm-f1"):
    words = X.mask_sets(X.FUSED, 11)[name]
    want = X.mixed_reference(X.FUSED, 11, d, name)
    for broken in (X.broken_keep_dropped(vals, words, 2), X.broken_hi_word(vals, words)):
      assert X.first_difference(X.lower_median(broken), X.lower_median(want)) is not None, name
      assert X.first_difference(_ascending_sum(broken), _ascending_sum(want)) is not None, name
  for n, name, rule, f in ((12, "nnm-f0", X.MEDIAN, 0), (36, "nnm-f0", X.MEDIAN, 0), (11, "complement", X.TRMEAN, 2),
                           (25, "nnm-f1", X.TRMEAN, 0)):
    assert (name, f) in X.runs(X.FUSED, rule, n)
    cols = X.columns_of_kind(n, d, "ties") + X.columns_of_kind(n, d, "tiny")
    want = X.mixed_reference(X.FUSED, n, d, name)[:, cols]
    broken = X.broken_division(X.values(n, d), X.mask_sets(X.FUSED, n)[name], cols)
    seen = X.lower_median if rule == X.MEDIAN else (lambda m: _ascending_sum(m, f))
    assert X.first_difference(seen(broken), seen(want)) is not None, (n, name, rule)
