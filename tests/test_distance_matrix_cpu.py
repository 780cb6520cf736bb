"""The mirror of tests/distance_matrix.py against the sources of the distance pass, and the case lists of
tests/test_gpu_distance_matrix.py against every instance those sources can reach (no GPU needed).

Parsed out of csrc/gram_bf16.hip, csrc/pairwise.hip and csrc/api.cpp: the BM_B3_CASE list, the plane threshold,
kB3Chunk / kB3Waves / kB3MaxBlocks, the NSETS and b3_workgroups_per_cu expressions and the probe rows of the centre
(evaluated by the C expression evaluator of tests/test_instance_matrix_cpu.py), the grid rule, the slice rule of
gram_finish, pair_geometry's candidate table with its thread and LDS limits, and the gate's default tau.  A K or a
candidate added to the sources without a case that runs it fails here."""

import pathlib
import re

import pytest

from tests import distance_matrix as D
from tests.test_instance_matrix_cpu import c_eval

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "byzantinemomentum_amd" / "csrc"
CUS = 256


def _int(text, name):
  m = re.search(r"constexpr int " + name + r"\s*=\s*([^;]+);", text)
  assert m, name
  return c_eval(m.group(1), {})


class Source:
  def __init__(self):
    gram = (CSRC / "gram_bf16.hip").read_text()
    pair = (CSRC / "pairwise.hip").read_text()
    api = (CSRC / "api.cpp").read_text()
    self.max_rows = int(re.search(r"#define\s+BM_MAX_ROWS\s+(\d+)", (ROOT / "include" / "bm_gar.h").read_text()).group(1))
    self.b3_cases = tuple(int(k) for k in re.findall(r"BM_B3_CASE\((\d+)\)", gram))
    assert "const int K = (n + 3) / 4;" in gram
    self.plane_threshold = 1 << int(re.search(
      r"planes = \(d_total >= \(\(int64_t\)1 << (\d+)\)\) \? 2 : 3;", gram).group(1))
    self.chunk, self.waves, self.max_blocks = (_int(gram, k) for k in ("kB3Chunk", "kB3Waves", "kB3MaxBlocks"))
    self.nsets = re.search(r"static constexpr int NSETS = ([^;]+);", gram).group(1)
    self.wpc = re.search(r"constexpr int b3_workgroups_per_cu\(int K, int NPL\) \{\s*return ([^;]+);", gram).group(1)
    # the grid rule of gram3_partials and the entry condition of the steady-state loop, as the mirror restates them
    for line in ("const int64_t chunks = (d + kB3Chunk - 1) / kB3Chunk;",
                 "int blocks = compute_units() * b3_workgroups_per_cu(K, planes);",
                 "if (blocks > kB3MaxBlocks) blocks = kB3MaxBlocks;",
                 "const int64_t need = (chunks + kB3Waves - 1) / kB3Waves;",
                 "if (blocks > need) blocks = (int)(need > 0 ? need : 1);",
                 "const int64_t full = d / kB3Chunk;",
                 "if (steady != 0 && c + (2 * NSETS - 1) * nw < full) {",
                 "} while (c + (2 * NSETS - 1) * nw < full);"):
      assert line in gram, line
    self.probes = re.search(r"constexpr int kPa = ([^,]+), kPb = ([^,]+), kPc = ([^;]+);", gram).groups()
    self.probe_lanes = ("x", re.search(r"const int src_b = ([^;]+);", gram).group(1),
                        re.search(r"const int src_c = ([^;]+);", gram).group(1))
    # the slice rule of gram_finish
    self.slices_max = _int(gram, "kGramSlicesMax")
    finish = gram[gram.index("int gram_finish("):]
    assert "const int chunks = (int)((per_block + 63) / 64);" in finish
    self.slice_workgroups = int(re.search(r"int slices = (\d+) / chunks;", finish).group(1))
    assert "if (slices > kGramSlicesMax) slices = kGramSlicesMax;" in finish
    m = re.search(r"if \(slices > blocks / (\d+)\) slices = blocks / (\d+);", finish)
    assert m.group(1) == m.group(2)
    self.slice_min_blocks = int(m.group(1))
    assert "if (slices < 1 || blocks + slices > kB3MaxBlocks) slices = 1;" in finish
    # pair_geometry
    table = re.search(r"const int cand\[(\d+)\]\[2\] = \{(.+?)\};", pair)
    self.cand = tuple((int(a), int(b)) for a, b in re.findall(r"\{(\d+), (\d+)\}", table.group(2)))
    assert len(self.cand) == int(table.group(1))
    self.pair_max_threads = _int(pair, "kPairMaxThreads")
    self.pair_lds_limit = c_eval(re.search(r"if \(2 \* tile_bytes > ([^)]+)\) continue;", pair).group(1), {})
    self.dma_block, self.dma_pitch = _int(pair, "kDmaBlock"), _int(pair, "kDmaPitch")
    self.pair_grid_max = c_eval(re.search(r"static int pair_grid_blocks[^}]+?int blocks = ([^;]+);", pair).group(1), {})
    self.tau = float(re.search(r'env_double\("BM_PAIR_TAU", ([^)]+)\)', api).group(1))

  def probe_rows(self, n):
    K = (n + 3) // 4
    rows = []
    for k_expr, lane_expr in zip(self.probes, self.probe_lanes):
      lane = c_eval(lane_expr, {"K": K, "n": n, "x": 0})  # lane (rho = lane >> 4, x) holds row 4 k + rho
      rows.append(4 * c_eval(k_expr, {"K": K}) + (lane >> 4))
    return tuple(rows)


@pytest.fixture(scope="module")
def src():
  return Source()


@pytest.fixture(scope="module")
def reached():
  out = {}
  for group in D.GROUPS:
    got = set()
    for case in D.cases(group, CUS):
      got |= D.instances(case, CUS)
    out[group] = got
  return out


def test_mirror_constants_match_the_sources(src):
  assert src.max_rows == D.BM_MAX_ROWS
  assert src.b3_cases == D.B3_CASES and src.b3_cases == tuple(range(1, (src.max_rows + 3) // 4 + 1))
  assert src.plane_threshold == D.PLANE_THRESHOLD
  assert (src.chunk, src.waves, src.max_blocks) == (D.K_B3_CHUNK, D.K_B3_WAVES, D.K_B3_MAX_BLOCKS)
  assert (src.slices_max, src.slice_workgroups, src.slice_min_blocks) == (
    D.K_GRAM_SLICES_MAX, D.GRAM_SLICE_WORKGROUPS, D.GRAM_SLICE_MIN_BLOCKS)
  assert src.cand == D.PAIR_CAND
  assert (src.pair_max_threads, src.pair_lds_limit) == (D.K_PAIR_MAX_THREADS, D.PAIR_LDS_LIMIT)
  assert (src.dma_block, src.dma_pitch, src.pair_grid_max) == (D.K_DMA_BLOCK, D.K_DMA_PITCH, D.PAIR_GRID_MAX)
  assert src.tau == D.PAIR_TAU


def test_mirror_expressions_match_the_sources(src):
  for K in src.b3_cases:
    for npl in (2, 3):
      env = {"K": K, "NPL": npl}
      assert c_eval(src.nsets, env) == D.b3_nsets(K, npl), env
      assert c_eval(src.wpc, env) == D.b3_workgroups_per_cu(K, npl), env
  for n in range(1, src.max_rows + 1):
    assert src.probe_rows(n) == D.probe_rows(n), n
    assert all(r < n for r in D.probe_rows(n)), n


def test_pair_geometry_mirror():
  """What pairwise.hip documents of its geometry: row_bytes in {256, 512, 1024}, at most 512 lanes, two tile buffers
  within 32 KB, one 16-lane unit per 16 pair tiles and strip."""
  for n in range(1, D.BM_MAX_ROWS + 1):
    g = D.pair_geometry(n)
    assert (g.strips, g.slots) in D.PAIR_CAND and g.row_bytes in (256, 512, 1024), g
    assert g.threads <= D.K_PAIR_MAX_THREADS and g.threads % 64 == 0 and 16 * g.ut * g.strips <= g.threads, g
    # (61-64 rows: no candidate's two buffers stay within 32 KB, the rule falls back to its first, narrowest one)
    assert 2 * g.nb * D.K_DMA_PITCH <= D.PAIR_LDS_LIMIT or (g.ng == 16 and (g.strips, g.slots) == D.PAIR_CAND[0]), g
    assert g.width == g.row_bytes // 4, g
    assert g == D.pair_geometry(4 * g.ng)._replace(n=n)  # the geometry follows the number of 4-row groups alone


def test_steady_lengths(src):
  """At steady_length every wave of the instance enters the steady-state loop, some go on in the generic loop, the last
  chunk is ragged; 64 coordinates less than the bare minimum and the last wave no longer enters."""
  for cus in (CUS, 304, 64):
    for K in src.b3_cases:
      for npl in (3, 2):
        d = D.steady_length(K, npl, cus)
        assert d < D.PLANE_THRESHOLD and d % D.K_B3_CHUNK != 0
        in_steady, in_generic, nw = D.gram_loops(4 * K, d, npl, True, cus)
        assert in_steady == nw and 0 < in_generic < nw, (cus, K, npl)
        short = d - (D.K_B3_CHUNK * 7 + 5) - D.K_B3_CHUNK
        assert D.gram_loops(4 * K, short, npl, True, cus)[0] == nw - 1, (cus, K, npl)
        assert D.gram_loops(4 * K, d, npl, False, cus)[0] == 0 and D.gram_loops(4 * K, d, npl, True, cus, 0)[0] == 0


def test_case_lists_reach_every_gram_instance(src, reached):
  everything = set().union(*reached.values())
  for K in src.b3_cases:
    for npl in (3, 2):
      for aligned in (True, False):
        assert ("gram", K, npl, aligned, "generic") in everything, (K, npl, aligned)
      assert ("gram", K, npl, True, "steady") in reached["steady"], (K, npl)
      assert ("gram", K, npl, True, "steady") not in reached["knob_steady"], (K, npl)
      assert ("gram", K, npl, True, "generic") in reached["knob_steady"], (K, npl)
  # within one K the four row counts 4K-3 .. 4K differ in the padded rows and the probes: all 64 run, both forms
  for off in (0, 4):
    assert {c.n for c in D.cases("rows3", CUS) if c.offset == off} == set(range(1, src.max_rows + 1))
  two = {c.n for c in D.cases("planes2", CUS)}
  assert two == {4 * K for K in src.b3_cases} | {4 * K - 3 for K in src.b3_cases}
  assert min(c.d for c in D.cases("planes2", CUS)) >= 65536  # (the 1e-6 bar of two planes needs the length)
  assert all(c.d_total >= src.plane_threshold for c in D.cases("planes2", CUS))


def test_case_lists_reach_every_direct_geometry(src, reached):
  selected = {(g.strips, g.slots) for g in map(D.pair_geometry, range(1, src.max_rows + 1))}
  for form, group in (("whole", "direct_whole"), ("gated", "gated"), ("gated", "rank_gated")):
    got = {(i[1], i[2]) for i in reached[group] if i[0] == "direct" and i[4] == form}
    assert got == selected, (form, group, selected - got)
  for aligned in (True, False):
    assert {(i[1], i[2]) for i in reached["direct_whole"] if i[3] == aligned} == selected
    assert any(i[0] == "direct" and i[3] == aligned for i in reached["gated"])
  assert all(i[0] == "direct" and i[4] == "whole" for i in reached["direct_whole"])
  # every sub-stack size the gate can list: k = 2 .. n - 2 through a clique with at most one probe row in it, n - 1
  # and n through near-duplicate pairs, the last two at the long length too (five rows cannot all be listed:
  # distance_matrix.expected_listed)
  listed = {}
  for case in D.cases("gated", CUS):
    rows = D.expected_listed(case)
    if rows and case.offset == 0:
      listed.setdefault((case.n, case.d), set()).add(len(rows))
  for n in D.GATED_N:
    top = n - 1 if n == 5 else n
    assert listed[(n, D.D_GATED)] == set(range(2, top + 1)), (n, sorted(listed[(n, D.D_GATED)]))
    assert {2, top - 1 if n > 5 else top, top} <= listed[(n, D.D_GATED_LONG)], (n, sorted(listed[(n, D.D_GATED_LONG)]))
  for case in D.cases("gated", CUS):  # the groups of a pairs stack keep the probes apart wherever all rows are listed
    if case.kind[0] == "pairs":
      groups = D.near_groups(case)
      assert sorted(r for g in groups for r in g) == list(range(case.kind[1])) and all(len(g) in (2, 3) for g in groups)
  # one tile width each with three trips through both buffers
  widths = {D.pair_geometry(n).width for n in range(1, src.max_rows + 1)}
  long = D.direct_long_cases("direct_whole", (("BM_PAIR_MODE", 1),))
  assert {D.pair_geometry(c.n).width for c in long} == widths == {64, 128, 256}
  for c in long:
    w = D.pair_geometry(c.n).width
    assert c.d > 2 * 1024 * w + 7 and c.d % w != 0 and D.pair_grid(c.n, c.d) == D.PAIR_GRID_MAX


def test_case_lists_reach_the_slice_counts(reached):
  assert {i[1] for i in reached["slices"] if i[0] == "gram_reduce"} == {1, 2, D.K_GRAM_SLICES_MAX}
  assert any(i == ("gram_reduce", 1) for i in reached["rows3"])


def test_case_generators():
  for n in range(1, D.BM_MAX_ROWS + 1):
    assert D.aliases(n) == 0 if n < 3 else 2 <= D.aliases(n) < n
    shape = D.rank_shape(n)
    if shape is not None:
      f, m = shape
      assert n >= 4 * f + 3 and m == n - f - 2 and m >= 1
    for k in range(2, n + 1):
      for where in D.PLACEMENTS:
        rows = D.clique_rows(n, k, where)
        assert len(set(rows)) == k and list(rows) == sorted(rows) and 0 <= rows[0] and rows[-1] < n
  assert D.rank_shape(1) is None and D.rank_shape(2) is None
  coords = D.nonfinite_coordinates(D.NONFINITE_D)
  assert sorted(c % 64 for c in coords[:-1]) == list(range(64)) and coords[-1] >= D.NONFINITE_D // 64 * 64
  assert max(coords) < D.NONFINITE_D
  keys = [D.case_key(c) for g in D.GROUPS for c in D.cases(g, CUS) if g not in ("knob_steady", "direct_whole",
                                                                               "rank_plain", "rank_gated")]
  assert len(keys) == len(set(keys))
