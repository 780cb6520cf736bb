"""The instance mirror of tests/instance_matrix.py against the sources, and the case lists of
tests/test_gpu_instance_matrix.py against every instance the sources can reach (no GPU needed).

Parsed out of csrc/: the BM_BULYAN_CASE table, bm_bulyan_pass2_eval_supported, bm_colwise_eval_supported, the order_pair
buckets, kBurstMaxRows / kBurstMaxRowsClosest, the burst condition, BM_MAX_ROWS and every launcher's kMaxVec expression
(evaluated by a small C expression evaluator).  An instance added to the sources without a case that runs it fails
here."""

import pathlib
import re

import pytest

from tests import instance_matrix as M

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "byzantinemomentum_amd" / "csrc"
HEADER = ROOT / "include" / "bm_gar.h"


# ---------------------------------------------------------------------------------------------------------------------
# A C expression evaluator: integers, names, ! && || == != < <= > >= + - * / ( ) and ?:

_TOKEN = re.compile(r"\s*(\d+|[A-Za-z_]\w*|&&|\|\||==|!=|<=|>=|[-+*/()<>!?:])")


def c_eval(expr, env):
  toks, pos = [], 0
  expr = expr.strip()
  while pos < len(expr):
    m = _TOKEN.match(expr, pos)
    if not m:
      raise ValueError(f"cannot parse {expr[pos:]!r}")
    toks.append(m.group(1))
    pos = m.end()
  toks.append(None)
  i = 0

  def peek():
    return toks[i]

  def take(want=None):
    nonlocal i
    t = toks[i]
    if want is not None and t != want:
      raise ValueError(f"expected {want!r}, got {t!r} in {expr!r}")
    i += 1
    return t

  def primary():
    t = take()
    if t == "(":
      v = ternary()
      take(")")
      return v
    if t == "!":
      return int(not primary())
    if t == "-":
      return -primary()
    if t.isdigit():
      return int(t)
    if t == "true" or t == "false":
      return int(t == "true")
    return int(env[t])

  def binary(level):
    ops = (("||",), ("&&",), ("==", "!="), ("<", "<=", ">", ">="), ("+", "-"), ("*", "/"))
    if level == len(ops):
      return primary()
    v = binary(level + 1)
    while peek() in ops[level]:
      op = take()
      w = binary(level + 1)
      v = {"||": lambda: int(bool(v) or bool(w)), "&&": lambda: int(bool(v) and bool(w)), "==": lambda: int(v == w),
           "!=": lambda: int(v != w), "<": lambda: int(v < w), "<=": lambda: int(v <= w), ">": lambda: int(v > w),
           ">=": lambda: int(v >= w), "+": lambda: v + w, "-": lambda: v - w, "*": lambda: v * w,
           "/": lambda: int(v / w)}[op]()
    return v

  def ternary():
    c = binary(0)
    if peek() == "?":
      take("?")
      a = ternary()
      take(":")
      b = ternary()
      return a if c else b
    return c

  v = ternary()
  if peek() is not None:
    raise ValueError(f"trailing tokens in {expr!r}")
  return v


def test_c_eval():
  env = {"N": 30, "kClosest": 1}
  assert c_eval("(N <= 28) ? 4 : ((!kClosest && N <= 52) ? 4 : (N <= (kClosest ? 54 : 56) ? 2 : 1))", env) == 2
  assert c_eval("1 + 2 * 3 == 7 && !(4 < 3)", {}) == 1


# ---------------------------------------------------------------------------------------------------------------------
# What the sources say

def _read(name):
  return (CSRC / name).read_text()


def _function(text, name):
  """The text of the function `name` from its signature to the next line that starts a new top-level item."""
  m = re.search(r"\bint\s+" + name + r"\s*\(", text)
  assert m, name
  end = re.search(r"\n}\s*\n", text[m.end():])
  return text[m.start(): m.end() + end.end()]


def _constexpr(body, name):
  m = re.search(r"constexpr\s+(?:int|bool)\s+" + name + r"\s*=\s*([^;]+);", body)
  assert m, name
  return m.group(1)


def _op_values():
  return {k: int(v) for k, v in re.findall(r"\b(BM_OP_[A-Z]+)\s*=\s*(\d+)", HEADER.read_text())}


class Source:
  def __init__(self):
    self.max_rows = int(re.search(r"#define\s+BM_MAX_ROWS\s+(\d+)", HEADER.read_text()).group(1))
    self.ops = _op_values()
    dispatch = _read("colwise_dispatch.h")
    self.burst_rows = int(re.search(r"constexpr int kBurstMaxRows\s*=\s*(\d+);", dispatch).group(1))
    self.burst_rows_closest = int(re.search(r"constexpr int kBurstMaxRowsClosest\s*=\s*(\d+);", dispatch).group(1))
    vec_fn = _function(dispatch, "launch_colwise_vec")
    self.burst_cond = re.search(r"if constexpr \((VEC == 4 && .+)\) \{\n\s*// burst form", vec_fn).group(1)
    n_fn = _function(dispatch, "launch_colwise_n")
    self.colwise_kclosest = _constexpr(n_fn, "kClosest")
    self.colwise_kmaxvec = _constexpr(n_fn, "kMaxVec")
    bulyan = _read("bulyan.hip")
    entry = _function(bulyan, "bm_bulyan_pass2")
    self.bulyan_cases = [(int(a), int(b)) for a, b in re.findall(r"BM_BULYAN_CASE\((\d+),\s*(\d+)\)", entry)]
    self.bulyan_fast_kmaxvec = _constexpr(_function(bulyan, "launch_bulyan_fast"), "kMaxVec")
    self.bulyan_eval_kmaxvec = _constexpr(_function(bulyan, "launch_bulyan_eval"), "kMaxVec")
    self.aksel_kmaxvec = _constexpr(_function(bulyan, "launch_aksel_n"), "kMaxVec")
    sup = _function(bulyan, "bm_bulyan_pass2_eval_supported")
    self.bulyan_eval_shapes = [(int(a), int(b)) for a, b in re.findall(r"n == (\d+) && f == (\d+)", sup)]
    assert "m == n - f - 2" in sup
    search = _read("search_eval.hip")
    self.eval_kmaxvec = _constexpr(_function(search, "launch_eval"), "kMaxVec")
    self.order_pair_kmaxvec = _constexpr(_function(search, "launch_order_pair"), "kMaxVec")
    sup = _function(search, "bm_colwise_eval_supported")
    med_line = re.search(r"if \(op == BM_OP_MEDIAN\) return ([^;]+);", sup).group(1)
    rest = sup[sup.index(med_line) + len(med_line):]
    self.colwise_eval = {"median": tuple(int(x) for x in re.findall(r"n == (\d+)", med_line))}
    others = tuple(int(x) for x in re.findall(r"n == (\d+)", rest))
    for op in ("TRMEAN", "PHOCAS", "MEAMED"):
      assert f"BM_OP_{op}" in rest
      self.colwise_eval[op.lower()] = others
    sup = _function(search, "bm_order_pair_supported")
    self.order_pair_max_h = int(re.search(r"h >= 1 && h <= (\d+)", sup).group(1))
    entry = _function(search, "bm_order_pair")
    self.order_pair_buckets = tuple(int(b) for a, b in re.findall(r"if \(h <= (\d+)\) return launch_order_pair<(\d+)>",
                                                                   entry))
    assert all(int(a) == b for a, b in zip(re.findall(r"if \(h <= (\d+)\)", entry), self.order_pair_buckets))
    self.order_pair_buckets += (int(re.findall(r"\n\s*return launch_order_pair<(\d+)>", entry)[-1]),)

  def env(self, **kw):
    return dict(self.ops, kBurstMaxRows=self.burst_rows, kBurstMaxRowsClosest=self.burst_rows_closest, **kw)

  def colwise_kmax(self, rule, n):
    op = self.ops["BM_OP_" + rule.upper()]
    closest = c_eval(self.colwise_kclosest, self.env(OP=op))
    return c_eval(self.colwise_kmaxvec, self.env(N=n, OP=op, kClosest=closest))

  def burst(self, rule, n, vec):
    return bool(c_eval(self.burst_cond, self.env(N=n, OP=self.ops["BM_OP_" + rule.upper()], VEC=vec)))

  def reachable(self):
    """Every (kernel, N, VEC, form) instance a call can run (the format of instance_matrix.instances)."""
    out = set()
    widths = lambda kmax: [v for v in (4, 2, 1) if v <= kmax]  # noqa: E731  (VEC 2 / 1: rows at 8- / 4-byte offsets)
    for rule in M.RULES:
      for n in range(1, self.max_rows + 1):
        kmax = self.colwise_kmax(rule, n)
        out |= {("colwise", rule, n, v, "plain") for v in widths(kmax)}
        if kmax >= 4 and self.burst(rule, n, 4):
          out.add(("colwise", rule, n, 4, "burst"))
    for n, f in self.bulyan_cases:
      out |= {("bulyan_pass2", (n, f), v, "plain") for v in widths(c_eval(self.bulyan_fast_kmaxvec, {"MMAX": n - f - 2}))}
    out.add(("bulyan_pass2_generic", 0, 1, "plain"))
    for n in range(1, self.max_rows + 1):
      out |= {("aksel_pass1", n, v, "plain") for v in widths(c_eval(self.aksel_kmaxvec, {"N": n}))}
    for rule, ns in self.colwise_eval.items():
      for n in ns:
        out |= {("colwise_eval", rule, n, v, "plain") for v in widths(c_eval(self.eval_kmaxvec, {"N": n}))}
    for n, f in self.bulyan_eval_shapes:
      out |= {("bulyan_pass2_eval", (n, f), v, "plain")
              for v in widths(c_eval(self.bulyan_eval_kmaxvec, {"MMAX": n - f - 2}))}
    for b in self.order_pair_buckets:
      out |= {("order_pair", b, v, "plain") for v in widths(c_eval(self.order_pair_kmaxvec, {"N": b}))}
    return out


@pytest.fixture(scope="module")
def src():
  return Source()


# ---------------------------------------------------------------------------------------------------------------------

def test_mirror_constants_match_the_sources(src):
  assert src.max_rows == M.BM_MAX_ROWS
  assert (src.burst_rows, src.burst_rows_closest) == (M.K_BURST_MAX_ROWS, M.K_BURST_MAX_ROWS_CLOSEST)
  assert tuple(src.bulyan_cases) == M.BULYAN_CASES
  assert tuple(src.bulyan_eval_shapes) == M.BULYAN_EVAL_SHAPES
  assert src.colwise_eval == M.COLWISE_EVAL
  assert src.order_pair_max_h == M.ORDER_PAIR_MAX_H and src.order_pair_buckets == M.ORDER_PAIR_BUCKETS
  assert src.order_pair_buckets[-1] == src.order_pair_max_h


def test_mirror_vector_widths_match_the_sources(src):
  for n in range(1, src.max_rows + 1):
    for rule in M.RULES:
      assert src.colwise_kmax(rule, n) == M.colwise_max_vec(rule, n), (rule, n)
      assert src.burst(rule, n, 4) == (n <= M.burst_limit(rule)), (rule, n)
      assert not src.burst(rule, n, 2) and not src.burst(rule, n, 1)
    assert c_eval(src.aksel_kmaxvec, {"N": n}) == M.aksel_max_vec(n), n
    assert c_eval(src.eval_kmaxvec, {"N": n}) == M.eval_max_vec(n), n
    assert c_eval(src.order_pair_kmaxvec, {"N": n}) == M.eval_max_vec(n), n
    for mmax in range(1, src.max_rows + 1):
      assert c_eval(src.bulyan_fast_kmaxvec, {"MMAX": mmax}) == M.bulyan_max_vec(mmax), mmax
      assert c_eval(src.bulyan_eval_kmaxvec, {"MMAX": mmax}) == M.bulyan_max_vec(mmax), mmax


def test_case_lists_reach_every_instance(src):
  reachable = src.reachable()
  reached = set()
  for case in M.all_cases(cus=256):
    got = M.instances(case, cus=256)
    assert got <= reachable, (case, got - reachable)
    reached |= got
  missing = sorted(map(str, reachable - reached))
  assert not missing, f"{len(missing)} instances no case runs, e.g. {missing[:8]}"


def test_every_group_reaches_what_it_promises():
  """The groups that exist for one family of instances do reach it (the knob groups run their knob's form)."""
  burst = {i for c in M.cases("knob_burst", 256) for i in M.instances(c, 256)}
  assert burst == {("colwise", r, n, 4, "burst") for r in M.RULES for n in range(1, M.burst_limit(r) + 1)}
  default = {i for c in M.cases("knob_burst", 256) for i in M.instances(c._replace(knobs=()), 256)}
  assert all(i[-1] == "plain" for i in default)  # the parent's digests come from the plain form
  long = {i for c in M.cases("colwise_long", 256) for i in M.instances(c, 256)}
  assert {("colwise", r, n, 4, "burst") for r in M.RULES for n in range(1, M.burst_limit(r) + 1)} <= long
  resnet = {i for c in M.cases("colwise_resnet", 256) for i in M.instances(c, 256)}
  assert all(i[-1] == "burst" for i in resnet)
  wide = [c for c in M.cases("knob_wide", 256)]
  for c in wide:
    assert M.instances(c, 256) != M.instances(c._replace(knobs=()), 256), c
  fast = {i for c in M.cases("bulyan", 256) for i in M.instances(c, 256)}
  assert fast == {("bulyan_pass2", p, v, "plain") for p in M.BULYAN_CASES
                  for v in (4, 2, 1) if v <= M.bulyan_max_vec(p[0] - p[1] - 2)}
  generic = {i for c in M.cases("bulyan_generic", 256) for i in M.instances(c, 256)}
  assert generic == {("bulyan_pass2_generic", 0, 1, "plain")}
  for c in M.cases("bulyan_generic", 256):
    assert c.n >= 4 * c.f + 3 and 1 <= c.m <= c.n - c.f - 2


def test_case_generators_place_rows_at_their_offsets():
  for off in M.OFFSETS:
    offs = M.row_offsets(off, 7)
    assert len(offs) == 7 and all(o in (0, 4, 8, 12) for o in offs)
    assert M.vec_width(offs) == {0: 4, 8: 2}.get(off, 1)
  assert len(set(M.row_offsets("mixed", 4))) == 4
  assert M.burst_lengths(256)[0] // 4 // (256 * 1024) == 1 and M.burst_lengths(256)[1] % 4 == 2
