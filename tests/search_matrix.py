"""The scalar form of the attacks' factor search (csrc/search_core.h through csrc/linesearch.cpp on the host and
csrc/search_device.hip on the device; attacks/identical.py:67-77) against a float64 search ON THE VECTORS: a reference
that knows rows, differences and sums only, the case list, a model of the device kernel's merge that says which of its
paths a case reaches, and the bars (a helper module, not a conftest; the shape of tests/selection_matrix.py).

The host and the device form share their closed forms, so holding one to the other bit for bit
(tests/test_gpu_search_device.py) cannot see a mistake in what they share.  Here both are held, candidate by candidate,
to the rule evaluated on the actual candidate stack:

  reference   `Reference(inputs, k)`: for a factor t, byz = avg.double() + t * direction.double(); the n x n distances
              of honests + [byz] * k as roots of float64 sums of squared DIFFERENCES; Krum's score the ascending sum of
              the n - f - 1 smallest of a row (krum.py:44-62), Bulyan's of the m smallest (bulyan.py:48-62); the stable
              order; the objective |mean(selected rows) - avg|^2; the search `oracle.gar_oracle.line_maximize` around
              it.  No inner product, no Gram form, nothing of search_core.h.
  gap         per candidate, the smallest relative difference between the score of a selected and of an unselected row
              (rows of identical content count as one: swapping them changes nothing); `order_gap` the same between
              any two rows that are neighbours in the order (reported only: mutual nearest neighbours tie exactly
              when one distance is added, on both sides).
  cases       `CASES` (what tests/test_search_matrix_cpu.py runs on the host form and tests/test_gpu_search_matrix.py on
              the device form) and `STEP_CASES`.
  reach       `merge_model`: below / b1 / c2 / c3 per honest row, zeros / rest of the Byzantine row, kb — the stretches of
              attack_search_kernel, from float64 distances; the CPU file ties it to the source and proves that the cases
              reach every path it names.

Where the inputs are CRAFTED (kinds `collapsed` and `on_row`) the point the objective is measured from is the case's
own `avg`, not the mean of its rows: the closed forms hold around any point, and an exact coincidence of a candidate
with a row needs one that lies on the rows' grid.  Bulyan's m stays within 1 .. n - f - 2 (bulyan.py:116); m = n runs
in Krum mode only.
"""

import math
import os
import sys
from collections import namedtuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from oracle import gar_oracle as O  # noqa: E402

# ---------------------------------------------------------------------------------------------------------------------
# Mirror of csrc/search_device.hip (held to the source by tests/test_search_matrix_cpu.py)

BM_MAX_ROWS = 64
K_SEARCH_WAVES = 16
K_SORT_ROWS_PER_WAVE = BM_MAX_ROWS // K_SEARCH_WAVES  # row i is sorted by wave i % 16: a wave's rows wrap at 16, 32, 48
K_RANK_CHUNK = BM_MAX_ROWS // K_SEARCH_WAVES
LDS_OPT_IN_BYTES = 48 * 1024
GROUP = 8  # loads of a stretch leave in groups of eight


def row_span(h):
  return (h + 7) & ~7


def search_ld(h):
  return row_span(h) + 1


def search_lds_bytes(h):
  return (2 * h * search_ld(h) + 2 * BM_MAX_ROWS + 2) * 8 + 2 * K_SEARCH_WAVES * BM_MAX_ROWS * 4


def krum_take(n, f):
  return max(0, min(n - f - 1, n - 1))


# ---------------------------------------------------------------------------------------------------------------------
# Bars

G = 1e-5                  # gap threshold: the distance pass's bar per entry; a score is a sum of roots, each within 5e-6
EXACT_BAR_CAP = 1e-6      # the bar tests/test_linesearch_cpu.py already uses for this comparison
# |y - y64| / max(y64, floor) of the host form on exact distances, worst over the cases of a group, measured by
# tests/test_search_matrix_cpu.py (profiles/search_errors.txt); the bar is 16 x that, and never above the cap.
EXACT_WORST = {"hetero": 4.9e-10, "tight": 1.4e-10, "momentum": 2.6e-10, "duplicates": 1.3e-9, "collapsed": 6.7e-9,
               "on_row": 4.5e-16}
DEVICE_REL = 2e-5  # the project's own bar on distances of the device's pass: 2e-5 |y64| + floor
FIXED_FACTORS = (0.0, 1e-9, 0.3, 1.0, 1.1, -2.5, 17.0, 32767.0)
EVALS = (1, 2, 3, 7, 16, 40)


def exact_bar(kind):
  return min(EXACT_BAR_CAP, 16.0 * EXACT_WORST[kind])


# ---------------------------------------------------------------------------------------------------------------------
# Cases

Case = namedtuple("Case", "kind h k f m attack negative evals seed")
Inputs = namedtuple("Inputs", "rows avg direction")  # fp32: (h, d), (d,), (d,)
D_SMALL, D_PASS = 2003, 20011
KINDS = ("hetero", "tight", "momentum", "duplicates", "collapsed", "on_row")
REFERENCE_GRID = ((9, 2, 2), (20, 5, 5), (14, 11, 11), (39, 12, 12), (27, 24, 24))  # reproduce.py:122-209 as (h, k, f)
STRUCTURE_H = (1, 2, 8, 9, 16, 17, 32, 33, 48, 49, 62)
# a draw at the seed 7 n + f that misses the conditions of the CPU file is replaced by another seed: (case) -> seed
RESEEDED = {("hetero", 20, 5, 5, None, "empire", False, 40): 1180, ("on_row", 33, 31, 30, None, "on_row", True, 16): 4478,
            ("duplicates", 20, 1, 0, 18, "empire", False, 16): 2147,
            ("duplicates", 49, 15, 15, None, "empire", True, 16): 2463}
# (case, rule) whose float64 search ends on its start: the cursor walks back to x = 0 in ever shorter steps and the
# objectives come as close as the abscissae (7e-11 to 9e-16 apart), at every seed tried — `empire` with `negative` puts
# the copies at (1 + x) avg, which Krum on hetero rows selects from x = 0 on.  Exempt from the two-best condition, and
# only these; abscissae and factor are held to the float64 search there all the same.
ENDS_ON_START = frozenset(((("hetero", h, k, f, None, "empire", True, e), "krum")
                           for h, k, f, e in ((9, 2, 2, 16), (20, 5, 5, 16), (39, 12, 12, 16), (63, 1, 1, 16), (20, 5, 5, 40))))


def two_best_condition(case, best_two, bar):
  """The rules ("krum" / "average") of a case whose two best objectives are neither equal nor 100 bars apart."""
  return [rule for rule, apart in best_two.items() if apart < 100 * bar and (tuple(case)[:-1], rule) not in ENDS_ON_START]


def case_id(case):
  return "%s-h%d-k%d-f%d-m%s-%s%s-e%d" % (case.kind, case.h, case.k, case.f, case.m, case.attack,
                                           "neg" if case.negative else "", case.evals)


def default_m(h, k, f):
  return h + k - f - 2


def _case(kind, h, k, f, m=None, attack="empire", negative=False, evals=16):
  n = h + k
  if m is None and default_m(h, k, f) < 1:
    m = 1  # no default at this size (n - f - 2 < 1): plain Krum
  case = Case(kind, h, k, f, m, attack if kind != "on_row" else "on_row", negative, evals, 7 * n + f)
  return case._replace(seed=RESEEDED.get(tuple(case)[:-1], case.seed))


def _cases():
  out = []
  variety = [(a, s) for a in ("empire", "little") for s in (False, True)]
  kinds3 = ("hetero", "tight", "momentum")
  turn = 0

  def add(kind, h, k, f, m=None, evals=16, every_attack=False, only=None):
    nonlocal turn
    for attack, negative in (variety if every_attack else [only or variety[turn % 4]]):
      case = _case(kind, h, k, f, m, attack, negative, evals)
      if case not in out:
        out.append(case)
    turn += 1

  # the reference's worker counts: every kind of input, every attack, both signs; m = default, 1 and n
  for h, k, f in REFERENCE_GRID:
    for kind in KINDS:
      add(kind, h, k, f, every_attack=kind in kinds3)
    for m in (1, h + k):
      for kind in kinds3:
        add(kind, h, k, f, m)
  # the cursor at other budgets
  for evals in EVALS:
    add("hetero", 20, 5, 5, evals=evals, every_attack=True)
  # structure: both sides of every boundary in h, with one copy and with as many as n <= 64 allows
  for i, h in enumerate(STRUCTURE_H):
    for k in (1, BM_MAX_ROWS - h):
      f = min(k, (h + k - 3) // 2) if h + k >= 5 else 0
      # (tight rows next to many copies: once take > h - 1 every honest score holds a distance to the candidate, and at
      # t = 32767 those distances drown the tight rows' own — no seed keeps the gap; tight runs with one copy)
      # two rows lie opposite each other around their mean, and take = 2 > h - 1: neither tight nor on_row keeps the gap
      first = kinds3[i % 3] if (k == 1 and h != 2) or kinds3[i % 3] != "tight" else "hetero"
      add(first, h, k, f, only=("empire", False) if h == 2 else None)
      add(("duplicates", "on_row", "collapsed")[i % 3] if h != 2 else "collapsed", h, k, f)
  # more honest rows than a distance pass serves (search only, the distances uploaded), and no copy at all
  add("hetero", 63, 1, 1, every_attack=True)
  add("tight", 64, 0, 3, every_attack=True)
  add("momentum", 14, 0, 3)
  add("hetero", 1, 0, 0)
  # declared and real counts that differ
  for kind in kinds3:
    add(kind, 20, 3, 5)
    add(kind, 20, 5, 3)
  # take = n - f - 1 at 0, 1, 7, 8, 9, 16, n - 1 and <= k - 1 (then the Byzantine row's score adds zeros only)
  for i, (h, k, take) in enumerate(((20, 5, 0), (20, 5, 1), (20, 5, 7), (20, 5, 8), (20, 5, 9), (20, 5, 16), (20, 1, 20),
                                    (33, 12, 8), (33, 12, 16), (14, 11, 7), (14, 11, 10), (9, 30, 8), (9, 30, 29))):
    f = h + k - 1 - take
    # (take = n - 1: every score holds the distances to the candidate, which drown the rest at t = 32767 unless the
    # direction is short — one copy, along the small mean)
    add(kinds3[i % 3], h, k, f, m=max(1, min(h + k, h - 2)), only=("empire", False) if take == h + k - 1 else None)
    if take >= 16:  # (below that rows that have twins tie exactly with their nearest class: sums of the same numbers)
      add("duplicates", h, k, f, m=max(1, min(h + k, h - 2)))
  return out


CASES = _cases()

# On the distances of the device's pass: the avg of the crafted kinds is the case's own, a distance pass serves
# h + 2 <= 64 rows and `little` needs two; the budgets other than 16 are about the cursor (forty evaluations converge: the
# best two objectives come as close as the last steps are short).  Two draws of `duplicates` with one copy keep their two
# best objectives 3e-4 and 4e-4 apart, under 100 device bars, at every seed tried: they run on exact distances only.
DEVICE_SKIP = (("duplicates", 9, 1, 1, None, "little", True, 16), ("duplicates", 49, 1, 1, None, "little", True, 16))
DEVICE_CASES = [c for c in CASES if c.kind in ("hetero", "tight", "momentum", "duplicates") and 2 <= c.h <= 62
                and c.evals == 16 and tuple(c)[:-1] not in DEVICE_SKIP]
LONG_CASES = [c for c in DEVICE_CASES if c.kind == "hetero" and (c.h, c.k, c.f, c.m, c.attack, c.negative) in
              ((20, 5, 5, None, "empire", False), (39, 12, 12, None, "little", True))]  # these at d = 20 011 as well

StepCase = namedtuple("StepCase", "gar n f attack negative seed")
STEP_CASES = (StepCase("krum", 25, 5, "empire", False, 180), StepCase("krum", 51, 12, "little", False, 369),
              StepCase("average", 25, 5, "empire", True, 180), StepCase("bulyan", 25, 5, "little", False, 180),
              StepCase("bulyan", 51, 12, "empire", False, 369))


def honest_rows(kind, h, k, f, d, seed):
  """The h fp32 honest rows of a case, (h, d)."""
  n = h + k
  if kind in ("hetero", "tight", "momentum"):
    return torch.stack(O.make_stack(kind, h + max(k, 1), max(k, 1), d, seed)[0][:h])
  gen = torch.Generator().manual_seed(seed)
  base = 0.3 * torch.randn(d, generator=gen)
  if kind == "duplicates":  # h // 3 distinct rows: exact ties among the honest distances and among the scores
    few = [base + (0.5 + 0.1 * i) * torch.randn(d, generator=gen) for i in range(max(1, h // 3))]
    return torch.stack([few[i % len(few)] for i in range(h)])
  if kind == "collapsed":
    return torch.stack([base] * h)
  if kind == "on_row":  # on a grid of 2^-10 below 16: every difference and every sum of two is exact in fp32
    rows = torch.stack([base + (0.5 + 0.1 * i) * torch.randn(d, generator=gen) for i in range(h)])
    return torch.round(rows.clamp(-7.0, 7.0) * 1024.0) / 1024.0
  raise ValueError((kind, n))


def direction_of(rows, avg, attack):
  """`grad_att` of identical.py:65 as the host computes it (:129-141)."""
  if attack == "empire":
    return avg.neg()
  if attack == "little":
    return rows.var(dim=0).sqrt_() if rows.shape[0] > 1 else torch.zeros_like(avg)
  raise ValueError(attack)


def inputs_of(case, d=D_SMALL):
  """rows, avg and direction of a case, formed on the CPU in fp32 (the device file forms avg and direction with the
  product where the distances come from the device's pass)."""
  rows = honest_rows(case.kind, case.h, case.k, case.f, d, case.seed)
  if case.kind == "collapsed":
    avg = rows[0].clone()  # the mean of equal rows: a_i = 0 exactly
    return Inputs(rows, avg, direction_of(rows, avg, case.attack))
  if case.kind == "on_row":
    avg = torch.round(rows.mean(dim=0) * 1024.0) / 1024.0
    target = rows[case.h // 2].clone()
    rows = rows.clone()
    direction = target - avg  # exact: avg + 1 * direction IS rows[h // 2], bit for bit, in fp32 and in float64
    assert torch.equal(avg + direction, target) and torch.equal(avg.double() + direction.double(), target.double())
    return Inputs(rows, avg, direction)
  avg = rows.mean(dim=0)
  return Inputs(rows, avg, direction_of(rows, avg, case.attack))


def exact_ext(inputs):
  """The (h+2)^2 squared distances among honests + [avg, avg + direction] in float64 from the rows (direct
  differences; the last row unrounded): what isolates the search from the distance pass."""
  rows = torch.cat([inputs.rows.double(), inputs.avg.double()[None], (inputs.avg.double() + inputs.direction.double())[None]])
  out = torch.empty(rows.shape[0], rows.shape[0], dtype=torch.float64)
  for i in range(rows.shape[0]):
    out[i] = (rows - rows[i]).pow(2).sum(dim=1)
  return out.contiguous()


def objective_floor(inputs):
  """tests/test_gpu_parity_r2.py:412: an objective that is zero up to rounding comes out of a cancellation among h^2
  inner products, so the absolute floor is relative to the spread of the honest rows: 1e-8 h honest_norm_dev^2."""
  h = inputs.rows.shape[0]
  spread = (inputs.rows.double() - inputs.avg.double()).pow(2).sum().item()
  return 1e-8 * h * spread / max(h - 1, 1)


# ---------------------------------------------------------------------------------------------------------------------
# The float64 reference

Candidate = namedtuple("Candidate", "t order scores classes selection objective gap order_gap")


class Reference:
  """The rule on the vectors in float64 for the candidate stacks honests + [avg + t direction] * k of one case."""

  def __init__(self, inputs, k):
    self.rows = inputs.rows.double()
    self.avg = inputs.avg.double()
    self.direction = inputs.direction.double()
    self.h, self.k = self.rows.shape[0], k
    self.n = self.h + k
    hh = torch.empty(self.h, self.h, dtype=torch.float64)
    for i in range(self.h):
      hh[i] = (self.rows - self.rows[i]).pow(2).sum(dim=1).sqrt_()
    self.hh = hh.numpy()
    # rows of identical content form one class, named by its first row
    self.honest_class = np.array([int(np.flatnonzero(self.hh[i] == 0.0)[0]) for i in range(self.h)], dtype=np.int64)

  def byzantine(self, t):
    return self.avg + t * self.direction

  def distances(self, t):
    """(n x n distances with a +inf diagonal, the honest rows' distances to the candidate)."""
    h, n = self.h, self.n
    dq = (self.rows - self.byzantine(t)).pow(2).sum(dim=1).sqrt_().numpy()
    dist = np.zeros((n, n))
    dist[:h, :h] = self.hh
    dist[:h, h:] = dq[:, None]
    dist[h:, :h] = dq[None, :]
    np.fill_diagonal(dist, math.inf)
    return dist, dq

  def classes(self, dq):
    on = np.flatnonzero(dq == 0.0)
    byz = int(self.honest_class[on[0]]) if len(on) else self.h
    return np.concatenate([self.honest_class, np.full(self.k, byz, dtype=np.int64)])

  def scores(self, dist, take):
    """Ascending sums of the `take` smallest of every row (the diagonal is +inf and take <= n - 1)."""
    if take <= 0:
      return np.zeros(self.n)
    return np.cumsum(np.sort(dist, axis=1), axis=1)[:, take - 1]  # (a cumulative sum adds left to right)

  def objective(self, selection, t):
    """|mean(selected rows) - avg|^2."""
    picked = np.asarray(selection, dtype=np.int64)
    kb = int((picked >= self.h).sum())
    # (every row stands for the first row of its content, in index order: selections of identical content add the same
    # numbers in the same order and tie exactly, as they do in the reference where they are the same vectors)
    named = np.sort(self.honest_class[picked[picked < self.h]])
    # mean(rows) - avg as the mean of (row - avg): the same quantity, without the cancellation against |avg|
    total = (self.rows[torch.from_numpy(named)] - self.avg).sum(dim=0) + kb * (self.byzantine(t) - self.avg)
    diff = total / float(len(picked))
    return (diff * diff).sum().item()

  def candidate(self, t, take, m=None):
    """The stable order of the scores that add `take` distances; with m, the selection order[:m], its objective and
    the gap between selected and unselected rows."""
    dist, dq = self.distances(t)
    scores = self.scores(dist, take)
    order = np.argsort(scores, kind="stable")
    classes = self.classes(dq)
    ranked, ranked_class = scores[order], classes[order]
    apart = ranked_class[1:] != ranked_class[:-1]
    order_gap = _relative_gap(ranked[:-1][apart], ranked[1:][apart])
    if m is None:
      return Candidate(t, order.tolist(), scores, classes, None, None, None, order_gap)
    inside, outside = order[:m], order[m:]
    gap = math.inf
    if len(outside):
      # the order is ascending: the closest pair of different content lies between the last selected rows of a class
      # and the first unselected ones of another — all pairs are few enough to look at
      si, so = scores[inside][:, None], scores[outside][None, :]
      differ = classes[inside][:, None] != classes[outside][None, :]
      if differ.any():
        gap = _relative_gap(np.broadcast_to(si, differ.shape)[differ], np.broadcast_to(so, differ.shape)[differ])
    return Candidate(t, order.tolist(), scores, classes, inside.tolist(), self.objective(inside, t), gap, order_gap)

  def average(self, t):
    return self.objective(np.arange(self.n), t)


def _relative_gap(a, b):
  if len(a) == 0:
    return math.inf
  scale = np.maximum(np.abs(a), np.abs(b))
  with np.errstate(invalid="ignore", divide="ignore"):
    rel = np.where(scale > 0.0, np.abs(a - b) / scale, 0.0)
  return float(rel.min())


def same_up_to_identical_rows(order, want, classes):
  """Two orders over distinct rows (a permutation, or the first m entries of one) that differ only by exchanging rows of
  identical content."""
  return len(order) == len(want) and len(set(order)) == len(order) and all(0 <= a < len(classes) for a in order) and \
      all(classes[a] == classes[b] for a, b in zip(order, want))


def vector_search(reference, case, rule):
  """The reference's search (tools.line_maximize around the rule on the vectors, rule "krum" / "average"): factor,
  [(x, y)], and per evaluation the Candidate (Krum) or None (Average)."""
  n = reference.n
  seen = []

  def scape(x):
    t = -x if case.negative else x
    if rule == "average":
      seen.append(None)
      return reference.average(t)
    cand = reference.candidate(t, krum_take(n, case.f), case.m or default_m(case.h, case.k, case.f))
    seen.append(cand)
    return cand.objective

  factor, trace = O.line_maximize(scape, evals=case.evals)
  return factor, trace, seen


def replay(trace, factor):
  """(a) the cursor: the abscissae and the factor a form reports must be the ones tools.line_maximize's restatement
  proposes when it is fed that form's objectives, bit for bit."""
  fed = iter(trace)

  def scape(x):
    xo, yo = next(fed)
    assert x == xo, ("abscissa", x, xo)
    return yo

  want, _ = O.line_maximize(scape, evals=len(trace))
  assert want == factor, ("factor", want, factor)


def two_best_differ_by(trace):
  """The relative difference of the two largest DISTINCT objectives of a trace (inf when there is one value only)."""
  values = sorted({y for _, y in trace}, reverse=True)
  if len(values) < 2 or values[0] == 0.0:
    return math.inf
  return (values[0] - values[1]) / values[0]


# ---------------------------------------------------------------------------------------------------------------------
# The merge of attack_search_kernel, from float64 distances

Merge = namedtuple("Merge", "below b1 c2 c3 most1 most3 zeros rest kb")


def _longest(values, limit):
  return limit if any(v >= limit for v in values) else max(values, default=0)


def merge_model(reference, t, take, m):
  """What attack_search_kernel walks at factor t: per honest row i, `below` of its h - 1 sorted honest distances lie
  under dq_i, and the `take` smallest of the merged sequence are b1 of the row, c2 copies of dq_i, c3 more of the row;
  the stretches run to the longest one over ALL 64 lanes of wave 0 (`longest` ballots the whole wave): a lane beyond h
  carries dq = +inf and walks row 0, so all h - 1 values lie below and its b1 is min(h - 1, take) — most1 / most3 are
  the kernel's loop lengths, the per-row b1 / c2 / c3 each lane's own; the Byzantine row adds k - 1 zeros and `rest` sorted dq."""
  h, k = reference.h, reference.k
  _, dq = reference.distances(t)
  below, b1, c2, c3 = [], [], [], []
  for i in range(h):
    others = np.delete(reference.hh[i], i)
    lo = int((others < dq[i]).sum())
    below.append(lo)
    b1.append(min(lo, take))
    c2.append(min(take - b1[-1], k))
    c3.append(take - b1[-1] - c2[-1])
  zeros = min(k - 1, take) if k > 0 else 0
  rest = take - zeros if k > 0 else 0
  cand = reference.candidate(t, take, m)
  kb = sum(1 for i in cand.selection if i >= h)
  idle_b1 = [min(h - 1, take)] if h < BM_MAX_ROWS else []  # lanes h .. 63 of wave 0
  idle_c3 = [take - b - min(take - b, k) for b in idle_b1]
  return Merge(below, b1, c2, c3, _longest(b1 + idle_b1, take), _longest(c3 + idle_c3, take), zeros, rest, kb)


def reach_of(merge, k):
  """The names of the paths one candidate's merge reaches."""
  out = set()
  for b1, c2, c3 in zip(merge.b1, merge.c2, merge.c3):
    if c2 == 0:
      out.add("c2=0")
    if 0 < c2 < k:
      out.add("0<c2<k")
    if k > 0 and c2 == k and c3 > 0:
      out.add("c2=k,c3>0")
    if c3 == 0:
      out.add("c3=0")
  for name, most in (("b1", merge.most1), ("c3", merge.most3)):
    if most > 0 and most % GROUP == 0:
      out.add(name + " ends on a group")
    if most > GROUP and most % GROUP == 1:
      out.add(name + " one past a group")
  if k > 0:
    out.add("kb=0" if merge.kb == 0 else ("kb=k" if merge.kb == k else "0<kb<k"))
    if merge.rest == 0:
      out.add("rest=0")
  return out


REACH = ("c2=0", "0<c2<k", "c2=k,c3>0", "c3=0", "b1 ends on a group", "b1 one past a group", "c3 ends on a group",
         "c3 one past a group", "kb=0", "0<kb<k", "kb=k", "rest=0")


def structural_tie(case, t):
  """Candidates at which rows of different content tie by construction — exactly so in float64 and in the scalar form,
  whatever the draw: take = 0 (every score is an empty sum), a single honest row (its score and its copy's are the one
  distance), and two honest rows at |t| <= 1e-6 (both are equally far from their mean, which the candidate then is: exactly so on exact
  distances, to the last bits of two entries of the distance pass otherwise — the two rows then count as one content)."""
  return krum_take(case.h + case.k, case.f) == 0 or case.h == 1 or (case.h == 2 and abs(t) <= 1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# The comparison itself, for any form of the search

Study = namedtuple("Study", "worst worst_rel gap order_gap best_two reach")  # best_two: {rule: distance}


def examine(case, inputs, form, within, rankings_need_copies=False):
  """Hold one form of the search to the float64 search on the vectors at one case (a - e of the test files' headers).
  form.search(rule) -> (factor, [(x, y)]); form.rankings(mode, m, ts) -> one permutation per factor;
  form.objective(rule, t) -> (y, selection) or None where the form reports no selection of its own (the device form:
  the selection is then its Krum ranking's first m rows).  within(y, y64, floor) -> bool is the objective's bar.
  Returns what it measured: the worst |y - y64| / max(y64, floor) and |y - y64| / y64, the smallest gap, ..."""
  h, k, f, n = case.h, case.k, case.f, case.h + case.k
  ref = Reference(inputs, k)
  floor = objective_floor(inputs)
  m = case.m or default_m(h, k, f)
  take = krum_take(n, f)
  tag = case_id(case)
  worst, worst_rel, gap, order_gap, best_two, reach = 0.0, 0.0, math.inf, math.inf, {}, set()
  ranked = k >= 1 or not rankings_need_copies

  def measure(y, y64, where):
    nonlocal worst, worst_rel
    assert within(y, y64, floor), (tag, where, y, y64, floor)
    if y != y64:
      worst = max(worst, abs(y - y64) / max(y64, floor))
      worst_rel = max(worst_rel, abs(y - y64) / y64 if y64 > floor else 0.0)

  signed = lambda x: -x if case.negative else x  # noqa: E731
  krum_trace = None
  for rule in ("krum", "average"):
    factor, trace = form.search(rule)
    replay(trace, factor)                                                                     # a
    want_factor, want_trace, seen = vector_search(ref, case, rule)
    best_two[rule] = two_best_differ_by(want_trace)
    assert [x for x, _ in trace] == [x for x, _ in want_trace] and factor == want_factor, (tag, rule, trace, want_trace)  # d
    if rule == "krum":
      krum_trace = trace
      continue
    for (x, y), (_, y64) in zip(trace, want_trace):                                           # e
      measure(y, y64, (rule, x))
      if form.objective(rule, signed(x)) is not None:
        assert form.objective(rule, signed(x)) == (y, list(range(n))), (tag, rule, x)

  # b, c: the permutation in Krum mode with the case's f, in Bulyan mode at m = the case's and 1; the objective of the
  # selection the form made
  ts = [signed(x) for x, _ in krum_trace] + list(FIXED_FACTORS)
  orders = form.rankings("krum", m, ts) if ranked else [None] * len(ts)
  bulyan_ms = sorted({mm for mm in (m, 1) if 1 <= mm <= n - f - 2}) if ranked else []
  bulyan = {mb: form.rankings("bulyan", mb, ts) for mb in bulyan_ms}
  for i, t in enumerate(ts):
    cand = ref.candidate(t, take, m)
    if h == 2 and structural_tie(case, t):  # the two rows are one another's mirror image around the candidate
      cand.classes[1] = cand.classes[0]
    sel = None
    if orders[i] is not None:
      assert sorted(orders[i]) == list(range(n)), (tag, "krum", t, orders[i])
      assert same_up_to_identical_rows(orders[i], cand.order, cand.classes), (tag, "krum", t, orders[i], cand.order, cand.order_gap)
      sel = orders[i][:m]
    own = form.objective("krum", t)
    if own is not None:
      assert sel is None or own[1] == sel, (tag, t, own[1], sel)
      sel = own[1]
      if i < len(krum_trace):
        assert own[0] == krum_trace[i][1], (tag, t)  # one evaluation = the search's evaluation, bit for bit
    if sel is not None:
      assert same_up_to_identical_rows(sel, cand.selection, cand.classes), (tag, t, sel, cand.selection, cand.gap)
    y = krum_trace[i][1] if i < len(krum_trace) else (own[0] if own is not None else None)
    if y is not None:
      # (no selection of the form's own: without copies the device form ranks nothing — the float64 selection then)
      measure(y, ref.objective(sel if sel is not None else cand.selection, t), ("krum", t))
    if not structural_tie(case, t):
      gap = min(gap, cand.gap)
    order_gap = min(order_gap, cand.order_gap)
    reach |= reach_of(merge_model(ref, t, take, m), k)
    for mb in bulyan_ms:
      cand_b = ref.candidate(t, mb)
      if h == 2 and structural_tie(case, t):
        cand_b.classes[1] = cand_b.classes[0]
      assert sorted(bulyan[mb][i]) == list(range(n)), (tag, "bulyan", mb, t, bulyan[mb][i])
      assert same_up_to_identical_rows(bulyan[mb][i], cand_b.order, cand_b.classes), \
          (tag, "bulyan", mb, t, bulyan[mb][i], cand_b.order, cand_b.order_gap)
      order_gap = min(order_gap, cand_b.order_gap)
  return Study(worst, worst_rel, gap, order_gap, best_two, frozenset(reach))


def within_exact(kind):
  bar = exact_bar(kind)
  return lambda y, y64, floor: abs(y - y64) <= bar * max(y64, floor)


def within_device(y, y64, floor):
  return abs(y - y64) <= DEVICE_REL * abs(y64) + floor


def bulyan_search(reference, case):
  """The reference's search around Bulyan on the vectors in float64 (oracle.gar_oracle.bulyan): factor, [(x, y)]."""
  def scape(x):
    byz = reference.byzantine(-x if case.negative else x)
    out = O.bulyan(list(reference.rows) + [byz] * reference.k, case.f, precision="f64") - reference.avg
    return out.dot(out).item()
  return O.line_maximize(scape, evals=case.evals)


def conditions_at(case, inputs):
  """(smallest gap over the trace and FIXED_FACTORS, {rule: distance of the two best objectives}) of the float64 search
  alone: what the comparison needs of a draw, whatever form is compared."""
  ref = Reference(inputs, case.k)
  take, m = krum_take(case.h + case.k, case.f), case.m or default_m(case.h, case.k, case.f)
  best_two, gap = {}, math.inf
  for rule in ("krum", "average"):
    _, trace, _ = vector_search(ref, case, rule)
    best_two[rule] = two_best_differ_by(trace)
    if rule == "krum":
      for t in [(-x if case.negative else x) for x, _ in trace] + list(FIXED_FACTORS):
        if not structural_tie(case, t):
          gap = min(gap, ref.candidate(t, take, m).gap)
  return gap, best_two


# ---------------------------------------------------------------------------------------------------------------------
# profiles/search_errors.txt: BM_SEARCH_ERRORS=FILE makes both test files record what they measure, one line per
# (source, kind, h), merged into what FILE already holds from the other file's run

_RECORD = {}


def record(source, case, got, bar):
  path = os.environ.get("BM_SEARCH_ERRORS")
  if not path:
    return
  if not _RECORD and os.path.exists(path):
    for line in open(path):
      part = line.split()
      if len(part) == 9 and part[0] != "#":
        _RECORD[(part[0], part[1], int(part[2]))] = [float(v) for v in part[3:8]] + [part[8]]
  key = (source, case.kind, case.h)
  old = _RECORD.get(key, [0.0, 0.0, math.inf, math.inf, 0, bar])
  _RECORD[key] = [max(old[0], got.worst), max(old[1], got.worst_rel), min(old[2], got.gap),
                  min([old[3]] + [v for r, v in got.best_two.items() if (tuple(case)[:-1], r) not in ENDS_ON_START]),
                  int(old[4]) + 1, bar]
  with open(path, "w") as out:
    out.write("# source kind h  worst |y - y64| / max(y64, floor)  worst / y64 where y64 > floor  smallest gap  "
              "two best apart by (ENDS_ON_START left out)  cases  bar\n")
    for (src, kind, h), v in sorted(_RECORD.items()):
      out.write("%-14s %-10s %-3d %.2e %.2e %.2e %.2e %d %s\n" % (src, kind, h, v[0], v[1], v[2], v[3], v[4], v[5]))
