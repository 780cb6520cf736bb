"""Which compiled instance a call lands in, seeded inputs that reach every instance, and the float64 references the
instance tests compare against (a helper module, not a conftest).

A call's result depends on more than the rule and the row count: it runs in ONE of many compiled instances, chosen at
run time and invisible to the caller, by
  * the row count N (one kernel per N = 1..64, colwise_dispatch.h; per (n, f) for Bulyan's pass 2, bulyan.hip),
  * the vector width VEC = 4 / 2 / 1, the widest every row pointer and the output allow (Alignment,
    launch_plan.h) capped per instance by its `kMaxVec`,
  * the launch form (plain grid-stride, or the burst form of the column kernels), and the BM_* tuning knobs.
The per-column arithmetic is the same in every instance, so a column must give the same bits whichever instance
computed it.

Three parts:
  * a mirror of the dispatch rules: `instances(case, cus)` returns the (kernel, N, VEC, form) instances a call runs;
    tests/test_instance_matrix_cpu.py holds the mirror to the sources and the case lists below to the instances the
    sources can reach;
  * seeded case generators: the rows of a case are cut out of ONE flat allocation so that each starts at byte offset 0,
    4, 8 or 12 ("mixed": a different offset per row), and the same values are copied to every offset, so that outputs
    can be compared bit for bit across widths;
  * float64 references of the coordinate-wise rules (the closest-to-centre window, its legal alternatives at exact
    ties) shared with tests/test_gpu_parity_r2.py.

`python tests/instance_matrix.py GROUP` (with BM_* knobs in the environment) prints one JSON line: the SHA-256 of every
output of GROUP's cases — how the knob tests compare a knob's instances with the defaults, one process per knob (the
knobs are read once per process).
"""

import hashlib
import json
import math
import os
import sys
from collections import namedtuple

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from oracle import gar_oracle as O  # noqa: E402

# ---------------------------------------------------------------------------------------------------------------------
# Mirror of the dispatch rules (colwise_dispatch.h, bulyan.hip, search_eval.hip, bm_common.h, include/bm_gar.h)

MEDIAN, TRMEAN, PHOCAS, MEAMED = "median", "trmean", "phocas", "meamed"
RULES = (MEDIAN, TRMEAN, PHOCAS, MEAMED)
CLOSEST = (PHOCAS, MEAMED)

BM_MAX_ROWS = 64
K_BURST_MAX_ROWS = 25          # median / trimmed mean
K_BURST_MAX_ROWS_CLOSEST = 22  # phocas / meamed
K_BURST_THREADS = 1024
K_BURST_SLOTS = 10             # iterations staged in LDS per burst (160 KB / (1024 lanes * 16 bytes))
K_COL_BLOCK = 256
K_COL_MAX_BLOCKS = 256 * 64
K_MAX_COLS_PER_LAUNCH = 1 << 29

# register-resident Bulyan pass 2 (BM_BULYAN_CASE), in the order of the source
BULYAN_CASES = ((11, 2), (15, 3), (19, 4), (25, 5), (23, 5), (27, 6), (31, 7), (35, 8), (39, 9), (43, 10), (47, 11),
                (51, 12), (51, 10), (7, 1))
BULYAN_EVAL_SHAPES = ((11, 2), (25, 5), (51, 12))       # bm_bulyan_pass2_eval_supported, m = n - f - 2
COLWISE_EVAL = {MEDIAN: (3,), TRMEAN: (11, 25, 51), PHOCAS: (11, 25, 51), MEAMED: (11, 25, 51)}  # bm_colwise_eval_supported
ORDER_PAIR_MAX_H = 51                                   # bm_order_pair_supported: 1 <= h <= 51
ORDER_PAIR_BUCKETS = (11, 25, 51)                       # h <= 11 -> 11, h <= 25 -> 25, else 51

DEFAULT_KNOBS = {"BM_COL_BURST": 8, "BM_COL_WIDE": 1, "BM_BULYAN_SHORT": 1}


def colwise_max_vec(rule, n):
  """kMaxVec of launch_colwise_n<N, OP>."""
  closest = rule in CLOSEST
  if n <= 28:
    return 4
  if not closest and n <= 52:
    return 4
  return 2 if n <= (54 if closest else 56) else 1


def bulyan_max_vec(mmax):
  """kMaxVec of launch_bulyan_fast / launch_bulyan_eval (MMAX = n - f - 2 ranked rows)."""
  return 4 if mmax <= 20 else (2 if mmax <= 44 else 1)


def aksel_max_vec(n):
  """kMaxVec of launch_aksel_n<N>."""
  return 2 if n <= 52 else 1


def eval_max_vec(n):
  """kMaxVec of launch_eval<N, OP> and launch_order_pair<N> (search_eval.hip)."""
  return 4 if n <= 28 else 2


def burst_limit(rule):
  return K_BURST_MAX_ROWS if rule in (MEDIAN, TRMEAN) else K_BURST_MAX_ROWS_CLOSEST


def vec_width(byte_offsets):
  """Alignment::vec (launch_plan.h): the widest vector every pointer allows (allocations themselves are 256-byte aligned)."""
  bits = 0
  for o in byte_offsets:
    bits |= o
  return 4 if bits % 16 == 0 else (2 if bits % 8 == 0 else 1)


def order_pair_bucket(h):
  for b in ORDER_PAIR_BUCKETS:
    if h <= b:
      return b
  raise ValueError(h)


# A case: one call of one entry point.  offset: 0 / 4 / 8 bytes for every row, or "mixed" (row_offsets); knobs: the
# BM_* values its process runs with (() = defaults); group: the test that runs it.
Case = namedtuple("Case", "group kernel rule n f m offset d knobs")


def row_offsets(offset, count):
  """Byte offset of each of `count` distinct rows: the same for all, or for "mixed" 4, 0, 12, 8, 4, ... (VEC = 1)."""
  if offset == "mixed":
    return [(4 + 12 * i) % 16 for i in range(count)]
  return [offset] * count


def _body_tail(vec, d):
  """(VEC of the body launch or None, whether a VEC = 1 launch takes the rest): the split of the launchers that run
  the d % VEC trailing columns as a second, scalar launch."""
  body = vec if vec >= 2 and d // vec > 0 else None
  return body, (d - (d // vec) * vec if body else d) > 0


def instances(case, cus=256):
  """The (kernel, N, VEC, form) instances the call of `case` runs, under the case's knobs, on a device with `cus`
  compute units.  N is the row count, or (n, f) for Bulyan's pass 2."""
  knobs = dict(DEFAULT_KNOBS, **dict(case.knobs))
  k = case.kernel
  if k == "colwise":
    # launch_colwise_n / launch_colwise_vec: one launch per 2^29 columns, the d % VEC tail inside it (Tail::kRides, launch_plan.h)
    vec = min(vec_width(row_offsets(case.offset, case.n)), colwise_max_vec(case.rule, case.n))
    if vec == 4 and case.n > 28 and knobs["BM_COL_WIDE"] == 0:
      vec = 2
    if vec == 4 and case.n <= burst_limit(case.rule):
      nvec = min(case.d, K_MAX_COLS_PER_LAUNCH) // 4
      if knobs["BM_COL_BURST"] > 0 and nvec // (cus * K_BURST_THREADS) >= knobs["BM_COL_BURST"]:
        return {("colwise", case.rule, case.n, 4, "burst")}
    return {("colwise", case.rule, case.n, vec, "plain")}
  if k == "bulyan":
    mmax = case.n - case.f - 2
    if case.m == mmax and (case.n, case.f) in BULYAN_CASES:
      vec = min(vec_width(row_offsets(case.offset, case.n)), bulyan_max_vec(mmax))
      if vec == 4 and case.d // 4 > 0:
        v = 4
      elif vec >= 2 and case.d // 2 > 0:
        v = 2
      else:
        v = 1
      return {("bulyan_pass2", (case.n, case.f), v, "plain")}
    return {("bulyan_pass2_generic", 0, 1, "plain")}
  if k == "aksel":
    vec = min(vec_width(row_offsets(case.offset, case.n)), aksel_max_vec(case.n))
    if vec == 2 and case.n > 28 and knobs["BM_COL_WIDE"] == 0:
      vec = 1
    body, tail = _body_tail(vec, case.d)
    out = {("aksel_pass1", case.n, body, "plain")} if body else set()
    return out | ({("aksel_pass1", case.n, 1, "plain")} if tail else set())
  if k in ("colwise_eval", "bulyan_pass2_eval", "order_pair"):
    # honest rows + avg + dir (or lo + hi) at the case's offset: one body launch at the widest VEC, then VEC = 1
    if k == "colwise_eval":
      key, cap = case.n, eval_max_vec(case.n)
      name = ("colwise_eval", case.rule)
    elif k == "bulyan_pass2_eval":
      key, cap = (case.n, case.f), bulyan_max_vec(case.n - case.f - 2)
      name = ("bulyan_pass2_eval",)
    else:
      key = order_pair_bucket(case.n)
      cap = eval_max_vec(key)
      name = ("order_pair",)
    vec = min(vec_width(row_offsets(case.offset, case.n)), cap)
    body, tail = _body_tail(vec, case.d)
    out = {name + (key, body, "plain")} if body else set()
    return out | ({name + (key, 1, "plain")} if tail else set())
  raise ValueError(k)


# ---------------------------------------------------------------------------------------------------------------------
# The case lists (every GPU test of tests/test_gpu_instance_matrix.py runs exactly the cases of its group)

OFFSETS = (0, 4, 8, "mixed")
D_SHORT = 2051                 # vector body + a 3-column tail
D_LONG = 17_000_003            # more than one grid-stride trip per lane at every VEC (16384 x 256 lanes); burst form at
                               # VEC 4 from 8 iterations per CU: 16 of them here, across the 10-slot staging groups
D_SWEEP = 515                  # the f sweep
D_RESNET18 = 11_173_962
D_BULYAN = (4099, 30011)


def f_main(n):
  return (n - 1) // 4


def burst_lengths(cus):
  """1 and 1.5 iterations of the burst form per CU, each with a tail."""
  span = 4 * cus * K_BURST_THREADS
  return (span + 3, span + span // 2 + 2)


BULYAN_GENERIC = ((13, 2, 9), (29, 6, 21), (64, 15, 47), (25, 5, 7), (51, 12, 20), (19, 4, 5), (7, 1, 2))


def cases(group, cus=256):
  out = []
  if group == "colwise_short" or group == "colwise_long":
    d = D_SHORT if group == "colwise_short" else D_LONG
    for n in range(1, BM_MAX_ROWS + 1):
      for rule in RULES:
        for off in OFFSETS:
          out.append(Case(group, "colwise", rule, n, f_main(n), None, off, d, ()))
  elif group == "colwise_f":
    for n in range(1, BM_MAX_ROWS + 1):
      for f in range(1, (n - 1) // 2 + 1):
        for rule in (TRMEAN, PHOCAS, MEAMED):
          out.append(Case(group, "colwise", rule, n, f, None, 0, D_SWEEP, ()))
  elif group == "colwise_resnet":
    for n in (11, 20):
      for rule in (PHOCAS, MEAMED):
        out.append(Case(group, "colwise", rule, n, f_main(n), None, 0, D_RESNET18, ()))
  elif group == "knob_burst":
    for rule in RULES:
      for n in range(1, burst_limit(rule) + 1):
        for d in burst_lengths(cus):
          out.append(Case(group, "colwise", rule, n, f_main(n), None, 0, d, (("BM_COL_BURST", 1),)))
  elif group == "knob_wide":
    for rule in (MEDIAN, TRMEAN):
      for n in range(29, 53):
        out.append(Case(group, "colwise", rule, n, f_main(n), None, 0, D_SHORT, (("BM_COL_WIDE", 0),)))
    for n in range(29, 53):
      out.append(Case(group, "aksel", None, n, 0, None, 0, D_SHORT, (("BM_COL_WIDE", 0),)))
  elif group in ("bulyan", "knob_bulyan_short"):
    knobs = (("BM_BULYAN_SHORT", 0),) if group == "knob_bulyan_short" else ()
    for n, f in BULYAN_CASES:
      for off in (0, 8, 4):
        for d in D_BULYAN:
          out.append(Case(group, "bulyan", None, n, f, n - f - 2, off, d, knobs))
  elif group == "bulyan_generic":
    for n, f, m in BULYAN_GENERIC:
      for off in (0, 4):
        out.append(Case(group, "bulyan", None, n, f, m, off, 4099, ()))
  elif group == "aksel":
    for n in range(1, BM_MAX_ROWS + 1):
      for off in (0, 8, 4):
        out.append(Case(group, "aksel", None, n, 0, None, off, D_SHORT, ()))
  elif group == "colwise_eval":
    for rule, ns in COLWISE_EVAL.items():
      for n in ns:
        f = 0 if rule == MEDIAN else (n - 1) // 4 + (1 if rule == PHOCAS else 0)
        for off in (0, 4, 8):
          out.append(Case(group, "colwise_eval", rule, n, f, None, off, 4099, ()))
  elif group == "bulyan_pass2_eval":
    for n, f in BULYAN_EVAL_SHAPES:
      for off in (0, 4, 8):
        out.append(Case(group, "bulyan_pass2_eval", None, n, f, n - f - 2, off, 4099, ()))
  elif group == "order_pair":
    for h in (2, 11, 12, 25, 26, 51):
      for off in (0, 4, 8):
        out.append(Case(group, "order_pair", None, h, 0, None, off, 4099, ()))
  else:
    raise ValueError(group)
  return out


GROUPS = ("colwise_short", "colwise_long", "colwise_f", "colwise_resnet", "knob_burst", "knob_wide", "bulyan",
          "knob_bulyan_short", "bulyan_generic", "aksel", "colwise_eval", "bulyan_pass2_eval", "order_pair")


def all_cases(cus=256):
  return [c for g in GROUPS for c in cases(g, cus)]


# ---------------------------------------------------------------------------------------------------------------------
# Seeded inputs

def place(distinct, offset):
  """Copy the rows of `distinct` (u x d, on the GPU) into ONE flat allocation so that row i starts at byte offset
  row_offsets(offset, u)[i] modulo 16; returns the views."""
  u, d = distinct.shape
  offs = row_offsets(offset, u)
  stride = (d + 3) // 4 * 4 + 4
  flat = torch.empty(u * stride + 4, dtype=torch.float32, device=distinct.device)
  assert flat.data_ptr() % 256 == 0
  if len(set(offs)) == 1:
    o = offs[0] // 4
    flat[:u * stride].view(u, stride)[:, o:o + d].copy_(distinct)
  else:
    for i in range(u):
      flat[i * stride + offs[i] // 4: i * stride + offs[i] // 4 + d].copy_(distinct[i])
  views = [flat[i * stride + offs[i] // 4: i * stride + offs[i] // 4 + d] for i in range(u)]
  for v, o in zip(views, offs):
    assert v.data_ptr() % 16 == o
  return views


def rows_of(views, rowmap):
  """The gradient list: row i is the view of distinct row rowmap[i] (aliased rows are the SAME tensor object)."""
  return [views[j] for j in rowmap]


N_KINDS = 5  # NaN x f, NaN x (f + 1), +-inf, +-0, half the rows +inf


def hot_starts(d):
  """Column windows whose values the colwise tests check in full at long lengths: the start, the second grid-stride
  trip of the plain kernels at VEC 1 / 2 / 4, a burst staging-group boundary, and the end."""
  trip = K_COL_MAX_BLOCKS * K_COL_BLOCK
  starts = [0]
  for s in (trip, 2 * trip, 4 * trip, K_BURST_SLOTS * 256 * K_BURST_THREADS * 4):
    if s + 512 < d - 1024:
      starts.append(s - 512)
  return starts


def colwise_values(n, d, f, seed, device="cuda:0"):
  """(distinct u x d float32 on the device, rowmap) for the coordinate-wise rules: randn rows; from n = 10 on, n // 5
  aliased Byzantine rows (the same storage repeated); every 7th column quantised to halves (heavy ties); and, at every
  hot start and in the d % 4 trailing columns, columns holding exactly f and f + 1 NaNs, +-inf, zeros of both signs
  and +inf in half the rows — each kind in all four lane positions of a 16-byte group."""
  gen = torch.Generator(device=device).manual_seed(seed)
  b = n // 5 if n >= 10 else 0
  h = n - b
  u = h + (1 if b else 0)
  vals = torch.randn(u, d, generator=gen, device=device)
  if b:
    vals[h] = -0.1 * vals[:h].mean(dim=0)
  vals[:, 3::7] = (vals[:, 3::7] * 2).round() / 2
  rowmap = list(range(h)) + [h] * b

  def inject(col, kind):
    col = int(col)
    if kind == 0 or kind == 1:
      for t in range(f + kind):
        vals[(col + t) % h, col] = math.nan
    elif kind == 2:
      vals[col % h, col] = math.inf
      vals[(col + 1) % h, col] = -math.inf
    elif kind == 3:
      vals[:, col] = 0.0
      vals[1::2, col] = -0.0
    else:
      vals[::2, col] = math.inf

  for s in hot_starts(d):
    for kind in range(N_KINDS):
      for r in range(4):
        c = s + 16 * kind + 5 * r + 1
        if c < d - 8:
          inject(c, kind)
  for back, kind in ((1, 1), (2, 2), (3, 3), (4, 0), (5, 4)):
    if d - back >= 0:
      inject(d - back, kind)
  return vals, rowmap


def sample_columns(d):
  """Columns the references check: every column up to 64 K coordinates, else 1024 from each hot start plus the end
  (where the special values are)."""
  if d <= (1 << 16):
    return None
  idx = [torch.arange(s, s + 1024) for s in hot_starts(d)] + [torch.arange(d - 1024, d)]
  return torch.cat(idx)


# ---------------------------------------------------------------------------------------------------------------------
# References

def window_candidates(st, keep, centre):
  """(mean of the reference-legal window, ambiguous mask, list of alternative means) per column."""
  g = st.to(torch.float64)
  n, d = g.shape
  srt = g.sort(dim=0).values
  win, amb = O.closest_window(st, keep, centre)
  # alternatives: every contiguous window of `keep` sorted values (the topk result is always one of them
  # when deviations tie only at the window edges)
  csum = torch.cat([torch.zeros(1, d, dtype=torch.float64), srt.cumsum(dim=0)])
  alts = [(csum[s + keep] - csum[s]) / keep for s in range(n - keep + 1)]
  return win, amb, alts


def sorted_window(srt, keep, centre, eps):
  """float64 closest-to-centre window on the device from the column-sorted stack `srt` (n x d): (mean, tie) where tie
  marks columns with an excluded value within `eps` of as far from the centre as the window's edge (a last-bit
  difference of the centre may legitimately flip the choice there).  The window start is the number of leading values
  farther than their mirror (trmean.py:45-50 keeps the nearest)."""
  n, d = srt.shape
  dev = (srt - centre).abs()
  lo = torch.zeros(d, dtype=torch.long, device=srt.device)
  hi = torch.full((d,), n - 1, dtype=torch.long, device=srt.device)
  cols = torch.arange(d, device=srt.device)
  for _ in range(n - keep):
    drop_lo = dev[lo, cols] > dev[hi, cols]
    lo = torch.where(drop_lo, lo + 1, lo)
    hi = torch.where(drop_lo, hi, hi - 1)
  total = torch.zeros(d, dtype=torch.float64, device=srt.device)
  for k in range(keep):
    total += srt[lo + k, cols]
  tie = ((dev[(lo - 1).clamp(min=0), cols] - dev[hi, cols]).abs() <= eps) & (lo > 0) | \
        ((dev[(hi + 1).clamp(max=n - 1), cols] - dev[lo, cols]).abs() <= eps) & (hi < n - 1)
  return total / keep, tie


def closest_reference(st, rule, f):
  """float64 reference of phocas / meamed on the stack `st` (n x k float32, any device): (want, srt64).

  The centre is formed the way the library defines it — the trimmed mean as the fp32 sum of the sorted ranks
  f .. n-f-1 in ascending order, correctly rounded division; the lower median — and the window of the n - f values
  nearest it is chosen on fp32 deviations |x - c| (the last t < f whose value is farther than the one m places above
  starts the window after it, trmean.py:45-50); the window is then summed in float64.  NaNs sort last as +inf; the
  result is NaN where more than f values are NaN, where the centre is NaN (meamed: any NaN in the column) or where the
  float64 sum is."""
  n, k = st.shape
  keep = n - f
  isnan = torch.isnan(st)
  nan_count = isnan.sum(dim=0)
  s32 = torch.where(isnan, torch.full_like(st, math.inf), st).sort(dim=0).values
  if rule == PHOCAS:
    acc = torch.zeros(k, dtype=torch.float32, device=st.device)
    for i in range(f, n - f):
      acc = acc + s32[i]
    centre = (acc.double() / (n - 2 * f)).float()
    centre[nan_count > f] = math.nan
  else:
    centre = s32[(n - 1) // 2].clone()
    centre[nan_count > 0] = math.nan
  s = torch.zeros(k, dtype=torch.long, device=st.device)
  for t in range(f):
    s = torch.where((s32[t] - centre).abs() > (s32[t + keep] - centre).abs(), torch.full_like(s, t + 1), s)
  s64 = s32.double()
  cols = torch.arange(k, device=st.device)
  total = torch.zeros(k, dtype=torch.float64, device=st.device)
  for i in range(keep):
    total += s64[s + i, cols]
  want = total / keep
  want[(nan_count > f) | torch.isnan(centre)] = math.nan
  return want, s64, centre


def alternatives_ok(got, s64, centre, keep, tol):
  """Columns where an exact float64 deviation tie makes another window legal and `got` is that window's mean."""
  n, k = s64.shape
  dev = (s64 - centre.double()).abs()
  ok = torch.zeros(k, dtype=torch.bool, device=s64.device)
  for s in range(n - keep + 1):
    # window [s, s + keep) is legal if nothing outside is strictly nearer than something inside
    inside = dev[s:s + keep].max(dim=0).values
    outside = torch.cat([dev[:s], dev[s + keep:]]).min(dim=0).values if keep < n else torch.full_like(inside, math.inf)
    legal = outside >= inside
    mean = s64[s:s + keep].sum(dim=0) / keep
    ok |= legal & ((got == mean) | ((got - mean).abs() <= tol))
  return ok


def check_close(got, want, tol, scale):
  """(ok mask): NaN where want is NaN, the same infinity where want is infinite, else |got - want| <= tol *
  max(|want|, scale)."""
  got = got.double()
  want = want.double().to(got.device)
  nw, ng = torch.isnan(want), torch.isnan(got)
  inf = torch.isinf(want)
  fin = ~nw & ~inf
  ok = (nw & ng) | (inf & (got == want))
  bound = tol * torch.clamp(want.abs(), min=scale)
  ok |= fin & ~ng & ((got - want).abs() <= bound)
  return ok


def same_bits_strict(a, b):
  """Bit-for-bit equality of two float32 tensors (the sign of a zero and the NaN pattern included)."""
  return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def median_ok(got, st):
  """Bit-exact against the oracle's median (torch.median), except that where the median is a zero and the column
  holds zeros of both signs only its value is compared: which zero a sort returns first among equal keys is
  implementation-defined (torch's CPU sort and the kernels' min / max network differ there)."""
  want = O.median(list(st))
  got = got.cpu()
  zero = st == 0
  zero_tie = (want == 0) & (zero & torch.signbit(st)).any(dim=0) & (zero & ~torch.signbit(st)).any(dim=0)
  same = (got.view(torch.int32) == want.view(torch.int32)) | (torch.isnan(got) & torch.isnan(want))
  return same | (zero_tie & (got == 0))


def scale_of(st):
  fin = torch.isfinite(st)
  return float(st[fin].abs().max()) if bool(fin.any()) else 1.0


def check_colwise(rule, f, got, st):
  """The suite's bars for one coordinate-wise output `got` (float32, k columns) of the stack `st` (n x k float32,
  CPU): median bit-exact, trmean within 1e-6 scale of the oracle, phocas / meamed within 2e-6 scale of the float64
  window (or of another legal window at an exact tie).  Returns the mask of failing columns."""
  got = got.cpu()
  n = st.shape[0]
  if rule == MEDIAN:
    return ~median_ok(got, st)
  scale = scale_of(st)
  if rule == TRMEAN:
    return ~check_close(got, O.trmean(list(st), f), 1e-6, scale)
  want, s64, centre = closest_reference(st, rule, f)
  ok = check_close(got, want, 2e-6, scale)
  if not bool(ok.all()):
    bad = ~ok
    ok[bad] = alternatives_ok(got.double()[bad], s64[:, bad], centre[bad], n - f, 2e-6 * scale)
  return ~ok


# ---------------------------------------------------------------------------------------------------------------------
# Running one case (the knob digests and the GPU tests share this)

def _bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


def colwise_seed(case):
  return 7919 * case.n + 104729 * case.f + (1 if case.d == D_SHORT else case.d % 1000003)


def run_colwise(case, vals=None, rowmap=None):
  """(output, rows) of one coordinate-wise case."""
  bm = _bm()
  if vals is None:
    vals, rowmap = colwise_values(case.n, case.d, case.f, colwise_seed(case))
  rows = rows_of(place(vals, case.offset), rowmap)
  fn = getattr(bm.gars, case.rule)
  out = fn(rows) if case.rule == MEDIAN else fn(rows, case.f)
  return out, rows


def distinct_rows(rows):
  """(u x d tensor of the distinct rows of `rows` on the GPU, rowmap) — aliased entries of `rows` map to one row."""
  distinct, rowmap, seen = [], [], {}
  for g in rows:
    if id(g) not in seen:
      seen[id(g)] = len(distinct)
      distinct.append(g)
    rowmap.append(seen[id(g)])
  return torch.stack(distinct).to("cuda:0"), rowmap


def bulyan_stack(n, f, d):
  """(rows on the host, honest count, distinct rows on the GPU, rowmap): O.make_stack's hetero stack."""
  rows, h = O.make_stack("hetero", n, f, d, seed=13 * n + f + d % 97)
  return (rows, h) + distinct_rows(rows)


def run_bulyan(case, stack=None):
  """(output, ranking, rows on the device) of one Bulyan case."""
  bm = _bm()
  if stack is None:
    stack = bulyan_stack(case.n, case.f, case.d)
  _, _, distinct, rowmap = stack
  dev = rows_of(place(distinct, case.offset), rowmap)
  bm.gars.invalidate_rank_cache()
  ranking = bm.gars.bulyan_ranking(dev, case.f, case.m)
  return bm.bulyan(dev, case.f, case.m), ranking, dev


def aksel_pass1(rows):
  """bm_aksel_pass1 with its median output: (median float32[d], squared distances float64[n])."""
  from byzantinemomentum_amd import _lib, gars
  n, d, device = gars._validate(rows)
  lib = _lib.load()
  med = torch.empty(d, dtype=torch.float32, device=device)
  sq = torch.empty(_lib.MAX_ROWS, dtype=torch.float64, device=device)
  ws = gars._workspace(device, _lib.WS_AKSEL, n, d, "ws_aksel")
  with torch.cuda.device(device):
    _lib.check(lib.bm_aksel_pass1(_lib.pointer_table(rows), n, d, gars._ptr(med), gars._ptr(sq), gars._ptr(ws),
                                  gars._stream(device)), "bm_aksel_pass1")
  return med, sq[:n]


def aksel_stack(n, d):
  rows, h = O.make_stack("hetero", n, n // 5, d, seed=31 * n + 5)
  return (rows,) + distinct_rows(rows)


def run_aksel(case, stack=None):
  """(median output, squared distances, selection, aksel output, rows on the device) of one Aksel case."""
  bm = _bm()
  if stack is None:
    stack = aksel_stack(case.n, case.d)
  _, distinct, rowmap = stack
  dev = rows_of(place(distinct, case.offset), rowmap)
  med, sq = aksel_pass1(dev)
  bm.gars.invalidate_rank_cache()
  sel = bm.gars.aksel_selection(dev, case.n // 5)
  return med, sq, sel, bm.aksel(dev, case.n // 5), dev


def _sha(t):
  return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def digests(group, cus, check=None):
  """{case: SHA-256 of its output(s)} for the cases of a knob group, under the knobs of THIS process.  `check(case,
  output, rows)` is called on every colwise output (the parent validates what it hashes)."""
  out = {}
  for case in cases(group, cus):
    key = "/".join(str(x) for x in (case.kernel, case.rule, case.n, case.f, case.m, case.offset, case.d))
    if case.kernel == "colwise":
      res, rows = run_colwise(case)
      if check is not None:
        check(case, res, rows)
      out[key] = _sha(res)
    elif case.kernel == "bulyan":
      res, ranking, _ = run_bulyan(case)
      out[key] = _sha(res) + ":" + ",".join(map(str, ranking))
    elif case.kernel == "aksel":
      med, _, sel, _, _ = run_aksel(case)
      out[key] = _sha(med) + ":" + ",".join(map(str, sel))
    else:
      raise ValueError(case.kernel)
  return out


if __name__ == "__main__":
  torch.cuda.init()
  group = sys.argv[1]
  res = digests(group, torch.cuda.get_device_properties(0).multi_processor_count)
  torch.cuda.synchronize()
  print(json.dumps({"group": group, "knobs": {k: os.environ.get(k) for k in DEFAULT_KNOBS}, "digests": res}))
