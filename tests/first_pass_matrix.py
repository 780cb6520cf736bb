"""Which compiled instance of the step's first pass a call lands in, seeded inputs that reach every instance, and the
expected results computed from the inputs alone (a helper module, not a conftest).

The first pass (csrc/step.hip) compiles into 144 device instances and a call chooses among them at run time, invisibly
to the caller:
  * momentum_stats_kernel without a rule: T = 8, 12 (EXACT or with row predicates), 14, 20 (EXACT only) x VEC 4 / 2 / 1
    x CLIP x BURST                                                                                        72 instances
  * momentum_stats_stream_kernel: T = 20, 40, 64 x VEC x CLIP                                             18
  * momentum_stats_kernel with a rule riding along: (T, NB) = (20, 5), (14, 11) x four rules x
    {no clip, CLIP, NOMOM} x BURST                                                                        48
  * momentum_gram_kernel: TT = 20, 14 x {no clip, CLIP, NOMOM}                                             6
plus tail_gram_kernel, step_finish_kernel and the body / tail cut of for_body_and_tail.  The load / clip / momentum
prologue, the column statistics and the epilogue exist once per kernel, so a column must give the same results
whichever instance computed it.

Three parts, as in tests/instance_matrix.py and tests/distance_matrix.py:
  * a mirror of the dispatch rules: `instances(case, cus)` returns the (kernel, T, VEC, EXACT, CLIP, BURST, RULE, NB,
    NOMOM) tuples a call of one of the five entry points launches; tests/test_first_pass_matrix_cpu.py holds the mirror
    to the sources and the case lists to the 144 instances;
  * seeded case generators: the rows of a case are cut from ONE flat allocation (instance_matrix.place) at byte offset
    0, 4, 8, 12 or "mixed", the same values at every offset;
  * the expected results, in torch on the CPU, never derived from a kernel output:
      - bit for bit: the clipped gradients (one fp32 multiply), the momentum buffers (an fma, emulated in float64 with
        the fp32 midpoints of the float64 sum exempted and held to 1 ulp), both averages (sequential fp32 sums from row
        0, one true division), the `empire` vector (two fp32 operations), max|avg|;
      - in float64: the four sums (centred at the expected fp32 average, as tools/pytorch.py:97-125 does), the
        `little` vector, the rule riding along (instance_matrix's references), the n x n squared distances.
    With the `little` attack the rule and the distances read the Byzantine vector the call returned, AFTER that vector
    has itself been held to its bar (its fp32 value is not determined to the last bit by the inputs; the rules' bars are
    tighter than the vector's).

`python tests/first_pass_matrix.py GROUP [PART]` runs GROUP's cases in this process under the BM_* knobs of the
environment (read once per process), holds them to the same bars and prints one JSON line: failures, a SHA-256 per
output, the worst errors seen.
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
from tests import instance_matrix as M  # noqa: E402
from tests import distance_matrix as D  # noqa: E402

# ---------------------------------------------------------------------------------------------------------------------
# Mirror of the dispatch rules (step.hip, launch_plan.h, bm_common.h)

BM_MAX_ROWS = 64
K_STEP_BLOCK = 256
K_STEP_BURST_BLOCK = 512
K_STEP_PIECE_CAP = 2047
K_MAX_COLS_PER_LAUNCH = 1 << 29
REGISTER_TIERS = (8, 12)            # dispatch_momentum_stats: t <= 8, t <= 12 (row predicates allowed)
EXACT_TIERS = (14, 20)              # ks == h == T only
STREAM_TIERS = (20, 40, 64)
FUSED_RULE_SHAPES = ((20, 5), (14, 11))                   # fused_rule_shape (h, nb)
NOMOM_SHAPES = tuple((20, nb) for nb in range(1, 7)) + ((14, 11),)  # nomom_shape (k, nb): the distance fusion without buffers
SQDIST_SHAPES = tuple((20, nb) for nb in range(1, 7)) + ((14, 11),)  # shape_ok of bm_momentum_stats_sqdist (ks == h)
RULES = M.RULES

DEFAULT_KNOBS = {"BM_STEP_BURST": 8, "BM_STEP_STREAM": 0}

ENTRIES = ("ms", "ms_colwise", "ms_sqdist", "ss_colwise", "ss_sqdist")  # bm_momentum_stats[_colwise|_sqdist], bm_stack_stats_*

# A case: one call of one entry point.
#   ks, h: sampled rows, buffers (ss_*: ks == h == the stack, no buffers); nb: Byzantine copies; rule, rule_f: the rule
#   riding along; clip: clipping factors present; attack, scale, direction; offset: as instance_matrix; kind: "iid" or
#   "momentum"; bad: None or (value, "s" | "b", row, column): one non-finite coordinate; null: None or the output that
#   is NULL; knobs: the BM_* values the case's process runs with.
Case = namedtuple("Case", "group entry ks h nb rule rule_f clip attack scale direction offset d d_total kind bad null knobs")


def stream_grid(work, block=K_STEP_BLOCK, cap=K_STEP_PIECE_CAP):
  return max(1, min(cap, (work + block - 1) // block))


def plan(vec, d):
  """for_body_and_tail<4>(Tail::kOwnLaunch, vec, d, kStepBlock, caps_of(kStepPieceCap)): [(VEC, vectors, grid)]."""
  assert d <= K_MAX_COLS_PER_LAUNCH  # longer passes are cut into pieces (not covered here)
  vec = min(vec, 4)
  if d // vec == 0:
    vec = 1
  out, body = [], 0
  if d > 0 and vec > 1:
    nvec = d // vec
    body = nvec * vec
    out.append((vec, nvec, stream_grid(nvec)))
  if body < d:
    out.append((1, d - body, stream_grid(d - body) if body == 0 else 1))
  return out


def burst_ready(nvec, cus, knobs):
  return knobs["BM_STEP_BURST"] > 0 and nvec // (cus * K_STEP_BURST_BLOCK) >= knobs["BM_STEP_BURST"]


def burst_form(nvec, grid, cus, knobs):
  """launch_momentum_stats_form: the burst form once every CU has BM_STEP_BURST iterations and the plain grid is larger."""
  return burst_ready(nvec, cus, knobs) and cus < grid


def fused_rule_shape(h, nb):
  return (h, nb) in FUSED_RULE_SHAPES


def nomom_shape(k, nb):
  return (k, nb) in NOMOM_SHAPES


def sqdist_shape(ks, h, nb):
  return ks == h and (h, nb) in SQDIST_SHAPES


def dispatch(vec, ks, h, clip, nvec, grid, cus, knobs):
  """dispatch_momentum_stats<VEC>: one instance."""
  t = max(ks, h)
  if knobs["BM_STEP_STREAM"] != 1:
    tier = None
    for r in REGISTER_TIERS:
      if tier is None and t <= r:
        tier = r
    for r in EXACT_TIERS:
      if tier is None and ks == r and h == r:
        tier = r
    if tier is not None:
      return ("stats", tier, vec, ks == tier and h == tier, clip, burst_form(nvec, grid, cus, knobs), None, 0, False)
  tier = [r for r in STREAM_TIERS if t <= r][0]
  return ("stream", tier, vec, False, clip, False, None, 0, False)


def case_rows(case):
  """Distinct input rows of a case: the sampled gradients, then the buffers."""
  return case.ks if case.entry.startswith("ss") else case.ks + case.h


def case_vec(case):
  """Alignment::vec over the row tables (the outputs are fresh allocations)."""
  return M.vec_width(M.row_offsets(case.offset, case_rows(case)))


def is_fused(case, cus):
  """Whether the call takes its fused kernel (the rule or the Gram inside the first pass) for its 16-byte body."""
  knobs = dict(DEFAULT_KNOBS, **dict(case.knobs))
  vec, d = case_vec(case), case.d
  stream = knobs["BM_STEP_STREAM"] == 1
  if case.entry == "ms_colwise":
    return not stream and case.ks == case.h and fused_rule_shape(case.h, case.nb) and vec == 4 and d >= 4
  if case.entry == "ss_colwise":
    return fused_rule_shape(case.ks, case.nb) and vec == 4 and d % 4 == 0 and 0 < d <= K_MAX_COLS_PER_LAUNCH and not stream
  if case.entry == "ms_sqdist":
    return (sqdist_shape(case.ks, case.h, case.nb) and vec == 4 and case.null != "honest_avg" and
            d <= K_MAX_COLS_PER_LAUNCH and not stream and burst_ready(d // 4, cus, knobs))
  if case.entry == "ss_sqdist":
    return (nomom_shape(case.ks, case.nb) and vec == 4 and d % 4 == 0 and d <= K_MAX_COLS_PER_LAUNCH and not stream and
            burst_ready(d // 4, cus, knobs))
  return False


def instances(case, cus=256):
  """The (kernel, T, VEC, EXACT, CLIP, BURST, RULE, NB, NOMOM) instances the call of `case` launches under the case's
  knobs on a device with `cus` compute units, body and tail launch included.  kernel: "stats" (momentum_stats_kernel),
  "stream", "gram", "tail_gram" (T = its 1..3 columns).  The fall-back kernels outside the family (bm_stack_stats,
  bm_colwise, the stand-alone distance pass) are not listed."""
  knobs = dict(DEFAULT_KNOBS, **dict(case.knobs))
  vec, d, ks, h, clip = case_vec(case), case.d, case.ks, case.h, case.clip
  fused = is_fused(case, cus)
  out = set()
  if case.entry in ("ms", "ms_colwise") or (case.entry == "ms_sqdist" and not fused):
    for v, nvec, grid in plan(vec, d):
      if v == 4 and fused:
        out.add(("stats", h, 4, True, clip, burst_form(nvec, grid, cus, knobs), case.rule, case.nb, False))
      else:
        out.add(dispatch(v, ks, h, clip, nvec, grid, cus, knobs))
  elif case.entry == "ss_colwise":
    if fused:
      for v, nvec, grid in plan(vec, d):
        out.add(("stats", ks, 4, True, False, burst_form(nvec, grid, cus, knobs), case.rule, case.nb, True))
  elif case.entry == "ms_sqdist":
    for v, nvec, grid in plan(vec, d):
      if v == 4:
        out.add(("gram", h, 4, True, clip, True, None, 0, False))
      else:
        out.add(dispatch(1, ks, h, clip, nvec, grid, cus, knobs))
        out.add(("tail_gram", nvec, 1, False, False, False, None, 0, False))
  elif case.entry == "ss_sqdist":
    if fused:
      out.add(("gram", ks, 4, True, False, True, None, 0, True))
  else:
    raise ValueError(case.entry)
  return out


def source_instances():
  """Every instance the sources can instantiate (the table of the module docstring): 72 + 18 + 48 + 6 = 144."""
  out = set()
  for vec in (4, 2, 1):
    for clip in (False, True):
      for burst in (False, True):
        for t in REGISTER_TIERS:
          for exact in (False, True):
            out.add(("stats", t, vec, exact, clip, burst, None, 0, False))
        for t in EXACT_TIERS:
          out.add(("stats", t, vec, True, clip, burst, None, 0, False))
      for t in STREAM_TIERS:
        out.add(("stream", t, vec, False, clip, False, None, 0, False))
  for t, nb in FUSED_RULE_SHAPES:
    for rule in RULES:
      for clip, nomom in ((False, False), (True, False), (False, True)):
        for burst in (False, True):
          out.add(("stats", t, 4, True, clip, burst, rule, nb, nomom))
    for clip, nomom in ((False, False), (True, False), (False, True)):
      out.add(("gram", t, 4, True, clip, True, None, 0, nomom))
  return out


# ---------------------------------------------------------------------------------------------------------------------
# The case lists (every GPU test of tests/test_gpu_first_pass_matrix.py runs exactly the cases of its group and part)

OFFSETS = (0, 4, 8, 12, "mixed")
D_PLAIN = (0, 1, 3, 4, 5, 255, 1024 + 3, 4 * 256 * 3 + 2)  # tail alone, body alone, body + tail of 1..3, several workgroups
D_BAD = 1024 + 3                                           # the non-finite variants: a body and a 3-column tail
D_RULE = 4 * 256 * 3
REGISTER_SHAPES = {8: ((1, 1), (3, 3), (8, 8), (8, 5)), 12: ((9, 9), (12, 12), (12, 7), (11, 9)), 14: ((14, 14),),
                   20: ((20, 20),)}
STREAM_SHAPES = {20: ((13, 13), (14, 13), (20, 19), (20, 17), (19, 1)),
                 40: ((21, 21), (22, 21), (40, 40), (40, 37), (39, 4)),
                 64: ((41, 41), (64, 64), (64, 50), (64, 1))}
ATTACKS = (("empire", 1.1), ("little", -1.5))
BAD_VALUES = ("nan", "inf", "-inf")
RULE_SHAPES = ((20, 20, 5), (14, 14, 11))
RULE_NEIGHBOURS = ((20, 20, 4), (20, 20, 6), (14, 14, 10), (21, 20, 5))
SQDIST_CASES = ((20, 1), (20, 5), (20, 6), (14, 11))
BURST_ONLY = (("BM_STEP_BURST", 1),)
STREAM_ONLY = (("BM_STEP_STREAM", 1),)
NULLS = ("sampled_avg", "honest_avg", "byz")


def _case(group, entry, ks, h, **kw):
  base = dict(nb=0, rule=None, rule_f=0, clip=False, attack="empire", scale=1.1, direction=False, offset=0, d=D_BAD,
              d_total=None, kind="iid", bad=None, null=None, knobs=())
  base.update(kw)
  return Case(group, entry, ks, h, **base)


def bad_variants(ks, h, d, vec):
  """One NaN, +inf or -inf in turn: in a sampled row and in a buffer, in the first and the last lane of a vector of the
  body and in the scalar tail.  The row follows the value: NaN in the last row (a sampled-only row where ks > h), +inf
  in row 0 (the pivot of the streaming form), -inf in row 1."""
  body = d // vec * vec
  cols = list(dict.fromkeys([body // 2 // vec * vec, body // 2 // vec * vec + vec - 1, d - 1]))  # (VEC 1: the middle and the end)
  out = []
  for i, value in enumerate(BAD_VALUES):
    for where, count in (("s", ks), ("b", h)):
      row = (count - 1, 0, min(1, count - 1))[i]
      out += [(value, where, row, c) for c in cols]
  return out


def first_pass_cases(group, shapes, knobs=()):
  """Items 1 and 2: every shape x clipping x attack x offset x length, BM_ATTACK_DIRECTION at one length, and the
  non-finite variants at D_BAD."""
  out = []
  for ks, h in shapes:
    attacks = ATTACKS if h > 1 else ATTACKS[:1]  # the unbiased variance of one row is not defined
    for clip in (False, True):
      for d in D_PLAIN + ((D_BAD, True),):  # (the expected values are cached per input: offsets and attacks innermost)
        d, direction = d if isinstance(d, tuple) else (d, False)
        for attack, scale in attacks:
          for off in OFFSETS if d > 0 else OFFSETS[:1]:  # (an empty row has no address to misalign)
            out.append(_case(group, "ms", ks, h, clip=clip, attack=attack, scale=scale, offset=off, d=d,
                             direction=direction, knobs=knobs))
    for off in (0, 8, 4):
      vec = M.vec_width([off])
      for i, bad in enumerate(bad_variants(ks, h, D_BAD, vec)):
        attack, scale = attacks[i % len(attacks)]
        out.append(_case(group, "ms", ks, h, clip=True, attack=attack, scale=scale, offset=off, d=D_BAD, bad=bad,
                         knobs=knobs))
  return out


def burst_lengths(vec, cus):
  """Exactly one iteration of the burst form per CU, and one iteration and a ragged second with a scalar tail."""
  one = vec * cus * K_STEP_BURST_BLOCK
  return (one, one + vec * (K_STEP_BURST_BLOCK * 3 + 70) + (vec - 1))


BURST_SHAPES = tuple(s for t in REGISTER_SHAPES for s in REGISTER_SHAPES[t] if s[1] >= 3)


def rule_fs(rule, h, nb):
  if rule == M.MEDIAN:
    return (0,)
  if (h, nb) == (20, 5):
    return tuple(range(1, (h + nb - 1) // 2 + 1))  # every legal rule_f: n >= 2 f + 1
  return (5, 11)


def rule_main_f(rule, nb):
  return 0 if rule == M.MEDIAN else min(nb, 11)


RULE_MODES = (("ms_colwise", False), ("ms_colwise", True), ("ss_colwise", False))  # no clip, CLIP, NOMOM


def rule_case(group, mode, ks, h, nb, rule, f, attack, scale, d, offset=0, knobs=()):
  entry, clip = mode
  return _case(group, entry, ks, h, nb=nb, rule=rule, rule_f=f, clip=clip, attack=attack, scale=scale, d=d, offset=offset,
               knobs=knobs)


def cases(group, cus=256, part=None):
  out = []
  if group == "register":
    tiers = REGISTER_SHAPES if part is None else {part: REGISTER_SHAPES[part]}
    for t in tiers:
      out += first_pass_cases(group, REGISTER_SHAPES[t])
  elif group == "stream":
    tiers = STREAM_SHAPES if part is None else {part: STREAM_SHAPES[part]}
    for t in tiers:
      out += first_pass_cases(group, STREAM_SHAPES[t])
  elif group == "knob_stream":  # item 2: the register shapes in the streaming form
    tiers = REGISTER_SHAPES if part is None else {part: REGISTER_SHAPES[part]}
    for t in tiers:
      out += first_pass_cases(group, REGISTER_SHAPES[t], STREAM_ONLY)
  elif group == "knob_burst":  # item 3
    for ks, h in BURST_SHAPES if part is None else (BURST_SHAPES[part],):
      for clip, (attack, scale) in zip((False, True), ATTACKS):
        for off in OFFSETS:
          vec = M.vec_width(M.row_offsets(off, ks + h))
          for d in burst_lengths(vec, cus):
            out.append(_case(group, "ms", ks, h, clip=clip, attack=attack, scale=scale, offset=off, d=d, knobs=BURST_ONLY))
  elif group in ("rule", "knob_burst_rule"):  # item 4
    burst = group == "knob_burst_rule"
    knobs = BURST_ONLY if burst else ()
    lengths = burst_lengths(4, cus) if burst else (D_RULE, D_RULE + 3)
    for ks, h, nb in RULE_SHAPES if part is None else (RULE_SHAPES[part],):
      for rule in RULES:
        for mode in RULE_MODES:
          for d in lengths:
            if burst:
              attack, scale = ATTACKS[RULES.index(rule) % 2]
              out.append(rule_case(group, mode, ks, h, nb, rule, rule_main_f(rule, nb), attack, scale, d, knobs=knobs))
              continue
            for f in rule_fs(rule, h, nb):
              out.append(rule_case(group, mode, ks, h, nb, rule, f, "empire", 1.1, d))
            out.append(rule_case(group, mode, ks, h, nb, rule, rule_main_f(rule, nb), "little", -1.5, d))
    if not burst:  # the neighbours that take the two-kernel fall-back (NOMOM with d % 4 != 0 is among the cases above)
      for rule in RULES:
        for i, (ks, h, nb) in enumerate(RULE_NEIGHBOURS):
          attack, scale = ATTACKS[i % 2]
          for mode in RULE_MODES[:2] + (RULE_MODES[2:] if ks == h else ()):
            out.append(rule_case(group, mode, ks, h, nb, rule, rule_main_f(rule, nb), attack, scale, D_RULE + 3))
        for mode in RULE_MODES:
          out.append(rule_case(group, mode, 20, 20, 5, rule, rule_main_f(rule, 5), "empire", 1.1, D_RULE, offset=8))
  elif group == "knob_burst_sqdist":  # item 5
    one = cus * 4 * K_STEP_BURST_BLOCK
    ragged = one + 2048 * 3 + 256 + 132
    modes = (("ms_sqdist", False, ATTACKS[0]), ("ms_sqdist", True, ATTACKS[1]), ("ss_sqdist", False, ATTACKS[0]))

    def sq(h, nb, entry, clip, attack, scale, d, **kw):
      return _case(group, entry, h, h, nb=nb, clip=clip, attack=attack, scale=scale, d=d, kind="momentum",
                   knobs=BURST_ONLY, **kw)

    for h, nb in SQDIST_CASES if part is None else SQDIST_CASES[part:part + 1]:
      for entry, clip, (attack, scale) in modes:
        for d in (one, ragged) + ((ragged + 1, ragged + 2, ragged + 3) if entry == "ms_sqdist" else ()):
          out.append(sq(h, nb, entry, clip, attack, scale, d))
      out.append(sq(h, nb, "ms_sqdist", False, "empire", 1.1, one, d_total=1 << 24))  # the other plane plan of the distance pass
      out.append(sq(h, nb, "ms_sqdist", False, "empire", 1.1, ragged + 3, bad=("nan", "s", 3, one // 2 + 1)))
    if part is None or part == len(SQDIST_CASES):  # more non-finite values, and the neighbours that take the two passes
      out.append(sq(20, 5, "ms_sqdist", False, "empire", 1.1, ragged + 3, bad=("inf", "b", 2, ragged + 2)))
      out.append(sq(20, 5, "ss_sqdist", False, "empire", 1.1, ragged, bad=("-inf", "s", 0, 7)))
      for entry, clip, (attack, scale) in modes:
        out.append(sq(20, 5, entry, clip, attack, scale, one, offset=8))  # 8-byte rows
        out.append(sq(20, 5, entry, clip, attack, scale, one - 4))        # one vector short of an iteration
      for entry in ("ms_sqdist", "ss_sqdist"):                            # 7 copies: no instance
        out.append(sq(20, 7, entry, False, "empire", 1.1, one))
  elif group == "null":  # item 6
    for ks, h in ((8, 8), (20, 20), (21, 21)):
      for null in (None,) + NULLS:
        for attack, scale in ATTACKS:
          out.append(_case(group, "ms", ks, h, clip=True, attack=attack, scale=scale, d=4 * 256 * 3 + 2, null=null))
  else:
    raise ValueError(group)
  return out


GROUPS = ("register", "stream", "knob_stream", "knob_burst", "rule", "knob_burst_rule", "knob_burst_sqdist", "null")
PARTS = {"register": tuple(REGISTER_SHAPES), "stream": tuple(STREAM_SHAPES), "knob_stream": tuple(REGISTER_SHAPES),
         "knob_burst": tuple(range(len(BURST_SHAPES))), "knob_burst_rule": tuple(range(len(RULE_SHAPES))),
         "knob_burst_sqdist": tuple(range(len(SQDIST_CASES) + 1))}


def all_cases(cus=256):
  return [c for g in GROUPS for c in cases(g, cus)]


def case_key(case):
  """The case without its group and knobs: a knob's child and the parent at the defaults name a case alike."""
  return "/".join(str(x) for x in case[1:-1])


# ---------------------------------------------------------------------------------------------------------------------
# Seeded inputs (on the CPU; the same values at every offset, clipping mode and attack)

F32 = torch.float32
_VALUES = {}


def coefficients(case):
  """(mu, 1 - dampening) of a case."""
  return (0.99, 0.01) if case.kind == "momentum" else (0.9, 0.1)


# A draw whose float64 fma sums hold more fp32 midpoints than MIDPOINT_CAP allows takes another seed (randn returns
# values of few mantissa bits now and then, whose products are short: midpoints are more frequent than 2^-29).
SEED_SALT = {(12, 7, "iid", 393216): 1, (20, 19, "iid", 3074): 1}  # (ks, h, kind, length of the draw): found on the CPU


def seed_of(ks, h, kind, d):
  return 1009 * ks + 31 * h + (7 if kind == "momentum" else 0) + d % 10007 + 100003 * SEED_SALT.get((ks, h, kind, d), 0)


def clean_values(ks, h, kind, d):
  """(sampled ks x d, buffers h x d) float32: `iid` randn rows; `momentum` the drift + noise stack of
  test_first_pass_with_the_distance_pass_riding_along.  Lengths up to the longest of D_PLAIN share one draw, and so do
  the long lengths of one 128 K bucket (the two burst lengths of a width, the lengths of the distance cases)."""
  full = max(D_PLAIN) if d <= max(D_PLAIN) else -(-(d + 8192) // (1 << 17)) * (1 << 17)
  key = (ks, h, kind, full)
  if key not in _VALUES:
    _VALUES.clear()
    gen = torch.Generator().manual_seed(seed_of(ks, h, kind, full))
    if kind == "iid":
      s = torch.randn(ks, full, generator=gen)
      b = torch.randn(h, full, generator=gen)
    else:
      drift = 0.1 * torch.randn(full, generator=gen)
      s = drift + torch.linspace(0.5, 1.5, ks)[:, None] * torch.randn(ks, full, generator=gen)
      b = 0.3 * drift + 0.05 * torch.randn(h, full, generator=gen)
    _VALUES[key] = (s, b)
  s, b = _VALUES[key]
  return s[:, :d], b[:, :d]


BAD = {"nan": math.nan, "inf": math.inf, "-inf": -math.inf}


def values(case):
  """(sampled, buffers or None, clipping factors float32[64] or None) of a case, on the CPU."""
  s, b = clean_values(case.ks, case.h, case.kind, case.d)
  if case.bad is not None:
    value, where, row, col = case.bad
    s, b = s.clone(), b.clone()
    (s if where == "s" else b)[row, col] = BAD[value]
  factors = None
  if case.clip:
    factors = torch.ones(BM_MAX_ROWS)
    factors[min(1, case.ks - 1)] = 0.5
    factors[case.ks - 1] = 0.25
  return s, (None if case.entry.startswith("ss") else b), factors


# ---------------------------------------------------------------------------------------------------------------------
# The expected results, from the inputs alone

MIDPOINT_CAP = 1e-6  # of the elements of a case (expected: 2^-29 each)


def clipped(s, factors):
  """g_i * cf_i: one fp32 multiply."""
  return s if factors is None else s * factors[:s.shape[0], None]


def fma_emulated(omd, g, mu, b):
  """(float32(float64(omd) * float64(g) + float64(fl32(mu * b))), midpoint mask).  The product is exact in float64; the
  two roundings (to float64, then to fp32) can differ from the one rounding of an fma only where the float64 sum is
  exactly halfway between two fp32 numbers: the low 29 bits of its mantissa are 0x10000000."""
  mub = b * torch.tensor(mu, dtype=F32)
  ref = torch.tensor(omd, dtype=F32).double() * g.double() + mub.double()
  mid = (ref.view(torch.int64) & 0x1FFFFFFF) == 0x10000000
  return ref.float(), mid & torch.isfinite(ref)


def seq_avg(rows):
  """Sequential fp32 sum in row order from row 0, one true division by float(k)."""
  acc = rows[0].clone()
  for i in range(1, rows.shape[0]):
    acc.add_(rows[i])
  return acc.div_(rows.shape[0])


def sums64(rows, avg):
  """(sum avg^2, sum_i ||x_i - avg||^2) in float64, centred at the fp32 average `avg` (tools/pytorch.py:97-125)."""
  a = avg.double()
  dev = 0.0
  for i in range(rows.shape[0]):
    diff = rows[i].double() - a
    dev += float((diff * diff).sum())
  return float((a * a).sum()), dev


def abs_max(avg):
  """torch's avg.abs().max(): NaN whenever the average holds a NaN; 0 for an empty average."""
  if avg.numel() == 0:
    return 0.0
  return math.nan if bool(torch.isnan(avg).any()) else float(avg.abs().max())


def byzantine(avg, rows, attack, scale, direction):
  """(the Byzantine vector, whether its bits are determined): `empire` avg + (-avg) * scale, two fp32 operations;
  `little` avg + scale * sqrt(unbiased column variance) in float64.  BM_ATTACK_DIRECTION: the product alone."""
  if attack == "empire":
    att = avg.neg().mul_(torch.tensor(scale, dtype=F32))
    return (att if direction else avg.add(att)), True
  att = scale * rows.double().var(dim=0, unbiased=True).sqrt() if rows.shape[1] else torch.zeros(0, dtype=torch.float64)
  return (att if direction else avg.double() + att), False


Expected = namedtuple("Expected", "g buffers mid s_avg h_avg sums_s sums_h max_s max_h")
_EXPECTED = {}


def expected(case):
  """Everything of a case that does not depend on the attack, cached over the offsets and attacks of one input."""
  key = (case.entry.startswith("ss"), case.ks, case.h, case.kind, case.d, case.clip, case.bad)
  if key not in _EXPECTED:
    _EXPECTED.clear()
    s, b, factors = values(case)
    g = clipped(s, factors)
    if b is None:
      buffers, mid = g, torch.zeros_like(g, dtype=torch.bool)
    else:
      mu, omd = coefficients(case)
      buffers, mid = fma_emulated(omd, g[:case.h], mu, b)
    s_avg, h_avg = seq_avg(g), seq_avg(buffers)
    _EXPECTED[key] = Expected(g, buffers, mid, s_avg, h_avg, sums64(g, s_avg), sums64(buffers, h_avg), abs_max(s_avg),
                              abs_max(h_avg))
  return _EXPECTED[key]


def midpoints(case):
  """(midpoint elements of the case, elements)."""
  e = expected(case)
  return int(e.mid.sum()), e.mid.numel()


# ---------------------------------------------------------------------------------------------------------------------
# Running one case on the GPU

DEV = "cuda:0"
_ATTACK_ID = {"empire": 0, "little": 1}
_DIRECTION = 16


def _bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


def momentum_stats_abi(sampled, buffers, mu, omd, factors, scale, attack, direction, null):
  """bm_momentum_stats through the C ABI, `null` (None or one of NULLS) passed as a NULL pointer."""
  import ctypes
  from byzantinemomentum_amd import _lib, gars
  ks, d, device = gars._validate(list(sampled))
  lib = _lib.load()
  outs = {name: (None if name == null else torch.empty(d, dtype=F32, device=device)) for name in NULLS}
  out6 = torch.empty(6, dtype=torch.float64, device=device)
  ws = gars._workspace(device, _lib.WS_STEP, 1, d, "ws_step")
  gars.invalidate_rank_cache()

  def opt(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)

  with torch.cuda.device(device):
    _lib.check(lib.bm_momentum_stats(
      _lib.pointer_table(sampled), ks, _lib.pointer_table(buffers), len(buffers), d, ctypes.c_float(mu),
      ctypes.c_float(omd), opt(factors), opt(outs["sampled_avg"]), opt(outs["honest_avg"]), opt(outs["byz"]),
      ctypes.c_float(scale), _ATTACK_ID[attack] | (_DIRECTION if direction else 0), gars._ptr(out6), gars._ptr(ws),
      gars._stream(device)), "bm_momentum_stats")
  return outs["sampled_avg"], outs["honest_avg"], outs["byz"], out6


def run_case(case):
  """The outputs of one call, on the CPU: a dict of `buffers` (h x d, None without buffers), `sampled_avg`,
  `honest_avg`, `byz`, `defense`, `sq`, `out6` (a list) and `stray`: whether anything outside the buffers changed in
  the allocation the rows were cut from (the sampled rows, the gaps between rows)."""
  bm = _bm()
  s, b, factors = values(case)
  ks, h = case.ks, case.h
  stack = s if b is None else torch.cat([s, b])
  views = M.place(stack.to(DEV), case.offset)
  flat = views[0]._base
  before = flat.clone()
  sampled, buffers = views[:ks], views[ks:]
  fdev = factors.to(DEV) if factors is not None else None
  mu, omd = coefficients(case)
  out = dict.fromkeys(("buffers", "sampled_avg", "honest_avg", "byz", "defense", "sq"))
  if case.entry == "ms":
    out["sampled_avg"], out["honest_avg"], out["byz"], out6 = momentum_stats_abi(
      sampled, buffers, mu, omd, fdev, case.scale, case.attack, case.direction, case.null)
  elif case.entry == "ms_colwise":
    out["sampled_avg"], out["honest_avg"], out["byz"], out["defense"], out6 = bm.stats.momentum_stats_colwise(
      sampled, buffers, mu, omd, fdev, case.scale, case.attack, case.rule, case.rule_f, case.nb)
  elif case.entry == "ms_sqdist":
    out["sampled_avg"], out["honest_avg"], out["byz"], out["sq"], out6 = bm.stats.momentum_stats_sqdist(
      sampled, buffers, mu, omd, fdev, case.scale, case.attack, case.nb, case.d_total)
  elif case.entry == "ss_colwise":
    out["honest_avg"], out["byz"], out["defense"], out6 = bm.stats.stack_stats_colwise(
      sampled, case.scale, case.attack, case.rule, case.rule_f, case.nb)
  elif case.entry == "ss_sqdist":
    out["honest_avg"], out["byz"], out["sq"], out6 = bm.stats.stack_stats_sqdist(sampled, case.scale, case.attack,
                                                                                 case.nb, case.d_total)
  else:
    raise ValueError(case.entry)
  torch.cuda.synchronize()
  if buffers:
    out["buffers"] = torch.stack(buffers).cpu()
    for v in list(buffers) + _same_views(before, flat, buffers):  # what the call may write: the buffers
      v.zero_()
  out["stray"] = not torch.equal(flat.view(torch.int32), before.view(torch.int32))
  for name in ("sampled_avg", "honest_avg", "byz", "defense", "sq"):
    if out[name] is not None:
      out[name] = out[name].cpu()
  out["out6"] = out6.tolist()
  return out


def _same_views(copy, flat, views):
  """The slices of `copy` (a clone of `flat`) that the views of `flat` cover."""
  return [copy[v.storage_offset() - flat.storage_offset(): v.storage_offset() - flat.storage_offset() + v.numel()]
          for v in views]


# ---------------------------------------------------------------------------------------------------------------------
# The bars (the suite's own)

TOL_LITTLE = 4e-6   # of max|want|: test_momentum_stats_kernel_tiers
TOL_SUMS = 1e-5     # relative, on sqrt(sum avg^2), sqrt(sum dev^2 / (k - 1)): the same test
TOL_MIDPOINT_AVG = 2e-7  # of max|avg|, on the columns that hold a midpoint element: the same test's bar on h_avg
TOL_SQDIST = D.TOL  # pair_mode_check.py: relative to the distance itself
TOL_TIE = 1e-9      # rankings: float64 scores within this (relative) count as tied


class Worst:
  """Worst error seen per (kernel family, T, VEC, quantity), next to its bar.  Bit-exact quantities count mismatches
  (bar 0), `midpoints` counts the exempted elements against the elements seen."""

  def __init__(self):
    self.table = {}

  def add(self, key, quantity, value, bar):
    k = tuple(key) + (quantity,)
    if quantity == "midpoints":
      v, b = self.table.get(k, (0, 0))
      self.table[k] = (v + value, b + bar)
    elif bar == 0:
      self.table[k] = (self.table.get(k, (0, 0))[0] + value, 0)
    else:
      self.table[k] = (max(self.table.get(k, (0.0, bar))[0], value), bar)

  def merge(self, entries):
    for family, t, vec, quantity, value, bar in entries:
      self.add((family, t, vec), quantity, value, bar)

  def entries(self):
    return [list(k) + list(v) for k, v in sorted(self.table.items(), key=lambda kv: tuple(map(str, kv[0])))]

  def lines(self):
    out = []
    for family, t, vec, quantity, value, bar in self.entries():
      if quantity == "midpoints":
        out.append(f"{family:10s} T={t:2d} VEC={vec}  {quantity:12s} {int(value)} exempted of {int(bar)} elements "
                   f"(cap {MIDPOINT_CAP:g} of a case)")
      elif bar == 0:
        out.append(f"{family:10s} T={t:2d} VEC={vec}  {quantity:12s} {int(value)} mismatches  bit-exact")
      else:
        out.append(f"{family:10s} T={t:2d} VEC={vec}  {quantity:12s} worst error {value:.3e}  bar {bar:g}")
    return out


ERRORS = Worst()


def table_key(case, cus):
  """(family, T, VEC) of the instance that runs the body of the case; fall-backs outside the family under "other"."""
  inst = [i for i in instances(case, cus) if i[0] != "tail_gram"]
  if not inst:
    return ("other", max(case.ks, case.h), case_vec(case))
  kernel, t, vec = max(inst, key=lambda i: i[2])[:3]
  rule = max(inst, key=lambda i: i[2])[6]
  return (kernel + ("+rule" if rule else ""), t, vec)


def bits_differ(got, want):
  """Mask of elements whose bits differ (every NaN equals every NaN: the payload of a NaN is not specified)."""
  same = (got.view(torch.int32) == want.view(torch.int32)) | (torch.isnan(got) & torch.isnan(want))
  return ~same


def close(got, want, tol):
  """One number against its float64 value: NaN for NaN, the same infinity, else within tol relative."""
  if math.isnan(want):
    return math.isnan(got)
  if math.isinf(want):
    return got == want
  return abs(got - want) <= tol * abs(want)


def rel_error(got, want):
  if not math.isfinite(want) or not math.isfinite(got):
    return 0.0
  return abs(got - want) / abs(want) if want != 0 else (0.0 if got == 0 else math.inf)


def hot_columns(d, cus):
  """Columns a float64 rule reference checks at long lengths: the start, the end of the first iteration of the burst
  form at 16-byte columns, and the end."""
  if d <= (1 << 16):
    return None
  one = 4 * cus * K_STEP_BURST_BLOCK
  idx = [torch.arange(0, 2048), torch.arange(d - 2048, d)]
  if one + 1024 < d - 2048:
    idx.append(torch.arange(one - 1024, one + 1024))
  return torch.cat(idx)


def check_sqdist(case, sq, rows64, worst_key, worst):
  """The distance bars on `sq` (n x n float64) against the float64 direct differences of `rows64` (h + 1 distinct rows:
  the buffers and the Byzantine vector)."""
  h, nb = case.h, case.nb
  n = h + nb
  rowmap = list(range(h)) + [h] * nb
  u = rows64.shape[0]
  # direct differences in float64 (no Gram form, no cancellation)
  small = torch.cdist(rows64, rows64, compute_mode="donot_use_mm_for_euclid_dist") ** 2
  small = torch.maximum(small, small.T)  # (bitwise symmetric; NaN stays NaN)
  small.fill_diagonal_(0.0)
  idx = torch.tensor(rowmap)
  want = small[idx][:, idx]
  finite_row = torch.isfinite(rows64).all(dim=1)[idx]
  fails = []
  same = (sq.view(torch.int64) == sq.T.contiguous().view(torch.int64)) | (torch.isnan(sq) & torch.isnan(sq.T))
  if not bool(same.all()):
    fails.append("not bitwise symmetric")
  if not bool((sq.diagonal() == 0).all()):
    fails.append("non-zero diagonal")
  good = [i for i in range(n) if finite_row[i]]
  for i in range(n):
    if not finite_row[i]:
      others = [j for j in range(n) if rowmap[j] != rowmap[i]]
      if bool(torch.isfinite(sq[i, others]).any()):
        fails.append(f"a finite distance from the non-finite row {i}")
  gi = torch.tensor(good, dtype=torch.long)
  sub_fails, rel = D.check_matrix(sq[gi][:, gi].contiguous(), want[gi][:, gi], [rowmap[i] for i in good], TOL_SQDIST)
  fails += sub_fails
  if math.isfinite(rel):
    worst.add(worst_key, "sqdist", rel, TOL_SQDIST)
  if len(good) == n and not sub_fails:
    from tests.pair_mode_check import same_up_to_ties
    f, m = nb, n - nb - 2
    got_dist, want_dist = sq.sqrt().numpy(), want.sqrt().numpy()
    for name in ("krum", "bulyan"):
      def scores(dist):
        if name == "krum":
          return O.krum_scores(dist, f)
        return [O._sum_smallest([dist[i, j] for j in range(n) if j != i], m) for i in range(n)]
      s64 = scores(want_dist)
      if not same_up_to_ties(O._stable_order(scores(got_dist)), O._stable_order(s64), s64, TOL_TIE):
        fails.append(f"{name} ranking differs from the float64 matrix's")
  return fails


def check_case(case, got, cus, worst=ERRORS):
  """Hold the outputs of one call to the bars; returns the list of failures (strings)."""
  e = expected(case)
  key = table_key(case, cus)
  nomom = case.entry.startswith("ss")
  ks, h, d = case.ks, case.h, case.d
  fails = []

  def fail(text):
    fails.append(f"{case_key(case)}: {text}")

  nmid, nel = midpoints(case)
  worst.add(key, "midpoints", nmid, nel)
  if nmid > MIDPOINT_CAP * nel:
    fail(f"{nmid} midpoint elements of {nel}: pick another seed")
  midcols = e.mid.any(dim=0)
  if got["stray"]:
    fail("a store outside the buffers (sampled rows or the gaps between rows changed)")
  # bit-exact: buffers, averages, max|avg|
  if not nomom:
    differ = bits_differ(got["buffers"], e.buffers)
    bad = differ & ~e.mid
    worst.add(key, "buffers", int(bad.sum()), 0)
    if bool(bad.any()):
      r, c = [int(x) for x in torch.nonzero(bad)[0]]
      fail(f"buffers: {int(bad.sum())} elements differ, first [{r}, {c}] {got['buffers'][r, c].item()!r} for "
           f"{e.buffers[r, c].item()!r}")
    ulps = (got["buffers"].view(torch.int32)[e.mid].long() - e.buffers.view(torch.int32)[e.mid].long()).abs()
    if bool((ulps > 1).any()):
      fail("a midpoint element more than 1 ulp off")
  scale_h = float(e.h_avg[torch.isfinite(e.h_avg)].abs().max()) if bool(torch.isfinite(e.h_avg).any()) else 1.0

  def exact(name, value, want):
    if value is None:
      return
    differ = bits_differ(value, want)
    bad = differ & ~midcols if name != "sampled_avg" else differ
    worst.add(key, name, int(bad.sum()), 0)
    if bool(bad.any()):
      c = int(torch.nonzero(bad)[0])
      fail(f"{name}: {int(bad.sum())} columns differ, first [{c}] {value[c].item()!r} for {want[c].item()!r}")
    if name != "sampled_avg" and bool(midcols.any()):
      off = (value[midcols].double() - want[midcols].double()).abs()
      if not bool((off[torch.isfinite(off)] <= TOL_MIDPOINT_AVG * scale_h).all()):
        fail(f"{name}: a midpoint column off by more than {TOL_MIDPOINT_AVG:g} of the largest")

  for name in NULLS:
    if name == case.null and got[name] is not None:
      fail(f"{name} was to be NULL")
    if name != case.null and got[name] is None and not (nomom and name == "sampled_avg"):
      fail(f"{name} missing")
  exact("sampled_avg", got["sampled_avg"], e.s_avg)
  exact("honest_avg", got["honest_avg"], e.h_avg)
  # the Byzantine vector
  byz_want, byz_exact = byzantine(e.h_avg, e.buffers, case.attack, case.scale, case.direction)
  byz_ok = True
  if got["byz"] is not None:
    if byz_exact:
      before = len(fails)
      exact("byz", got["byz"], byz_want)
      byz_ok = len(fails) == before
    else:
      fin = torch.isfinite(byz_want)
      top = float(byz_want[fin].abs().max()) if bool(fin.any()) else 1.0
      g64 = got["byz"].double()
      ok = (torch.isnan(byz_want) & torch.isnan(g64)) | (torch.isinf(byz_want) & (g64 == byz_want))
      err = (g64 - byz_want).abs()
      ok |= fin & (err <= TOL_LITTLE * top)
      worst.add(key, "little", float(err[fin & torch.isfinite(g64)].max()) / top if bool((fin & torch.isfinite(g64)).any()) else 0.0,
                TOL_LITTLE)
      byz_ok = bool(ok.all())
      if not byz_ok:
        c = int(torch.nonzero(~ok)[0])
        fail(f"little: column {c} {got['byz'][c].item()!r} for {byz_want[c].item()!r} (bar {TOL_LITTLE:g} x {top:g})")
  # out6: the four sums within 1e-5 on the forms the suite compares, the two maxima exactly
  o = got["out6"]
  triples = (("s", 0, ks, e.sums_h if nomom else e.sums_s, e.max_h if nomom else e.max_s), ("h", 3, h, e.sums_h, e.max_h))
  for tag, at, k, (n2, dev), top in triples:
    forms = [("norm_" + tag, math.sqrt(o[at]) if o[at] >= 0 else o[at], math.sqrt(n2) if n2 >= 0 else n2)]
    if k > 1:
      forms.append(("dev_" + tag, math.sqrt(o[at + 1] / (k - 1)) if o[at + 1] >= 0 else o[at + 1],
                    math.sqrt(dev / (k - 1)) if dev >= 0 else dev))
    else:
      forms.append(("dev_" + tag, o[at + 1], dev))  # one row: its deviation from itself, 0 (NaN if it is not finite)
    for name, value, want in forms:
      worst.add(key, name, rel_error(value, want), TOL_SUMS)
      if not close(value, want, TOL_SUMS):
        fail(f"{name}: {value!r} for {want!r}")
    same = (math.isnan(o[at + 2]) and math.isnan(top)) or o[at + 2] == top
    if not same and bool(midcols.any()) and tag == "h":
      same = close(o[at + 2], top, TOL_MIDPOINT_AVG)
    worst.add(key, "max_" + tag, 0 if same else 1, 0)
    if not same:
      fail(f"max_{tag}: {o[at + 2]!r} for {top!r}")
  # the rule and the distances riding along
  if got["defense"] is not None or got["sq"] is not None:
    if got["byz"] is None or not byz_ok:
      fail("no verified Byzantine vector: the rule / the distances were not checked")
      return fails
    byz_used = byz_want if byz_exact else got["byz"]
  if got["defense"] is not None:
    cols = hot_columns(d, cus)
    keep = ~midcols if cols is None else ~midcols[cols]
    pick = (lambda t: t) if cols is None else (lambda t: t[..., cols])
    st = torch.cat([pick(e.buffers), pick(byz_used)[None].expand(case.nb, -1)])[:, keep].contiguous()
    out = pick(got["defense"])[keep].contiguous()
    bad = M.check_colwise(case.rule, case.rule_f, out, st)
    if case.rule == M.MEDIAN:
      worst.add(key, case.rule, int(bad.sum()), 0)
    else:  # the worst error among the columns held to the primary window (an exact tie may make another window legal)
      tol = 1e-6 if case.rule == M.TRMEAN else 2e-6
      want = O.trmean(list(st), case.rule_f) if case.rule == M.TRMEAN else M.closest_reference(st, case.rule, case.rule_f)[0]
      err = (out.double() - want.double()).abs() / torch.clamp(want.double().abs(), min=M.scale_of(st))
      err = err[torch.isfinite(err) & ~bad]
      err = err[err <= tol]
      worst.add(key, case.rule, float(err.max()) if err.numel() else 0.0, tol)
    if bool(bad.any()):
      fail(f"{case.rule} f={case.rule_f}: {int(bad.sum())} columns outside the bars of check_colwise")
  if got["sq"] is not None:
    rows64 = torch.cat([e.buffers.double(), byz_used.double()[None]])
    fails += [f"{case_key(case)}: {t}" for t in check_sqdist(case, got["sq"], rows64, key, worst)]
  return fails


# ---------------------------------------------------------------------------------------------------------------------
# Digests: what must keep its bits from one form to another

def _sha(t):
  return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def digest(case, got):
  """{output: SHA-256} of the outputs of a case that are bit-exact across the forms of the first pass: buffers, both
  averages, the two maxima, and (`empire`: in every form; `little`: between the plain and the burst form of one kernel,
  see comparable) the Byzantine vector and what is computed from it."""
  out = {}
  for name in ("buffers", "sampled_avg", "honest_avg", "byz", "defense"):
    if got[name] is not None:
      out[name] = _sha(got[name])
  out["max"] = _sha(torch.tensor([got["out6"][2], got["out6"][5]], dtype=torch.float64))
  return out


def comparable(case, name):
  """Whether output `name` of `case` must have the same bits under the case's knob as at the defaults.  The `little`
  vector takes its variance from a two-pass sum in the register form and from a pivot form in the streaming one, and
  without buffers the fall-back is another kernel (bm_stack_stats): there it is held to its bar only."""
  if name in ("byz", "defense") and case.attack == "little":
    knobs = dict(case.knobs)
    return knobs.get("BM_STEP_STREAM", 0) != 1 and not case.entry.startswith("ss")
  return True


def differing(todo, mine, theirs):
  """Cases and outputs whose digest under the knob (`theirs`) is not the one at the defaults (`mine`)."""
  out = []
  for c in todo:
    k = case_key(c)
    if set(mine[k]) != set(theirs[k]):
      out.append(f"{k}: outputs {sorted(mine[k])} against {sorted(theirs[k])}")
      continue
    out += [f"{k}: {name}" for name in mine[k] if comparable(c, name) and mine[k][name] != theirs[k][name]]
  return out


def sweep(todo, cus, worst=ERRORS, digests=None, check=True):
  """Run and check the cases of `todo`; returns the failures and fills `digests` {case key: {output: SHA-256}}.
  check=False: the digests alone (the default-knob side of a group whose forms are all held to the bars elsewhere)."""
  fails = []
  for case in todo:
    got = run_case(case)
    if check:
      fails += check_case(case, got, cus, worst)
    if digests is not None:
      digests[case_key(case)] = digest(case, got)
  return fails


if __name__ == "__main__":
  torch.cuda.init()
  group = sys.argv[1]
  part = int(sys.argv[2]) if len(sys.argv) > 2 else None
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  digests = {}
  failures = sweep(cases(group, cus, part), cus, ERRORS, digests)
  torch.cuda.synchronize()
  print(json.dumps({"group": group, "part": part, "knobs": {k: os.environ.get(k) for k in DEFAULT_KNOBS},
                    "digests": digests, "failures": failures, "worst": ERRORS.entries()}))
