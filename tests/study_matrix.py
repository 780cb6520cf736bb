"""Which compiled instance of the study block (csrc/study.hip) and of the plain stack statistics (csrc/reduce.hip) a
call lands in, seeded inputs that reach every instance, and the expected results computed from the inputs alone (a
helper module, not a conftest).

study.hip compiles into 72 device instances and a call chooses among them at run time, invisibly to the caller:
  * study_stats_kernel<ATT, CM, L2, VEC>: 2 x 4 x 2 x 3 = 48, each with a run-time momentum stream and a run-time
    attack-average output;
  * study_stats_burst_kernel<ATT, CM, L2, MOM>: 2 x 3 x 2 x 2 = 24; U = 2 column groups per lane and iteration (U = 1
    with (L2 and CM >= 2) or MOM), 8 staged iterations per burst (4 with MOM);
plus study_finish_kernel and the body / tail cut of for_body_and_tail.  reduce.hip's stack_stats_kernel<KMAX, VEC> has
12: KMAX 8 / 16 / 24 x VEC 4 / 2 / 1, <32, 2>, <32, 1>, <64, 1> (25..32 rows run 8-byte columns, more rows 4-byte ones,
on the grid of the wide count).

Three parts, as in tests/first_pass_matrix.py (whose pieces this module reuses: fma_emulated, seq_avg, sums64, abs_max,
byzantine, Worst, the bars, the digests):
  * a mirror of the dispatch rules: `instances(case, cus)` returns the instances a call launches, its launch plan and
    the number of partial sets the finish kernel adds; `plain_iterations`, `burst_shape` and `burst_iterations` give
    the per-lane structure the case generators derive their lengths from;
  * seeded case generators: the vectors of a case are cut from ONE flat allocation with NaN-filled guard gaps
    (place_at: instance_matrix.place with a byte offset per vector and a gap in front of the first one);
  * the expected results, in torch on the CPU, never derived from a kernel output:
      - bit for bit: the attack average (sequential fp32 sums, one true division), C (mode 1: s; mode 2:
        fl(s + fl(mu C)); mode 3: the leading fma(w, oldest, C) emulated in float64, its midpoint columns accepted at
        either neighbour), M (an emulated fma, midpoints held to 1 ulp), the stack average, the `empire` vector, all
        maxima, every zero slot, the guard gaps and the inputs;
      - in float64 at the suite's own bars: Gram, dots and l2 at 1e-6 of |a||b|, the deviation sums at 1e-5 centred at
        the expected fp32 average, `little` at 4e-6 of the largest.

A sum over d coordinates hides one coordinate once d is long, so every long case carries power-of-two spikes at its
edge coordinates E (`edges`: coordinate 0, the end of the 16-byte body, the tail, both ends of the last live
iteration of the first and the last workgroup, either side of a burst boundary), and the short cases keep their
values at E away from zero: dropping or doubling one coordinate of E moves every non-zero sum by ten bars or more
(`insensitive`, held by tests/test_study_matrix_cpu.py).

`python tests/study_matrix.py GROUP [PART]` runs GROUP's cases in this process under the BM_* knobs of the environment
(read once per process), holds them to the same bars and prints one JSON line: failures, a SHA-256 per output, the
worst errors seen.
"""

import json
import math
import os
import sys
from collections import namedtuple

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from tests import instance_matrix as M  # noqa: E402
from tests import first_pass_matrix as F  # noqa: E402

# ---------------------------------------------------------------------------------------------------------------------
# Mirror of the dispatch rules (study.hip, reduce.hip, launch_plan.h, bm_common.h)

BM_MAX_ROWS = 64
STUDY_SLOTS = 32
K_STUDY_BLOCK = 256
K_STUDY_MAX_BLOCKS = 2048
K_STUDY_FOLD = 16                  # the plain form folds its fp32 chains into fp64 every 16 iterations
K_STUDY_BURST_THREADS = 1024
K_STUDY_SLOT_BUDGET = 8
K_RED_BLOCK = 256
K_MAX_PARTIAL_BLOCKS = 2048
STUDY_CAPS = (K_STUDY_MAX_BLOCKS, K_STUDY_MAX_BLOCKS)                 # (body, tail)
STATS_CAPS = (K_MAX_PARTIAL_BLOCKS - 1, K_MAX_PARTIAL_BLOCKS)
STACK_TIERS = (8, 16, 24)          # dispatch_stack_stats at the pointers' width; then <32, min(VEC, 2)>, <64, 1>
DEFAULT_KNOBS = {"BM_STUDY_BURST": 8}

# the eleven pointers of bm_study_stats_update, in the order its Alignment takes them
ROLES = ("s", "h", "def", "byz", "past", "oldest", "params", "origin", "curv", "a_out", "mom")

# A case: one call.  kernel: "study" (bm_study_stats_update), "stack" (bm_stack_stats) or "aliased" (both, on f copies
# of one vector).  f: f_real, or the stack's row count; cm, l2, mom, a_out: the study block's terms; offset: byte offset
# of every vector (the stack: as instance_matrix.row_offsets); mis: None or (role, bytes): one pointer moved on;
# spiked: the edge coordinates carry power-of-two spikes (long cases); bad: None or (value, role, place); arg: None or
# the argument behaviour the case pins; attack .. scaled: the stack's outputs; idx: which spike is the largest.
Case = namedtuple("Case", "group kernel f cm l2 mom a_out offset mis d spiked bad arg attack scale direction avg scaled "
                          "knobs idx")
Launch = namedtuple("Launch", "form inst vec first count grid part")


def stream_grid(work, block, cap):
  return max(1, min(cap, (work + block - 1) // block))


def cut(vec, d, block, caps):
  """for_body_and_tail<4>(Tail::kOwnLaunch, vec, d, block, caps): [(VEC, first coordinate, vectors, grid)]."""
  assert d <= M.K_MAX_COLS_PER_LAUNCH
  vec = min(vec, 4)
  if d // vec == 0:
    vec = 1
  out, body = [], 0
  if d > 0 and vec > 1:
    nvec = d // vec
    body = nvec * vec
    out.append((vec, 0, nvec, stream_grid(nvec, block, caps[0])))
  if body < d:
    out.append((1, body, d - body, stream_grid(d - body, block, caps[1]) if body == 0 else 1))
  return out


def given_roles(case):
  """The pointers the caller passes (the argument cases pass some the entry point then drops)."""
  att = case.f > 0
  out = ["s", "h", "def"]
  if att or case.arg == "byz_f0":
    out.append("byz")
  if case.cm >= 2:
    out.append("past")
  if case.cm == 3 and case.arg != "alias_past":
    out.append("oldest")
  if case.l2:
    out += ["params", "origin"]
  if case.cm >= 1 or case.arg == "curv_mode0":
    out.append("curv")
  if case.a_out:
    out.append("a_out")
  if case.mom:
    out.append("mom")
  if case.arg == "alias_sh":
    out.remove("h")
  return [r for r in ROLES if r in out]


def live_roles(case):
  """The pointers left after the entry point nulled what the call does not use: byz and a_out without an attack, past
  below mode 2, oldest below mode 3, curv in mode 0, params / origin unless both are given."""
  att = case.f > 0
  keep = {"s": True, "h": True, "def": True, "byz": att, "past": case.cm >= 2, "oldest": case.cm == 3,
          "params": case.l2, "origin": case.l2, "curv": case.cm >= 1, "a_out": att and case.a_out, "mom": case.mom}
  return [r for r in ROLES if keep[r]]


def role_offsets(case):
  """Byte offset (modulo 16) of every pointer of a study call."""
  out = {r: case.offset for r in ROLES}
  if case.mis is not None:
    out[case.mis[0]] = (case.offset + case.mis[1]) % 16
  if case.arg == "alias_past":
    out["oldest"] = out["past"]
  if case.arg == "alias_sh":
    out["h"] = out["s"]
  return out


def study_vec(case):
  offs = role_offsets(case)
  return M.vec_width([offs[r] for r in live_roles(case)])


def burst_shape(cm, l2, mom):
  """(U, staged iterations per burst) of study_stats_burst_kernel<ATT, CM, L2, MOM>."""
  return (1 if (l2 and cm >= 2) or mom else 2), (K_STUDY_SLOT_BUDGET // 2 if mom else K_STUDY_SLOT_BUDGET)


def burst_grid(cus):
  return min(cus, K_STUDY_MAX_BLOCKS)


def burst_iterations(nvec, cus):
  span = burst_grid(cus) * K_STUDY_BURST_THREADS
  return (nvec + span - 1) // span


def plain_iterations(nvec, grid, block=K_STUDY_BLOCK):
  """Iterations of the grid-stride loop of the busiest lane (lane 0 of workgroup 0)."""
  return (nvec + grid * block - 1) // (grid * block)


def study_burst_eligible(case, vec, nvec, cus):
  threshold = dict(DEFAULT_KNOBS, **dict(case.knobs))["BM_STUDY_BURST"]
  if threshold <= 0 or case.cm < 1 or vec != 4 or "a_out" in live_roles(case) or nvec >= (1 << 30):
    return False
  return nvec >= threshold * cus * K_STUDY_BURST_THREADS


def stack_vec(case):
  return M.vec_width(M.row_offsets(case.offset, case.f))  # (the two outputs are fresh allocations)


def dispatch_stack_stats(k, vec, nvec):
  """(KMAX, VEC, vectors) of the instance dispatch_stack_stats<vec> launches."""
  for tier in STACK_TIERS:
    if k <= tier:
      return tier, vec, nvec
  if k <= 32:
    return 32, min(vec, 2), nvec * (vec // 2 if vec > 2 else 1)
  return 64, 1, nvec * vec


def study_launches(case, cus):
  out, part = [], 0
  att, vec = case.f > 0, study_vec(case)
  for v, first, count, grid in cut(vec, case.d, K_STUDY_BLOCK, STUDY_CAPS):
    if study_burst_eligible(case, v, count, cus):
      grid = burst_grid(cus)
      out.append(Launch("burst", ("study_burst", att, case.cm, case.l2, case.mom), v, first, count, grid, part))
    else:
      out.append(Launch("plain", ("study", att, case.cm, case.l2, v), v, first, count, grid, part))
    part += grid
  return out, part


def stack_launches(k, vec, d):
  out, part = [], 0
  for v, first, count, grid in cut(vec, d, K_RED_BLOCK, STATS_CAPS):
    kmax, v2, n2 = dispatch_stack_stats(k, v, count)
    out.append(Launch("plain", ("stack", kmax, v2), v2, first, n2, grid, part))
    part += grid
  return out, part


def instances(case, cus=256):
  """(the set of instances the call of `case` launches, its launches, nparts of its finish kernel) under the case's
  knobs on a device with `cus` compute units.  "aliased": the study call's, then the stack call's."""
  if case.kernel == "stack":
    launches, nparts = stack_launches(case.f, stack_vec(case), case.d)
  else:
    launches, nparts = study_launches(case, cus)
    if case.kernel == "aliased":
      launches = launches + stack_launches(case.f, M.vec_width([case.offset]), case.d)[0]
  return {l.inst for l in launches}, launches, nparts


def source_instances():
  """Every instance the sources can instantiate: 48 + 24 + 12 = 84."""
  out = set()
  for att in (False, True):
    for l2 in (False, True):
      for cm in range(4):
        for vec in (4, 2, 1):
          out.add(("study", att, cm, l2, vec))
        if cm >= 1:
          for mom in (False, True):
            out.add(("study_burst", att, cm, l2, mom))
  for vec in (4, 2, 1):
    for tier in STACK_TIERS:
      out.add(("stack", tier, vec))
  out |= {("stack", 32, 2), ("stack", 32, 1), ("stack", 64, 1)}
  return out


def edges(case, cus=256):
  """The edge coordinates E of a case, in order: 0, the last coordinate of the wide body, every coordinate of a tail
  launch (or the last coordinate), the first and the last coordinate of the last live iteration of workgroup 0 and of
  the last workgroup of the first launch, and either side of every burst boundary."""
  _, launches, _ = instances(case, cus)
  launches = [l for l in launches if l.inst[0] != "stack"] or launches
  d = case.d
  if d == 0:
    return []
  out = [0, d - 1]
  body = launches[0]
  if len(launches) > 1:
    out += [launches[1].first - 1] + list(range(launches[1].first, d))
  block = K_STUDY_BURST_THREADS if body.form == "burst" else K_STUDY_BLOCK
  stride = body.grid * block
  for wg in (0, body.grid - 1):
    if wg * block < body.count:
      it = (body.count - 1 - wg * block) // stride
      lo = it * stride + wg * block
      hi = min(lo + block, body.count) - 1
      out += [lo * body.vec, hi * body.vec + body.vec - 1]
  if body.form == "burst":
    slots = burst_shape(case.cm, case.l2, case.mom)[1]
    for p0 in range(slots, burst_iterations(body.count, cus), slots):
      out += [p0 * stride * 4 - 1, p0 * stride * 4]
  return sorted(set(c for c in out if 0 <= c < d))


# ---------------------------------------------------------------------------------------------------------------------
# The case lists (every GPU test of tests/test_gpu_study_matrix.py runs exactly the cases of its group and part)

D_SHORT = 4 * (256 + 37) + 3        # two workgroups, the second ragged, and a 3-coordinate tail
D_EDGE = (0, 1, 3, 4, 5, 1023, 1024, 1027)
D_STACK = (0, 3, 1027, 4 * 256 * 3 + 2)
F_REALS = (1, 2, 3, 5, 64)
STACK_KS = ((1, 8), (9, 16), (17, 24), (25, 32), (33, 64))  # both edges of every tier
STACK_OFFSETS = (0, 4, 8, "mixed")
ATTACKS = (("empire", 1.1, False), ("little", -1.5, False), ("empire", 1.1, True), ("little", -1.5, True))
BURST_ONLY = (("BM_STUDY_BURST", 1),)
BAD_VALUES = ("nan", "inf", "-inf", "max")
BAD_PLACES = ("first", "lane63", "lane255", "last", "tail")
BURST_CLASSES = ((2, 8), (1, 8), (1, 4))
# the cheapest instance of each (U, slots) class: (f_real, cm, l2, mom)
CLASS_INSTANCE = {(2, 8): (0, 1, False, False), (1, 8): (0, 2, True, False), (1, 4): (0, 1, False, True)}
FULL = dict(f=3, cm=3, l2=True, mom=True, a_out=True)  # every pointer live
ARGS = ("a_out_f0", "byz_f0", "curv_mode0", "curv_nan_mode1", "alias_past", "alias_sh", "spare_slots", "d0")
LONG = 1 << 16  # cases from this length on carry spikes at their edge coordinates
MU, W_OLDEST = 0.9, -(0.9 ** 4)
MOM_MU, MOM_OMD = 0.99, 0.01


def _case(group, kernel="study", **kw):
  base = dict(f=0, cm=0, l2=False, mom=False, a_out=False, offset=0, mis=None, d=D_SHORT, spiked=False, bad=None,
              arg=None, attack="empire", scale=None, direction=False, avg=True, scaled=False, knobs=(), idx=0)
  base.update(kw)
  if base["d"] >= LONG:
    base["spiked"] = True
  return Case(group, kernel, **base)


def span_of(cus):
  return burst_grid(cus) * K_STUDY_BURST_THREADS


def burst_length(iterations, cus, tail):
  """16-byte columns: `iterations` - 1 full iterations of the burst form, a partly live last one (3 full workgroups'
  worth of lanes and 70 more), and `tail` trailing coordinates."""
  return 4 * ((iterations - 1) * span_of(cus) + 3 * K_STUDY_BURST_THREADS + 70) + tail


def fold_length():
  """The smallest d at which a lane of the plain form has K_STUDY_FOLD + 1 iterations (4-byte columns)."""
  return K_STUDY_FOLD * K_STUDY_MAX_BLOCKS * K_STUDY_BLOCK + 1


def nparts_length(nparts, tail):
  """16-byte columns: `nparts` - (1 if tail else 0) workgroups of the body, all full, and `tail` coordinates; beyond
  the grid cap the body is one workgroup of work longer than the grid."""
  groups = nparts - (1 if tail else 0)
  if groups > K_STUDY_MAX_BLOCKS:
    raise ValueError(nparts)
  return 4 * groups * K_STUDY_BLOCK + tail


def cases(group, cus=256, part=None):
  """The cases of a group, or of one part of it (a case keeps its index whichever way it is asked for)."""
  out = []

  def add(p, **kw):
    kw.setdefault("idx", len(out))
    out.append((p, _case(group, **kw)))

  if group == "plain":
    for p, off in enumerate((0, 8, 4)):  # VEC 4, 2, 1
      for cm in range(4):
        for l2 in (False, True):
          for mom in (False, True):
            add(p, cm=cm, l2=l2, mom=mom, offset=off)
            for a_out in (False, True):
              add(p, f=F_REALS[len(out) % len(F_REALS)], cm=cm, l2=l2, mom=mom, a_out=a_out, offset=off)
    for off in (0, 8, 4):
      for d in D_EDGE:
        add(3, d=d, offset=off if d else 0, **FULL)
    add(3, offset=12, **FULL)
    for role in ROLES:
      for by in (4, 8):
        add(3, mis=(role, by), **FULL)
    for f in F_REALS:
      add(3, **dict(FULL, f=f))
  elif group == "plain_long":
    add(0, f=3, cm=2, mom=True, offset=4, d=fold_length())
    add(1, d=4 * (K_STUDY_MAX_BLOCKS + 1) * K_STUDY_BLOCK + 3, **FULL)  # the grid cap and one workgroup of work more
    add(2, l2=True, mom=True, d=nparts_length(K_STUDY_MAX_BLOCKS, 0))  # (mode 0: the plain form at any CU count)
    add(2, d=nparts_length(64, 0), **FULL)
    add(2, d=nparts_length(65, 3), **FULL)
  elif group == "knob_burst":
    for p, att in enumerate((False, True)):  # all 24 instances at two iterations, the last partly live, and a tail of 3
      for cm in (1, 2, 3):
        for l2 in (False, True):
          for mom in (False, True):
            add(p, f=(1, 3, 5)[len(out) % 3] if att else 0, cm=cm, l2=l2, mom=mom, d=burst_length(2, cus, 3),
                knobs=BURST_ONLY)
    for cls in BURST_CLASSES:
      f, cm, l2, mom = CLASS_INSTANCE[cls]
      add(2, f=f, cm=cm, l2=l2, mom=mom, d=4 * span_of(cus), knobs=BURST_ONLY)      # one iteration, every lane live
      add(2, f=f, cm=cm, l2=l2, mom=mom, d=burst_length(3, cus, 2), knobs=BURST_ONLY)
    for p, cls in enumerate(BURST_CLASSES):  # one iteration past a burst
      f, cm, l2, mom = CLASS_INSTANCE[cls]
      add(3 + p, f=f, cm=cm, l2=l2, mom=mom, d=burst_length(cls[1] + 1, cus, 1), knobs=BURST_ONLY)
    add(6, d=burst_length(2, cus, 3), knobs=BURST_ONLY, **FULL)  # an attack-average output: the plain form
    for value, role, place in (("nan", "def", "lane1023"), ("max", "byz", "lane1023"), ("inf", "byz", "last"),
                               ("max", "def", "last")):
      add(6, d=burst_length(2, cus, 0), knobs=BURST_ONLY, bad=(value, role, place), **dict(FULL, a_out=False))
  elif group == "args":
    for arg in ARGS:
      kw = dict(FULL)
      if arg in ("a_out_f0", "byz_f0"):
        kw["f"] = 0
      if arg == "byz_f0":
        kw["a_out"] = False
      if arg == "curv_mode0":
        kw["cm"] = 0
      if arg == "curv_nan_mode1":
        kw["cm"] = 1
      if arg == "spare_slots":
        kw = dict(f=0, cm=0, l2=False, mom=False, a_out=False)
      add(None, arg=arg, d=0 if arg == "d0" else D_SHORT, **kw)
  elif group == "bad":
    for value in BAD_VALUES:
      for role in ("def", "byz"):
        for place in BAD_PLACES:
          add(None, offset=(0, 8, 4)[len(out) % 3], bad=(value, role, place), **dict(FULL, f=(3, 1, 5)[len(out) % 3]))
  elif group == "stack":
    for p, ks in enumerate(STACK_KS):
      for k in ks:
        attacks = ATTACKS if k > 1 else (ATTACKS[0], ATTACKS[2])  # the unbiased variance of one row is not defined
        for attack, scale, direction in attacks:  # every output combination of every attack at one length
          for avg in (False, True):
            add(p, kernel="stack", f=k, d=1027, attack=attack, scale=scale, direction=direction, avg=avg, scaled=True)
        for avg in (False, True):
          add(p, kernel="stack", f=k, d=1027, avg=avg)
        for off in STACK_OFFSETS:
          for d in D_STACK:
            n = len(out)
            attack, scale, direction = attacks[n % len(attacks)]
            add(p, kernel="stack", f=k, d=d, offset=off if d else 0, attack=attack, scale=scale, direction=direction,
                avg=n % 3 != 0, scaled=n % 5 != 0)
    last = len(STACK_KS)
    add(last, kernel="stack", f=3, d=4 * ((K_MAX_PARTIAL_BLOCKS - 1) * K_RED_BLOCK + 1) + 3, attack="little", scale=-1.5,
        scaled=True)  # the 2047-workgroup cap, one vector more, and a tail
    for i, value in enumerate(BAD_VALUES[:3]):
      for k in (5, 26, 40):
        add(last, kernel="stack", f=k, d=1027, attack="empire", scale=1.1, scaled=True,
            bad=(value, i, ("first", "last", "tail")[i]))
  elif group == "aliased":
    for f in (1, 3, 5, 64):
      for d in (D_SHORT, 4 * 256 * 3 + 2):
        add(None, kernel="aliased", f=f, a_out=True, d=d)
  else:
    raise ValueError(group)
  return [c for p, c in out if part is None or p == part]


GROUPS = ("plain", "plain_long", "knob_burst", "args", "bad", "stack", "aliased")
PARTS = {"plain": (0, 1, 2, 3), "plain_long": (0, 1, 2), "knob_burst": tuple(range(7)),
         "stack": tuple(range(len(STACK_KS) + 1))}


def all_cases(cus=256):
  return [c for g in GROUPS for c in cases(g, cus)]


def case_key(case):
  """The case without its group and knobs: a knob's child and the parent at the defaults name a case alike."""
  return "/".join(str(x) for x in case[1:-2]) + "/" + str(case.idx)


# ---------------------------------------------------------------------------------------------------------------------
# Seeded inputs (on the CPU)

F32 = torch.float32
SHORT_FULL = 4096
SPIKE_LOG2 = 8   # the smallest spike: 2^8; |E| <= 9, so the largest is at most 2^16 (see DESIGN.md for the room)
MAX_EDGES = 9
SEED_SALT = {}   # (role, length of the draw) -> salt, where a draw holds more fma midpoints than MIDPOINT_CAP allows
_DRAWS = {}


def _draw(role, full):
  if any(k[1] != full for k in _DRAWS):
    _DRAWS.clear()
  if (role, full) not in _DRAWS:
    seed = 7919 * (ROLES.index(role) + 1) + full % 10007 + 100003 * SEED_SALT.get((role, full), 0)
    _DRAWS[(role, full)] = torch.randn(full, generator=torch.Generator().manual_seed(seed))
  return _DRAWS[(role, full)]


def seq_avg_copies(byz, f):
  """The sequential fp32 mean of f copies of one vector (tools/pytorch.py:108-111)."""
  return F.seq_avg(byz[None].expand(f, -1))


def _tune_deviation(byz, cols, f, base=8.0):
  """At the columns `cols`, move byz into [base, 2 base), to the one of 64 evenly spaced values (and the 15 floats above each) where its deviation
  from the mean of its f copies is largest: that deviation is a rounding residue, zero in whole stretches of a binade
  (which ones depends on f) and larger at larger values."""
  for c in cols:
    x = float(byz[c])
    cand = torch.tensor([base + (j + abs(x) % 1.0) * base / 64 for j in range(64)], dtype=F32)
    cand = (cand.view(torch.int32)[:, None] + torch.arange(16, dtype=torch.int32)).view(F32).flatten()  # and 15 ulps on
    dev = (cand.double() - seq_avg_copies(cand, f).double()).abs()
    byz[c] = math.copysign(float(cand[int(dev.argmax())]), x)


def bad_column(case, place, cus=256):
  """The coordinate a `bad` place names, by the launch plan: the last component of lane 63 / 255 / 1023's vector of
  the last live iteration of workgroup 0, the first component of the last vector of the body, the last coordinate."""
  launches = instances(case, cus)[1]
  body = launches[0]
  if place == "first":
    return 0
  if place == "tail":
    return case.d - 1
  if place == "last":
    return (body.count - 1) * body.vec
  lane = int(place[4:])
  block = K_STUDY_BURST_THREADS if body.form == "burst" else K_STUDY_BLOCK
  it = (body.count - 1 - lane) // (body.grid * block)
  return (it * body.grid * block + lane) * body.vec + body.vec - 1


BAD = dict(F.BAD)
MAX_SHORT = 40.0  # "max": above every seeded normal; a long case takes the power of two above its largest spike


def values(case, cus=256):
  """{role: float32 vector} of the inputs of a study case (every role of INPUTS the caller passes)."""
  d = case.d
  full = SHORT_FULL if d <= SHORT_FULL else d
  roles = [r for r in given_roles(case) if r != "a_out"]
  v = {r: _draw(r, full)[:d].clone() for r in roles}
  e = edges(case, cus)
  assert len(e) <= MAX_EDGES, (case, e)
  if e:
    at = torch.tensor(e)
    if case.spiked:
      for i, c in enumerate(e):
        size = 2.0 ** (SPIKE_LOG2 + (i + case.idx) % len(e))  # the largest rotates with the case
        for r in roles:
          if r != "origin":
            v[r][c] = -size if (i % 2 == 1 and r in ("def", "byz")) else size
    else:
      for r in roles:
        v[r][at] += torch.copysign(torch.tensor(0.5), v[r][at])
      if "origin" in v:
        v["origin"][at] = -0.5 * v["params"][at]
      if case.f >= 3:
        # (one copy and two add up exactly)
        _tune_deviation(v["byz"], e, case.f)
  if case.arg == "curv_nan_mode1":
    v["curv"].fill_(math.nan)
  if case.arg == "byz_f0":
    v["byz"].fill_(math.nan)
  if case.bad is not None:
    value, role, place = case.bad
    col = bad_column(case, place, cus)
    if value == "max":
      v[role][col] = (2.0 ** (SPIKE_LOG2 + len(e)) if case.spiked else MAX_SHORT) * (-1.0 if role == "def" else 1.0)
      if role == "byz" and case.f >= 3 and not case.spiked:
        _tune_deviation(v[role], [col], case.f, MAX_SHORT)
    else:
      v[role][col] = BAD[value]
  if case.arg == "alias_past":
    v["oldest"] = v["past"]
  if case.arg == "alias_sh":
    v["h"] = v["s"]
  return v


def stack_values(case, cus=256):
  """The k x d rows of a stack case: first_pass_matrix's draw.  At the edge coordinates of a short case the rows share
  a sign, stay away from zero and row 0 stands sqrt(k) apart (an average and a deviation that count); in a long case
  row 0 carries 2^10 there and 2^11 at one of them (the bar of these sums, 2e-5, has no room for nine distinct powers
  of two)."""
  rows = F.clean_values(case.f, 1, "iid", case.d)[0].clone()
  e = edges(case, cus)
  assert len(e) <= MAX_EDGES
  if case.spiked:
    for i, c in enumerate(e):
      rows[0, c] = (2.0 ** 11 if i == case.idx % len(e) else 2.0 ** 10) * (-1.0 if i % 2 else 1.0)
  elif e:
    at = torch.tensor(e)
    sign = torch.copysign(torch.tensor(1.0), rows[0, at])
    rows[:, at] = sign * (rows[:, at].abs() + 0.5)
    rows[0, at] += sign * math.sqrt(case.f)
  if case.bad is not None:
    value, row, place = case.bad
    rows[row, {"first": 0, "last": case.d // 4 * 4 - 1, "tail": case.d - 1}[place]] = BAD[value]
  return rows


# ---------------------------------------------------------------------------------------------------------------------
# The expected results, from the inputs alone

TOL_DOT = 1e-6          # of |a||b|: test_study_stats_against_fp64
TOL_DEV = 1e-5          # slot 19, relative: the same test
TOL_SUMS = F.TOL_SUMS   # the stack sums, on the forms test_momentum_stats_kernel_tiers compares
TOL_LITTLE = F.TOL_LITTLE
MIDPOINT_CAP = F.MIDPOINT_CAP
GRAM = [(r, c) for r in range(4) for c in range(r, 4)]


def study_terms(case, v):
  """Yields (slot, per-coordinate float64 terms, absolute bar) of every sum slot of a study call that is not zero by
  construction; the slot's expected value is terms.sum().  Slot 4 r + c stands for the Gram entry (r, c), r <= c."""
  att = case.f > 0
  core = [v["s"].double(), v["h"].double(), v["def"].double()]
  a32 = seq_avg_copies(v["byz"], case.f) if att else None
  if att:
    core.append(a32.double())
  norm = [math.sqrt(float((c * c).sum())) for c in core]
  for r, c in GRAM:
    if c < len(core):
      yield 4 * r + c, core[r] * core[c], TOL_DOT * norm[r] * norm[c]
  if case.cm >= 2:
    for slot, other in ((16, v["past"]), (17, v["curv"])):
      o = other.double()
      yield slot, core[0] * o, TOL_DOT * norm[0] * math.sqrt(float((o * o).sum()))
  if att:
    yield 18, core[3] * core[3], TOL_DOT * norm[3] * norm[3]
    dev = (v["byz"].double() - core[3]) ** 2 * case.f  # f identical terms (tools/pytorch.py:117-121)
    yield 19, dev, TOL_DEV * float(dev.sum()) + 1e-30
  if case.l2:
    e = (v["params"].double() - v["origin"].double()) ** 2
    yield 22, e, TOL_DOT * float(e.sum())


def stack_terms(case, rows):
  """The same for bm_stack_stats: (0, avg^2) and (1, sum_i (x_i - avg)^2), centred at the expected fp32 average; the
  bars are the relative 1e-5 on the square roots the suite compares, 2e-5 on the sums."""
  a = F.seq_avg(rows).double()
  yield 0, a * a, 2 * TOL_SUMS * float((a * a).sum())
  dev = ((rows.double() - a) ** 2).sum(dim=0)
  yield 1, dev, 2 * TOL_SUMS * float(dev.sum())


def insensitive(case, cus=256):
  """[(slot, coordinate)]: the edge coordinates whose loss or doubling would move a non-zero sum slot of the case by
  less than ten of the slot's bars."""
  if case.d == 0:
    return []
  e = edges(case, cus)
  terms = stack_terms(case, stack_values(case, cus)) if case.kernel == "stack" else study_terms(case, values(case, cus))
  out = []
  for slot, t, bar in terms:
    if not math.isfinite(bar) or float(t.abs().sum()) == 0.0:
      continue
    out += [(slot, c) for c in e if not abs(float(t[c])) >= 10 * bar]
  return out


def next_up_down(t):
  bits = t.view(torch.int32)
  up = torch.where(t >= 0, bits + 1, bits - 1).view(F32)
  down = torch.where(t > 0, bits - 1, torch.where(t < 0, bits + 1, torch.full_like(bits, -0x7FFFFFFF))).view(F32)
  return up, down


StudyExpected = namedtuple("StudyExpected", "out bars a curv curv_alt curv_mid mom mom_mid")


def study_expected(case, v):
  """The 32 slots (float64; `bars`: {slot: absolute bar} of the sums, every other slot is exact), the attack average,
  C with the alternatives of its midpoint columns, and M with its midpoint mask."""
  out, bars = [0.0] * STUDY_SLOTS, {}
  for slot, t, bar in study_terms(case, v):
    out[slot], bars[slot] = float(t.sum()), bar
  for r, c in GRAM:
    out[4 * c + r] = out[4 * r + c]
  a = seq_avg_copies(v["byz"], case.f) if case.f > 0 else None
  if a is not None:
    out[20] = F.abs_max(a)
  out[21] = F.abs_max(v["def"])
  s = v["s"]
  mu32 = torch.tensor(MU, dtype=F32)
  curv = alt = mid = None
  if case.cm == 1:
    curv = s.clone()
  elif case.cm == 2:
    curv = s + v["curv"] * mu32
  elif case.cm == 3:
    t, mid = F.fma_emulated(W_OLDEST, v["oldest"], 1.0, v["curv"])
    curv = s + t * mu32
    alt = [s + x * mu32 for x in next_up_down(t)]
  mom = mom_mid = None
  if case.mom:
    mom, mom_mid = F.fma_emulated(MOM_OMD, v["def"], MOM_MU, v["mom"])
  return StudyExpected(out, bars, a, curv, alt, mid, mom, mom_mid)


def midpoints(case, cus=256):
  """(midpoint elements of the two emulated fmas of a study case, elements)."""
  e = study_expected(case, values(case, cus))
  n = el = 0
  for mid in (e.curv_mid, e.mom_mid):
    if mid is not None:
      n, el = n + int(mid.sum()), el + mid.numel()
  return n, el


# ---------------------------------------------------------------------------------------------------------------------
# Running one case on the GPU

DEV = "cuda:0"
GAP = 8  # floats between two vectors of the flat allocation, and in front of the first


def place_at(distinct, byte_offsets, fill=math.nan):
  """instance_matrix.place with one byte offset per row: the rows of `distinct` (a list of equally long vectors) in ONE
  flat allocation, row i at byte offset byte_offsets[i] modulo 16, NaN-filled gaps of at least GAP - 3 floats in front
  of, between and behind them.  Returns the views."""
  d = distinct[0].numel()
  stride = (d + 3) // 4 * 4 + GAP
  flat = torch.full((len(distinct) * stride + GAP,), fill, dtype=F32, device=DEV)
  assert flat.data_ptr() % 256 == 0
  views = []
  for i, (row, off) in enumerate(zip(distinct, byte_offsets)):
    lo = i * stride + 4 + off // 4
    views.append(flat[lo:lo + d])
    views[-1].copy_(row)
    assert views[-1].data_ptr() % 16 == off
  return views


def _bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


def _changed_outside(flat, before, writable):
  """Whether anything but the `writable` views changed in the allocation the vectors were cut from."""
  for w in writable:
    lo = w.storage_offset() - flat.storage_offset()
    before[lo:lo + w.numel()] = 0
    w.zero_()
  return not torch.equal(flat.view(torch.int32), before.view(torch.int32))


A_OUT_FILL = 7.0


def run_study(case, cus):
  """One call of bm_study_stats_update through the C ABI, `out` pre-filled with NaN.  Returns `out` (a list), `curv`,
  `mom`, `a_out` (CPU, None where not passed) and `stray`: whether anything the call may not write changed."""
  import ctypes
  from byzantinemomentum_amd import _lib, gars
  lib = _bm()._lib.load()
  v = values(case, cus)
  given = given_roles(case)
  offs = role_offsets(case)
  d = case.d
  views = dict(zip(given, place_at([v[r] if r != "a_out" else torch.full((d,), A_OUT_FILL) for r in given],
                                   [offs[r] for r in given])))
  flat = views["s"]._base
  before = flat.clone()
  ptr = dict(views)
  if case.arg == "alias_past":
    ptr["oldest"] = views["past"]
  if case.arg == "alias_sh":
    ptr["h"] = views["s"]
  out = torch.full((STUDY_SLOTS,), math.nan, dtype=torch.float64, device=DEV)
  ws = gars._workspace(flat.device, _lib.WS_STUDY, 1, d, "ws_study")

  def p(role):
    return ctypes.c_void_p(ptr[role].data_ptr()) if role in ptr else ctypes.c_void_p(0)

  with torch.cuda.device(flat.device):
    _lib.check(lib.bm_study_stats_update(
      p("s"), p("h"), p("def"), p("byz"), int(case.f), p("a_out"), p("past"), p("curv"), p("oldest"), int(case.cm),
      ctypes.c_float(MU), ctypes.c_float(W_OLDEST), p("params"), p("origin"), p("mom"), ctypes.c_float(MOM_MU),
      ctypes.c_float(MOM_OMD), d, gars._ptr(out), gars._ptr(ws), gars._stream(flat.device)), "bm_study_stats_update")
  torch.cuda.synchronize()
  gars.invalidate_rank_cache()
  live = live_roles(case)
  got = {"out": out.tolist()}
  writable = []
  for role in ("curv", "mom", "a_out"):
    got[role] = views[role].cpu() if role in views else None
    if role in views and role in live:
      writable.append(views[role])
  got["stray"] = _changed_outside(flat, before, writable)
  return got


def run_stack(case, cus, rows=None):
  """One call of bm_stack_stats.  Returns `avg`, `scaled` (CPU or None), `out3` (a list) and `stray`."""
  bm = _bm()
  rows = stack_values(case, cus) if rows is None else rows
  views = place_at(list(rows), M.row_offsets(case.offset, case.f))
  flat = views[0]._base
  before = flat.clone()
  res = bm.stats.stack_stats_async(views, scale=case.scale if case.scaled else None, attack=case.attack,
                                   want_avg=case.avg, direction=case.direction)
  torch.cuda.synchronize()
  got = {"avg": res[0].cpu() if res[0] is not None else None, "out3": res[1].tolist(),
         "scaled": res[2].cpu() if case.scaled else None}
  got["stray"] = _changed_outside(flat, before, [])
  return got


# ---------------------------------------------------------------------------------------------------------------------
# The bars

class Worst(F.Worst):
  """first_pass_matrix.Worst keyed by (kernel, instance, VEC)."""

  def lines(self):
    out = []
    for family, inst, vec, quantity, value, bar in self.entries():
      head = f"{family:11s} {inst:14s} VEC={vec}  {quantity:10s}"
      if quantity == "midpoints":
        out.append(f"{head} {int(value)} exempted of {int(bar)} elements (cap {MIDPOINT_CAP:g} of a case)")
      elif bar == 0:
        out.append(f"{head} {int(value)} mismatches  bit-exact")
      else:
        out.append(f"{head} worst error {value:.3e}  bar {bar:g}")
    return out


ERRORS = Worst()


def table_key(launch):
  inst = launch.inst
  if inst[0] == "stack":
    return ("stack", f"KMAX={inst[1]}", inst[2])
  name = f"ATT={int(inst[1])},CM={inst[2]},L2={int(inst[3])}"
  return (inst[0], name + (f",MOM={int(inst[4])}" if inst[0] == "study_burst" else ""), launch.vec)


def _same(got, want):
  return (math.isnan(got) and math.isnan(want)) or got == want


def _within(got, want, bar):
  """One sum against its float64 value: NaN for NaN, the same infinity, else within the absolute bar."""
  if not math.isfinite(want) or not math.isfinite(bar):
    return _same(got, want) if not math.isnan(want) else math.isnan(got)
  return abs(got - want) <= bar


def _exact(fail, worst, key, name, got, want, mid=None, alt=None):
  """Bit for bit outside `mid`; inside, one of `alt` (C) or within 1 ulp (M)."""
  differ = F.bits_differ(got, want)
  bad = differ if mid is None else differ & ~mid
  worst.add(key, name, int(bad.sum()), 0)
  if bool(bad.any()):
    c = int(torch.nonzero(bad)[0])
    fail(f"{name}: {int(bad.sum())} coordinates differ, first [{c}] {got[c].item()!r} for {want[c].item()!r}")
  if mid is not None and bool(mid.any()):
    worst.add(key, "midpoints", int(mid.sum()), mid.numel())
    if int(mid.sum()) > MIDPOINT_CAP * mid.numel():
      fail(f"{name}: {int(mid.sum())} midpoint elements of {mid.numel()}: pick another seed")
    if alt is not None:
      ok = ~differ
      for a in alt:
        ok |= ~F.bits_differ(got, a)
    else:
      ok = (got.view(torch.int32).long() - want.view(torch.int32).long()).abs() <= 1
    if not bool(ok[mid].all()):
      fail(f"{name}: a midpoint element more than 1 ulp off")


def check_study(case, got, cus, worst=ERRORS, knobs=None):
  """Hold the outputs of one study call to the bars; returns the list of failures (strings).  knobs: the BM_* values
  the process ran with where they are not the case's (the error table names the instance that ran)."""
  v = values(case, cus)
  e = study_expected(case, v)
  launches = instances(case if knobs is None else case._replace(knobs=knobs), cus)[1]
  key = table_key(launches[0]) if launches else ("study", "d=0", 0)
  fails = []

  def fail(text):
    fails.append(f"{case_key(case)}: {text}")

  if got["stray"]:
    fail("an input, a guard gap or an unused buffer changed")
  o = got["out"]
  for slot in range(STUDY_SLOTS):
    want = e.out[slot]
    r, c = min(slot // 4, slot % 4), max(slot // 4, slot % 4)
    bar = e.bars.get(4 * r + c if slot < 16 else slot)
    if bar is None:  # a maximum, or a zero
      worst.add(key, "max" if slot in (20, 21) else "zeros", 0 if _same(o[slot], want) else 1, 0)
      if not _same(o[slot], want):
        fail(f"slot {slot}: {o[slot]!r} for {want!r} (exact)")
      continue
    if math.isfinite(want) and math.isfinite(o[slot]) and bar > 0:
      name = "dev" if slot == 19 else ("l2" if slot == 22 else "dots")
      tol = TOL_DEV if slot == 19 else TOL_DOT
      worst.add(key, name, abs(o[slot] - want) / bar * tol, tol)
    if not _within(o[slot], want, bar):
      fail(f"slot {slot}: {o[slot]!r} for {want!r} (bar {bar:g})")
  live = live_roles(case)
  if "curv" in live:
    _exact(fail, worst, key, "C", got["curv"], e.curv, e.curv_mid, e.curv_alt)
  if "mom" in live:
    _exact(fail, worst, key, "M", got["mom"], e.mom, e.mom_mid)
  if "a_out" in live:
    _exact(fail, worst, key, "a_out", got["a_out"], e.a)
  return fails


def check_stack(case, got, cus, worst=ERRORS, rows=None):
  rows = stack_values(case, cus) if rows is None else rows
  k, d = case.f, case.d
  launches = instances(case, cus)[1]
  key = table_key([l for l in launches if l.inst[0] == "stack"][0]) if d else ("stack", "d=0", 0)
  fails = []

  def fail(text):
    fails.append(f"{case_key(case)}: {text}")

  if got["stray"]:
    fail("a row or a guard gap changed")
  avg = F.seq_avg(rows)
  if (got["avg"] is not None) != case.avg or (got["scaled"] is not None) != case.scaled:
    fail("outputs present do not match the request")
  if got["avg"] is not None:
    _exact(fail, worst, key, "avg", got["avg"], avg)
  if got["scaled"] is not None:
    want, exact = F.byzantine(avg, rows, case.attack, case.scale, case.direction)
    if exact:
      _exact(fail, worst, key, "empire", got["scaled"], want)
    elif d:
      fin = torch.isfinite(want)
      top = float(want[fin].abs().max()) if bool(fin.any()) else 1.0
      g64 = got["scaled"].double()
      err = (g64 - want).abs()
      ok = (torch.isnan(want) & torch.isnan(g64)) | (torch.isinf(want) & (g64 == want)) | (fin & (err <= TOL_LITTLE * top))
      both = fin & torch.isfinite(g64)
      worst.add(key, "little", float(err[both].max()) / top if bool(both.any()) else 0.0, TOL_LITTLE)
      if not bool(ok.all()):
        c = int(torch.nonzero(~ok)[0])
        fail(f"little: column {c} {got['scaled'][c].item()!r} for {want[c].item()!r} (bar {TOL_LITTLE:g} x {top:g})")
  n2, dev = F.sums64(rows, avg)
  o = got["out3"]
  forms = [("norm", math.sqrt(o[0]) if o[0] >= 0 else o[0], math.sqrt(n2) if n2 >= 0 else n2)]
  if k > 1:
    forms.append(("dev", math.sqrt(o[1] / (k - 1)) if o[1] >= 0 else o[1], math.sqrt(dev / (k - 1)) if dev >= 0 else dev))
  else:
    forms.append(("dev", o[1], dev))
  for name, value, want in forms:
    worst.add(key, name, F.rel_error(value, want), TOL_SUMS)
    if not F.close(value, want, TOL_SUMS):
      fail(f"{name}: {value!r} for {want!r}")
  top = F.abs_max(avg)
  worst.add(key, "max", 0 if _same(o[2], top) else 1, 0)
  if not _same(o[2], top):
    fail(f"max: {o[2]!r} for {top!r}")
  return fails


def run_aliased(case, cus, worst=ERRORS):  # (no knob reaches these cases: an attack-average output keeps the plain form)
  """The source's sentence "stack_stats_kernel on f aliased rows": the study block against bm_stack_stats on
  [byz] * f_real.  a_out and slot 20 bit for bit, slots 18 and 19 at the bars.  Both calls are held to the expected
  values as well."""
  study = run_study(case, cus)
  fails = check_study(case, study, cus, worst)
  byz = values(case, cus)["byz"]
  rows = byz[None].expand(case.f, -1)
  view = place_at([byz], [case.offset])[0]
  stack_case = case._replace(kernel="stack", avg=True, scaled=False)
  bm = _bm()
  avg, out3 = bm.stats.stack_stats_async([view] * case.f)
  torch.cuda.synchronize()
  stack = {"avg": avg.cpu(), "scaled": None, "out3": out3.tolist(), "stray": False}
  fails += check_stack(stack_case, stack, cus, worst, rows=rows)
  key = ("aliased", f"f={case.f}", study_vec(case))
  differ = int(F.bits_differ(study["a_out"], stack["avg"]).sum())
  worst.add(key, "a_out", differ, 0)
  o, o3 = study["out"], stack["out3"]
  if differ:
    fails.append(f"{case_key(case)}: a_out and the stack average differ in {differ} coordinates")
  if not _same(o[20], o3[2]):
    fails.append(f"{case_key(case)}: slot 20 {o[20]!r}, out3[2] {o3[2]!r}")
  for slot, other, tol in ((18, o3[0], TOL_DOT), (19, o3[1], TOL_DEV)):
    worst.add(key, f"slot{slot}", F.rel_error(o[slot], other), tol)
    if not abs(o[slot] - other) <= tol * abs(other):
      fails.append(f"{case_key(case)}: slot {slot} {o[slot]!r}, bm_stack_stats {other!r}")
  return fails, study, stack


# ---------------------------------------------------------------------------------------------------------------------
# Digests: what must keep its bits from the plain form to the burst form

def digest(case, got):
  out = {name: F._sha(got[name]) for name in ("curv", "mom", "a_out", "avg", "scaled") if got.get(name) is not None}
  o = got["out"] if "out" in got else got["out3"]
  out["max"] = F._sha(torch.tensor(o[20:22] if "out" in got else o[2:3], dtype=torch.float64))
  return out


def differing(todo, mine, theirs):
  out = []
  for c in todo:
    k = case_key(c)
    if set(mine[k]) != set(theirs[k]):
      out.append(f"{k}: outputs {sorted(mine[k])} against {sorted(theirs[k])}")
      continue
    out += [f"{k}: {name}" for name in mine[k] if mine[k][name] != theirs[k][name]]
  return out


def sweep(todo, cus, worst=ERRORS, digests=None, knobs=None):
  """Run and check the cases of `todo`; returns the failures and fills `digests` {case key: {output: SHA-256}}.
  knobs: the BM_* values of this process where they are not the cases' own (a knob group's cases at the defaults: the
  inputs, their edge coordinates included, stay those of the case as listed)."""
  fails = []
  for case in todo:
    if case.kernel == "stack":
      got = run_stack(case, cus)
      fails += check_stack(case, got, cus, worst)
    elif case.kernel == "aliased":
      more, got, _ = run_aliased(case, cus, worst)
      fails += more
    else:
      got = run_study(case, cus)
      fails += check_study(case, got, cus, worst, knobs)
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
