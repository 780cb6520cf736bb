"""The fixed-factor space of AggregationStep.run() — every rule x attack x momentum placement, the secondary arguments
laid over that product — and ONE float64 statement of the whole step to hold it against.  TEST INFRASTRUCTURE (a helper
module, not a conftest), shared by tests/test_step_matrix_cpu.py (tests/sharded_backend.OracleBackend, no GPU),
tests/test_gpu_step_matrix.py (the HIP backend) and scripts/step_matrix_probe.py.

Universe: a FIXED factor or a factorless attack.  Searched factors (`attack_evals`) stay with tests/search_matrix.py.
  rule        the 14 of step._RULES; gar_args of geomed / cclip as tests/test_gpu_center_step.GAR_ARGS, caf / dnc at
              power_iters = spectral_cases.T_END_TO_END
  attack      ATTACKS below: empire, little, anticge, nan, hidden at target_idx -1 / an interior index / "all",
              empire-strict at a positive int epsilon, minmax with each of the three perturbations, minsum
  placement   worker, server, update
  secondary   gradient_clip None / a value that clips some but not all rows; (f_decl, f_real) in (2, 2), (2, 1), (2, 0)
              at n = 11 and (5, 5) at n = 25; a negative factor for empire, little, hidden; Krum / Bulyan with `m`;
              params and origin given or not; single_call True / False
`cases()` is the full product at n = 11, f = 2, nb_past = 3, d = 1027 with the secondary values assigned so that every
(secondary value, rule), (secondary value, attack) and (secondary value, placement) pair occurs, plus PLAN cases: for
the six rules of the single call and the two attacks the first pass forms, worker placement at f_real = 2 / 0 with
single_call on / off — every plan the constructor can make in this universe is then reached.  A case is three steps; step
2 samples one gradient more than h.  `long_cases()`: the first pass riding along at lengths where the dispatch mirror
(tests/first_pass_matrix.is_fused) says it launches and where it falls back; they take no part in the CPU run.

`MatrixLoop` is the expectation: tests/attack_vectors_reference.Loop (clipping with the fp32 factor, the momentum
placements and the sequential fp32 honest mean as that restatement has them) with the Byzantine vector, the rule, both
momenta, cclip's carried start, the study row, the acceptation ratio and gamma formed here in float64 from the pieces
the project already pins one by one (oracle.gar_oracle at precision "f64", anticge_reference.anticge_f64,
minmax_reference.attack, center_cases.vector_iteration, spectral_cases.vector_spectral).  It imports nothing from
byzantinemomentum_amd.  Every discrete decision it takes is reported with its margin (`Expected.margins`); a case may
not rest on one closer than MARGINS says.
"""

import collections
import itertools
import math

import numpy as np
import torch

from oracle import gar_oracle as O
from tests import anticge_reference as A
from tests import center_cases as cc
from tests import minmax_reference as MR
from tests import spectral_cases as sc
from tests.attack_vectors_reference import Loop, assert_floats_close_nan, direction_of

RULES = ("krum", "bulyan", "median", "trmean", "phocas", "meamed", "aksel", "brute", "average", "cge", "geomed", "cclip",
         "caf", "dnc")
CENTER, SPECTRAL = ("geomed", "cclip"), ("caf", "dnc")
COLWISE, DISTANCE = ("median", "trmean", "phocas", "meamed"), ("krum", "bulyan")
PLACEMENTS = ("worker", "server", "update")
# (as tests/test_gpu_center_step.GAR_ARGS: nu = 1e-6 sqrt(4099); tests/test_step_matrix_cpu.py holds the two equal)
GAR_ARGS = {"geomed": dict(nu=1e-6 * math.sqrt(4099), iters=8), "cclip": dict(tau=2.0, iters=3),
            "caf": dict(power_iters=sc.T_END_TO_END), "dnc": dict(power_iters=sc.T_END_TO_END)}
M_ARG = 3            # Krum / Bulyan "with m"
D = 1027             # a 16-byte body that fills a workgroup and a tail of 3; target_idx = -1 falls in the tail
INTERIOR = 517
MU = DAMP = 0.9
NB_PAST = 3
STEPS = 3

Attack = collections.namedtuple("Attack", "key name factor args negative")  # negative: the factor it takes on that axis
ATTACKS = (
  Attack("empire", "empire", 1.1, None, -1.1),
  Attack("little", "little", 1.5, None, -1.5),
  Attack("anticge", "anticge", 1.1, None, None),
  Attack("nan", "nan", 1.1, None, None),
  Attack("hidden-last", "hidden", 1.5, {"target_idx": -1}, -1.5),
  Attack("hidden-interior", "hidden", 2.0, {"target_idx": INTERIOR}, -2.0),
  Attack("hidden-all", "hidden", 0.75, {"target_idx": "all"}, -0.75),
  Attack("empire-strict", "empire-strict", 2, None, None),
  Attack("minmax-unit", "minmax", 1.1, {"perturbation": "unit"}, None),
  Attack("minmax-std", "minmax", 1.1, {"perturbation": "std"}, None),
  Attack("minmax-sign", "minmax", 1.1, {"perturbation": "sign"}, None),
  Attack("minsum", "minsum", 1.1, None, None),
)
ATTACK = {a.key: a for a in ATTACKS}
FIRST_PASS_ATTACKS = ("empire", "little")       # the attacks the first pass forms itself
FF = ((11, 2, 2), (11, 2, 1), (11, 2, 0), (25, 5, 5))  # (n, f_decl, f_real)
# What the constructor refuses within the universe (each raises ValueError): empire-strict takes a positive int epsilon
# and has no `negative`, so the negative-factor axis does not reach it.
REFUSED = (dict(attack="empire-strict", attack_factor=-2), dict(attack="empire-strict", attack_factor=2, attack_negative=True))

# Thresholds a decision of the loop must clear, each the one its piece already uses; 1e-4 relative where none exists.
MARGINS = {"krum": 1e-4, "bulyan": 1e-4, "brute": 1e-4, "aksel": 1e-4, "cge": 1e-4, "clip": 1e-4,
           "bulyan_window": 0.999,  # share of Bulyan's columns decided beyond fp32 resolution (bulyan_pass2_f64)
           "anticge": A.MIN_NORM_GAP, "lambda": sc.MIN_MARGIN, "mass": sc.MIN_MARGIN, "dnc": sc.MIN_MARGIN, "minmax": 1e-3}

Case = collections.namedtuple("Case", "name rule attack placement n f_decl f_real clip m with_l2 single_call factor d seed group")


def gar_args(case):
  args = dict(GAR_ARGS.get(case.rule, {}))
  if case.m is not None:
    args["m"] = case.m
  return args


def nb_past_of(case):
  """NB_PAST, or what a case that carries an `nb_past` of its own says (tests/graph_matrix.py: 0)."""
  return getattr(case, "nb_past", NB_PAST)


def constructor_kwargs(case):
  """The keyword arguments of AggregationStep for a case (all but the aggregator)."""
  att = ATTACK[case.attack]
  return dict(nb_workers=case.n, nb_decl_byz=case.f_decl, nb_real_byz=case.f_real, gar=case.rule, gar_args=gar_args(case),
              momentum=MU, dampening=DAMP, momentum_at=case.placement, attack=att.name, attack_factor=case.factor,
              nb_past=nb_past_of(case), gradient_clip=case.clip, single_call=case.single_call, attack_args=att.args)


def sampled_rows(seed, it, count, d):
  """Seeded sampled gradients of step `it`: a common drift and worker noises whose scales are 12 % apart, in an order
  that is not the rows' (the last honest row is not the largest: a selection that confuses h with n - f_decl shows) —
  the norms concentrate within 2 % of their scale at d = 1027, so the rows keep their order by norm at every step."""
  gen = torch.Generator().manual_seed(7000 + 100 * seed + it)
  base = 0.2 * torch.randn(d, generator=gen)
  return [base + 0.5 * 1.12 ** ((11 * i + 5) % 26) * torch.randn(d, generator=gen) for i in range(count)]


def inputs(case):
  """[(sampled rows, params or None, origin or None)] of the case's steps; step 2 samples one gradient more than h.
  The parameters move by a fixed seeded vector per step (the comparison needs no model)."""
  h = case.n - case.f_real
  gen = torch.Generator().manual_seed(50 + case.seed)
  origin = torch.randn(case.d, generator=gen)
  out = []
  for it in range(STEPS):
    params = origin + 0.05 * it * torch.randn(case.d, generator=gen)
    rows = sampled_rows(case.seed, it, h + (1 if it == 2 else 0), case.d)
    out.append((rows, params if case.with_l2 else None, origin if case.with_l2 else None))
  return out


def clip_value(n, f_real, seed, d):
  """A clipping norm that separates the same few largest honest rows from the others at every step (the scales of the
  rows are fixed, their norms concentrate): one row where the draws allow it, so that the rows below keep distinct norms
  and the rankings by norm (CGE, anticge) stay decided.  tests/test_step_matrix_cpu.py asserts some-but-not-all on every
  step."""
  steps = [sorted((_norm64(g) for g in sampled_rows(seed, it, n - f_real, d)), reverse=True) for it in range(STEPS)]
  for k in range(1, n - f_real):  # the k largest rows of every step above, the others below: the smallest such k
    lo, hi = max(norms[k] for norms in steps), min(norms[k - 1] for norms in steps)
    if hi - lo > 0.01 * hi:
      return round(0.5 * (lo + hi), 1)
  raise AssertionError("no clipping norm separates the same rows at every step")


# Seeds of the cases whose default draw (seed 0) puts a decision under its threshold (a seed search over
# MatrixLoop's margins lists them): chosen once, then fixed.
SEEDS = {"dnc-hidden-last-update": 1, "dnc-hidden-all-update": 1}  # (seed 0: DnC's last removal under sc.MIN_MARGIN)


def _case(rule, att, placement, ff, clip, negative, m, with_l2, single_call, group="product", d=D, tag=""):
  n, f_decl, f_real = ff
  factor = att.negative if negative and att.negative is not None else att.factor
  name = f"{rule}-{att.key}-{placement}" + tag
  seed = SEEDS.get(name, 0)
  return Case(name, rule, att.key, placement, n, f_decl, f_real, clip_value(n, f_real, seed, d) if clip else None,
              m if rule in DISTANCE else None, with_l2, single_call, factor, d, seed, group)


_CASES = None


def cases():
  global _CASES
  if _CASES is not None:
    return _CASES
  out = []
  for (i, rule), (j, att), (k, placement) in itertools.product(enumerate(RULES), enumerate(ATTACKS), enumerate(PLACEMENTS)):
    ff = FF[(i + 2 * j + k) % 4]
    if rule == "brute":  # Brute at n = 25 is C(25, 5) subsets in Python on the oracle's side: one case of it
      ff = FF[3] if (j, k) == (0, 2) else FF[(i + j + k) % 3]
    out.append(_case(rule, att, placement, ff, clip=(i + j + k) % 2 == 1, negative=(i + k) % 2 == 1,
                     m=M_ARG if (j + k) % 2 == 1 else None, with_l2=(j + k) % 2 == 0, single_call=(i + j) % 2 == 0))
  for rule in DISTANCE + COLWISE:
    for key in FIRST_PASS_ATTACKS:
      for ff, single in itertools.product((FF[0], FF[2]), (True, False)):
        out.append(_case(rule, ATTACK[key], "worker", ff, clip=False, negative=False, m=None, with_l2=True,
                         single_call=single, group="plan", tag=f"-plan-f{ff[2]}-{'single' if single else 'sequence'}"))
  assert len({c.name for c in out}) == len(out)
  _CASES = out
  return out


def long_cases(cus=256):
  """The first pass riding along (plan.first_pass "rule" / "sqdist") where the mirror of the dispatch says the fused
  instance launches, and at a multiple of 4 where it falls back.  tests/first_pass_matrix.is_fused: the rule rides along
  at (h, f_real) = (20, 5) and (14, 11) only — never at n = 11 —, from d = 4 on at worker placement and at multiples of 4
  at update placement; the distance pass rides along from d / 4 >= 8 x 512 x CUs on (4 194 304 floats at 256 CUs).  So:
    * the four coordinate-wise rules at n = 25, f = 5: worker d = 1028 (fused, no tail; d = 1027 of the product is fused
      with a tail), update d = 1028 (fused) and update d = 1027 (falls back: no multiple of 4) — the shortest lengths the
      mirror allows;
    * Krum and Bulyan at n = 25, f = 5, worker and update, d = 8 x 512 x cus x 4 = 4 194 304 at 256 CUs: the shortest length
      at which the distance pass rides along (bm_momentum_stats_sqdist / bm_stack_stats_sqdist hand their matrix to
      rule_from_sq).  The float64 loop takes tens of seconds on such a case: it runs in step with the device and is not
      kept (step_matrix.run_case);
    * Krum and Bulyan at n = 11, worker and update: d = first_pass_matrix.burst_lengths(4, cus)[0] = 524 288, a multiple of
      4 at which the distance pass falls back to its own launch (it always does at n = 11).
  tests/test_gpu_step_matrix.py asserts of every one of them that the mirror says what its name says, on the device's own
  count of compute units."""
  from tests import first_pass_matrix as FP
  out = []
  for rule in COLWISE:
    for placement in ("worker", "update"):
      for key in FIRST_PASS_ATTACKS:
        out.append(_case(rule, ATTACK[key], placement, FF[3], clip=placement == "worker" and key == "little", negative=False,
                         m=None, with_l2=False, single_call=False, group="long", d=1028, tag="-fused-d1028"))
    out.append(_case(rule, ATTACK["empire"], "update", FF[3], clip=False, negative=False, m=None, with_l2=False,
                     single_call=False, group="long", d=D, tag=f"-fallback-d{D}"))
  ride = 8 * FP.K_STEP_BURST_BLOCK * cus * 4
  for rule in DISTANCE:
    for placement in ("worker", "update"):
      out.append(_case(rule, ATTACK["empire"], placement, FF[3], clip=False, negative=False, m=None, with_l2=False,
                       single_call=False, group="long", d=ride, tag=f"-fused-d{ride}"))
  burst = min(FP.burst_lengths(4, cus))
  for rule in DISTANCE:
    for placement in ("worker", "update"):
      out.append(_case(rule, ATTACK["empire"], placement, FF[0], clip=False, negative=False, m=None, with_l2=False,
                       single_call=False, group="long", d=burst, tag=f"-fallback-d{burst}"))
  return out


def first_pass_entry(case):
  """(entry of tests/first_pass_matrix, ks, h, nb) the case's first pass calls on steps 0 and 1, None when plain."""
  if case.attack not in FIRST_PASS_ATTACKS or case.f_real < 1 or case.placement == "server":
    return None
  if case.rule not in COLWISE + DISTANCE:
    return None
  h = case.n - case.f_real
  stem = "ms_" if case.placement == "worker" else "ss_"
  return stem + ("colwise" if case.rule in COLWISE else "sqdist"), h, h, case.f_real


# ---------------------------------------------------------------------------------------------------------------------
# The float64 statement of the step

Expected = collections.namedtuple(
  "Expected", "defense update byzantine honests server cclip_start floats gamma info margins clipped scale allowance decisions")

TWINS = ("attack_on_sampled", "rule_f_real", "clip_after_momentum", "cclip_restart", "update_no_dampening",
         "study_on_direction", "accept_vs_decl", "extra_in_honests")


def _norm64(t):
  return math.sqrt(t.double().pow(2).sum().item())


def _gap(lo, hi):
  """Relative gap of two sorted keys; inf when the larger is not finite: a NaN row ranks last, undisputed, and two keys
  that are both non-finite are ordered by index, not by value (the reference's sort is stable; Aksel under the nan
  attack, whose median is NaN everywhere)."""
  if not math.isfinite(hi):
    return math.inf
  return (hi - lo) / hi if hi > 0 else 0.0


def _boundary(order, keys, grads, positions):
  """Smallest relative gap between the keys at order[p - 1] and order[p] for p in `positions`, rows that are the same
  object (the Byzantine copies: either gives the same result) left out."""
  worst = math.inf
  for p in positions:
    if 0 < p < len(order) and grads[order[p - 1]] is not grads[order[p]]:
      worst = min(worst, _gap(keys[order[p - 1]], keys[order[p]]))
  return worst


def _mean64(rows):
  acc = torch.zeros_like(rows[0], dtype=torch.float64)
  for r in rows:
    acc = acc + r.double()
  return acc / len(rows)


def brute_f64(grads, f, h):
  """(selection, margin): the subset of n - f rows of smallest diameter on float64 distances and the relative gap to the
  best subset that holds OTHER rows (Byzantine copies are interchangeable).  The diameter of a subset is the largest
  distance none of whose ends was removed: pairs in descending order, every subset at once."""
  n = len(grads)
  dist = O.pairwise_distances(grads, "f64", clamp_nonfinite=False)
  removed = np.array(list(itertools.combinations(range(n), f)), dtype=np.int64).reshape(-1, f)
  out = np.zeros((len(removed), n), dtype=bool)
  out[np.arange(len(removed))[:, None], removed] = True
  pairs = sorted(((dist[x, y], x, y) for x in range(n) for y in range(x + 1, n)),
                 key=lambda p: -p[0] if math.isfinite(p[0]) else -math.inf)
  diam = np.full(len(removed), -1.0)
  for v, x, y in pairs:
    both = ~out[:, x] & ~out[:, y] & (diam < 0)
    diam[both] = v if math.isfinite(v) else math.inf
  diam[diam < 0] = 0.0
  # the kept honest rows and the NUMBER of kept Byzantine copies identify a subset up to interchangeable rows
  copies = (~out[:, h:]).sum(axis=1)
  best = {}
  for idx in np.argsort(diam, kind="stable"):
    key = (out[idx, :h].tobytes(), int(copies[idx]))
    if key not in best:
      best[key] = idx
      if len(best) == 2:
        break
  first, *second = list(best.values())
  assert math.isfinite(diam[first]), "no admissible subset"
  margin = _gap(diam[first], diam[second[0]]) if second else math.inf
  # (the reference returns the FIRST subset in lexicographic order among equals: the lowest indices of the copies)
  ties = np.nonzero(diam == diam[first])[0]
  sel = min(([i for i in range(n) if not out[t, i]] for t in ties))
  return sel, margin


def bulyan_pass2_f64(grads, order, f, m, observed):
  """Bulyan's second pass (bulyan.py:64-82) in float64 on the ranking `order`, as oracle.gar_oracle.bulyan has it, for a
  run in step with the device -> (output, share of the columns decided beyond fp32 resolution).
  Per column the pass averages the beta values nearest the median of theta averaged selections: a decision per column,
  millions of them in a long case, and some are bound to lie within the fp32 rounding of the selections (each the fp32
  mean of up to m rows: (m + 3) 2^-24 of the column's largest value).  In such a column — the gap between the beta-th
  and the (beta + 1)-th deviation at most that — both windows are legal, as tests/test_gpu_parity_r2.py has it for an
  exact tie, and the one nearer `observed` is the expectation: every later step of the loop then carries the same
  column.  Everywhere else the output is the float64 one, whatever was observed."""
  n = len(grads)
  m_max, theta = n - f - 2, n - 2 * f - 2
  beta = theta - 2 * f
  picked = []
  for i in range(theta):
    count = min(m, m_max - i)
    picked.append(_mean64([grads[g] for g in order[i:i + count]]))
  sel = torch.stack(picked)
  centre = sel.median(dim=0).values
  dev, idx = (sel - centre).abs().sort(dim=0)
  out = sel.gather(0, idx[:beta]).mean(dim=0)
  if beta >= theta:
    return out, 1.0
  tol = (m + 3) * 2.0 ** -24 * sel.abs().max(dim=0).values
  close = (dev[beta] - dev[beta - 1]) <= tol   # (a NaN column compares False: it keeps the float64 output)
  alt = out + (sel.gather(0, idx[beta:beta + 1])[0] - sel.gather(0, idx[beta - 1:beta])[0]) / beta
  seen = observed.double()
  swap = close & ((seen - alt).abs() < (seen - out).abs())
  return torch.where(swap, alt, out), 1.0 - float(close.double().mean())


class MatrixLoop(Loop):
  """One case's steps in float64.  step() -> Expected.  `twin`: one of TWINS, a plausible host-logic mistake built in on
  purpose (tests/test_step_matrix_cpu.py shows that the comparison catches each)."""

  def __init__(self, case, twin=None):
    super().__init__(case.n, case.f_decl, case.f_real, case.rule, case.placement, MU, DAMP, case.clip, nb_past_of(case))
    self.case, self.att, self.twin = case, ATTACK[case.attack], twin
    self.args = gar_args(case)
    self.start = None      # cclip: the previous defense
    self.server64 = None   # the server momentum in float64 (server / update placements)

  # -- step 0 / 1: clipping and momentum (the base class, with the fp32 clipping factor) -- #

  def begin(self, sampled, clip_f32=True):
    margin = math.inf
    clipped = []
    if self.clip is not None:
      for g in sampled:
        norm = _norm64(g)
        margin = min(margin, abs(norm - self.clip) / self.clip)
        clipped.append(norm > self.clip)
    self._clip_margin, self._clipped = margin, clipped
    if self.momentum_at == "server" and self.server64 is not None:
      self.server = self.server64.float()  # (the base class reads `self.server` as the fp32 tensor the step keeps)
    if self.twin == "clip_after_momentum" and self.clip is not None:
      clip, self.clip = self.clip, None
      try:
        honests, _ = super().begin(sampled, clip_f32)
      finally:
        self.clip = clip
      for g in honests:
        norm = _norm64(g)
        if norm > clip:
          g.mul_(clip / norm)
      kept, _ = self._now
      self._now = (kept, honests)
      return honests, None
    return super().begin(sampled, clip_f32)

  # -- step 2: the Byzantine vector -- #

  def byzantine(self, honests, source=None):
    """(vector float64 or None, gamma, info, margins) from the honest rows (fp32 tensors)."""
    att, rows = self.att, list(source if source is not None else honests)
    if self.f_real == 0:
      return None, None, None, {}
    return byzantine_vector(att.name, rows, self.case.factor, att.args, self.f_decl, self.f_real)

  # -- step 3: the rule -- #

  def aggregate(self, grads, f, observed=None):
    """(defense float64, acceptation ratio, margins) of the rule on float64 rows (the copies of the Byzantine vector being
    ONE object, as in the step)."""
    gar, n, h, args = self.gar, len(grads), self.h, self.args
    nan, margins = math.nan, {}
    h_count = self.n - self.f_decl if self.twin == "accept_vs_decl" else h

    def ratio(selected):
      return sum(1 for i in selected if i >= h_count) / len(selected)

    if gar in ("krum", "bulyan"):
      m_max = n - f - 2
      m = args.get("m") or m_max
      if gar == "krum":
        order, scores = O.krum_order(grads, f, "f64")
        margins["krum"] = _boundary(order, scores, grads, [m])
        return _mean64([grads[i] for i in order[:m]]), ratio(order[:m]), margins
      order, scores = O.bulyan_order(grads, f, m, "f64")
      margins["bulyan"] = _boundary(order, scores, grads, range(1, m_max + 1))
      if observed is None:
        return O.bulyan(grads, f, m, "f64"), nan, margins
      out, margins["bulyan_window"] = bulyan_pass2_f64(grads, order, f, m, observed)
      return out, nan, margins
    if gar == "median":
      return O.median(grads, "f64"), nan, margins
    if gar in ("trmean", "phocas", "meamed"):
      return getattr(O, gar)(grads, f, "f64"), nan, margins
    if gar == "average":
      return _mean64(grads), self.f_real / self.n, margins
    if gar == "aksel":
      count = (n + 1) // 2
      order, keys = O.aksel_order(grads, "f64")
      margins["aksel"] = _boundary(order, keys, grads, [count])
      return _mean64([grads[i] for i in order[:count]]), ratio(order[:count]), margins
    if gar == "brute":
      sel, margins["brute"] = brute_f64(grads, f, h)
      return _mean64([grads[i] for i in sel]), ratio(sel), margins
    if gar == "cge":
      return self._cge(grads, f, observed, ratio, margins)
    rows = np.stack([g.double().numpy() for g in grads])
    if gar in CENTER:
      usable = sc.usable_rows(rows)
      start = None if self.start is None or self.twin == "cclip_restart" else self.start.numpy()
      radius = args["nu"] if gar == "geomed" else args["tau"]
      v, _ = cc.vector_iteration(rows[usable], gar, radius, args["iters"], 0.0, start if gar == "cclip" else None)
      return torch.from_numpy(v), nan, margins
    count = f if gar == "caf" else min(int(math.ceil(1.0 * f)), max(n - 1, 0))
    ref = sc.vector_spectral(rows, gar, count, args["power_iters"])
    margins.update({key: value for key, value in ref.margins.items()})
    self._decisions = dict(rounds=ref.rounds, kept=ref.kept, zero=[bool(w == 0) for w in ref.weights])
    return torch.from_numpy(ref.out), nan, margins

  def _cge(self, grads, f, observed, ratio, margins):
    """CGE on float64 norms.  Against anticge the attack puts its vector within ONE fp32 rounding of the norm of a row
    CGE may keep (anticge.py:66-68): no arithmetic resolves which is smaller, the reference's own does not either.  As
    tests/anticge_reference.AnticgeLoop.finish: the ranking is also taken with the Byzantine norms moved by 1e-6 either
    way, and the admissible defense closest to `observed` is the expectation ("cge_choice" says which)."""
    n, h, keep = len(grads), self.h, len(grads) - f

    def ranked(scale):
      norms = [_norm64(g) * (scale if i >= h else 1.0) for i, g in enumerate(grads)]
      keys = [v if math.isfinite(v) else math.inf for v in norms]
      return sorted(range(n), key=lambda i: keys[i]), keys

    order, keys = ranked(1.0)
    disputed = self.att.name == "anticge" and 0 < self.f_real <= self.f_decl
    self.cge_choice = 1.0
    if disputed:
      # the one decision taken at a rounding by construction is left out of the margin: Byzantine copy against honest row
      honest = [i for i in order if i < h]
      margins["cge"] = _boundary(honest, keys, grads, range(1, len(honest)))
      if observed is not None:
        best = float((_mean64([grads[i] for i in order[:keep]]) - observed.double()).abs().max())
        for scale in (1 - 1e-6, 1 + 1e-6):
          other, _ = ranked(scale)
          err = float((_mean64([grads[i] for i in other[:keep]]) - observed.double()).abs().max())
          if err < best:
            best, order, self.cge_choice = err, other, scale
    else:
      margins["cge"] = _boundary(order, keys, grads, [keep])
    return _mean64([grads[i] for i in order[:keep]]), ratio(order[:keep]), margins

  # -- the whole step -- #

  def step(self, sampled, params=None, origin=None, observed=None):
    case, h, twin = self.case, self.h, self.twin
    honests, _ = self.begin(sampled)
    kept, _ = self._now                      # the sampled rows after clipping
    if twin == "extra_in_honests" and self.momentum_at != "worker" and len(kept) > h:
      extra = kept[h:]
      if self.momentum_at == "server":
        extra = [g.mul(1. - self.damp).add_(self.server, alpha=self.mu) for g in extra]
      honests = honests + [g.clone() for g in extra]
      self._now = (kept, honests)
    source = kept[:h] if twin == "attack_on_sampled" and self.momentum_at == "worker" else None
    byz, gamma, info, margins = self.byzantine(honests, source)
    margins = dict(margins)
    if self.clip is not None:
      margins["clip"] = self._clip_margin
    rows64 = [g.double() for g in honests]
    attacks = [byz] * self.f_real if byz is not None else []
    self._decisions = None
    defense, accept, rule_margins = self.aggregate(rows64 + attacks, self.f_real if twin == "rule_f_real" else self.f_decl,
                                                   observed)
    margins.update(rule_margins)
    if self.gar == "cclip":
      self.start = defense
    if self.server64 is None:
      self.server64 = torch.zeros_like(defense)
    if self.momentum_at == "server":
      self.server64 = defense
      update = defense
    elif self.momentum_at == "update":
      self.server64 = self.mu * self.server64 + (1.0 if twin == "update_no_dampening" else 1. - self.damp) * defense
      update = self.server64
    else:
      update = defense
    studied = attacks
    if twin == "study_on_direction" and byz is not None:
      studied = [byz - _mean64(honests)] * self.f_real
    res = study_block(kept, honests, studied, defense, list(self.pasts) if self.nb_past > 0 else [], self.mu)
    res["accept_ratio"] = accept
    res["l2_origin"] = _norm64(params - origin) if params is not None and origin is not None else math.nan
    if self.nb_past > 0:
      self.pasts.appendleft((res["sampled_grad_avg"], res["sampled_norm_avg"]))
    floats = {key: value for key, value in res.items() if isinstance(value, float)}
    scale = float(torch.stack(list(sampled)).abs().max())
    allowance = None
    if info is not None and not info["degenerate"]:  # tests/test_gpu_minmax.py (10): the allowance of the vector, per coordinate
      p, g = np.abs(info["p"]), info["gamma"]
      rows = np.stack([r.double().numpy() for r in honests])
      allowance = torch.from_numpy(g * p), torch.from_numpy((h + 4) * 2.0 ** -24 * (np.abs(rows).max(axis=0) + g * p))
    return Expected(defense, update, byz, [g.clone() for g in honests] if self.momentum_at == "worker" else None,
                    self.server64.clone() if self.momentum_at != "worker" else None,
                    self.start.clone() if self.start is not None else None, floats, gamma, info, margins,
                    list(self._clipped), scale, allowance, self._decisions)


def study_block(sampled, honests, attacks, defense, pasts, momentum):
  """oracle.gar_oracle.study_block at precision "f64" with the sampled and the honest average as the step's contract has
  them: the sequential fp32 mean the first pass writes (tests/first_pass_matrix.py holds it bit for bit), the deviations
  centred at it.  The attack average and the defense stay float64."""
  from tests.attack_vectors_reference import seq_mean

  def stats(rows, fp32_mean):
    if not rows:
      return None, math.nan, math.nan, math.nan
    avg = seq_mean([g.clone() for g in rows]).double() if fp32_mean else _mean64(rows)
    dev = math.sqrt(sum((g.double() - avg).pow(2).sum().item() for g in rows) / (len(rows) - 1)) if len(rows) >= 2 else math.nan
    return avg, _norm64(avg), dev, avg.abs().max().item()

  s_avg, s_norm, s_dev, s_max = stats(sampled, True)
  h_avg, h_norm, h_dev, h_max = stats(honests, True)
  a_avg, a_norm, a_dev, a_max = stats(attacks, False)
  d_norm, d_max = _norm64(defense), defense.abs().max().item()

  def cos(u, nu, v, nv):
    return math.nan if u is None or v is None else torch.dot(u, v).div_(nu).div_(nv).item()

  res = {
    "sampled_norm_dev": s_dev, "honest_norm_dev": h_dev, "attack_norm_dev": a_dev,
    "sampled_norm_avg": s_norm, "honest_norm_avg": h_norm, "attack_norm_avg": a_norm, "defense_norm_avg": d_norm,
    "sampled_norm_max": s_max, "honest_norm_max": h_max, "attack_norm_max": a_max, "defense_norm_max": d_max,
    "cosin_splhon": cos(s_avg, s_norm, h_avg, h_norm), "cosin_splatt": cos(s_avg, s_norm, a_avg, a_norm),
    "cosin_spldef": cos(s_avg, s_norm, defense, d_norm), "cosin_honatt": cos(h_avg, h_norm, a_avg, a_norm),
    "cosin_hondef": cos(h_avg, h_norm, defense, d_norm), "cosin_attdef": cos(a_avg, a_norm, defense, d_norm),
    "cosin_sampled": math.nan, "curv_sampled": math.nan,
  }
  if len(pasts) > 0:
    res["cosin_sampled"] = torch.dot(s_avg, pasts[0][0]).div_(s_norm).div_(pasts[0][1]).item()
    res["curv_sampled"] = momentum * sum(momentum ** i * torch.dot(s_avg, p).item() for i, (p, _) in enumerate(pasts))
  res["sampled_grad_avg"] = s_avg
  return res


def byzantine_vector(name, honests, factor=None, args=None, f_decl=None, f_real=None):
  """(vector float64, gamma or None, minmax_reference's record or None, margins) of an attack on fp32 honest rows.  The
  honest mean is the sequential fp32 mean the first pass leaves (tests/attack_vectors_reference.seq_mean) for the
  attacks the reference ships — its restatements use it —, the float64 mean for Min-Max / Min-Sum (minmax_reference)."""
  from tests.attack_vectors_reference import seq_mean
  args = dict(args or {})
  avg = seq_mean([g.clone() for g in honests]).double()
  if name == "nan":
    return torch.full_like(avg, math.nan), None, None, {}
  if name == "empire":
    return avg + factor * (-avg), None, None, {}
  if name == "little":
    std = torch.stack([g.double() for g in honests]).var(dim=0).sqrt()
    return avg + factor * std, None, None, {}
  if name == "hidden":
    return avg + factor * direction_of(avg, args.get("target_idx", -1)), None, None, {}
  if name == "empire-strict":
    return avg * (-factor), None, None, {}
  if name == "anticge":
    vector = A.anticge_f64(honests, f_decl, f_real).vector
    gap = math.inf
    if f_real <= f_decl:  # the rows the attack reads and the first one it leaves out (tests/test_gpu_anticge.selected_gap)
      ranked = sorted(honests, key=lambda g: g.double().pow(2).sum().item())
      gap = A.norm_gap(ranked[:len(honests) - f_decl + 1])
    return vector, None, None, {"anticge": gap}
  assert name in MR.MODES, name
  rows = np.stack([g.double().numpy() for g in honests])
  res = MR.attack(rows, args.get("perturbation", "std"), name)
  margins = {}
  if name == "minmax" and res["gammas"] is not None and len(res["gammas"]) > 1:
    two = np.sort(res["gammas"])[:2]
    margins["minmax"] = float((two[1] - two[0]) / two[1])
  return torch.from_numpy(res["vector"]), res["gamma"], res, margins


def below_margin(margins):
  """{decision: margin} of the decisions closer than their threshold."""
  return {key: value for key, value in margins.items() if key in MARGINS and not value >= MARGINS[key]}


# ---------------------------------------------------------------------------------------------------------------------
# Bars and the comparison (shared by the CPU run, the GPU run and the probe)

BAR_RULE = 2e-6              # x max|sampled|: the reference's rules (tests/test_gpu_parity_r2.py, tests/test_gpu_anticge.py)
BAR_GAMMA = 1.21e-07         # tests/test_gpu_minmax.py (10)
FLOATS_TOL = 1e-5


def rule_bar(rule):
  """(measure, bar) of a rule's d-sized outputs: "abs" = max|got - want| / max|sampled|, "norm" = |got - want| / |want|."""
  if rule in CENTER:
    return "norm", cc.BAR_B[rule]
  if rule in SPECTRAL:
    return "norm", sc.BAR_B[rule]
  return "abs", BAR_RULE


def floats_bar(rule):
  return cc.FLOATS_BAR if rule in CENTER + SPECTRAL else FLOATS_TOL


# {(rule, attack key): {quantity: bar}}: combinations whose measured error on an MI355X exceeds the bars above while
# every decision agrees — 4 x the worst of profiles/step_matrix_errors.txt (scripts/step_matrix_probe.py).
# Measured: the d-sized outputs (defense, update, server_momentum) in relative norm, the rule's measure —
#   geomed x hidden-last   worst 5.963e-07 (bar of the rule alone 4.080e-07)  -> 2.385e-06
#   caf x little           worst 4.576e-07 (4.072e-07)                        -> 1.830e-06
#   dnc x anticge          worst 4.321e-07 (3.897e-07)                        -> 1.728e-06
# Every decision of the device agrees with the loop's in these cases (geomed takes none; the filters' rounds, kept round
# and removed rows are compared).  The rules' own bars were measured on rows mu + N(0, 1), whose aggregate is about as
# long as a row (mean|x| is 1.2 x |aggregate| in norm); the rows here differ in scale by up to 13 x around a small common
# drift (2.3 x for geomed x hidden-last), so the fp32 roundings of the weights and of the sum weigh more against it.
#   floats()["curv_sampled"] — mu x sum_i mu^i <s, past_i>, which involves neither rule nor attack — under the center and
#   spectral rules: worst 1.134e-06 (geomed, caf, dnc x six attacks, one stream of sampled gradients, step 2;
#   center_cases.FLOATS_BAR 7.772e-07) -> 4.536e-06 for EVERY combination of those four rules, the quantity being the
#   same whatever the rule (dnc x hidden-last stood at 7.535e-07).
#   (FLOATS_BAR was measured against the oracle-backed step, which keeps the fp32 running combination C of the past
#   averages as the device does; the loop sums float64 dot products with every past average.  The reference's rules hold
#   the same key, with the same error, to 1e-5.)
_D_SIZED = ("defense", "update", "server_momentum", "cclip_start")
MEASURED_BARS = {(rule, attack.key): {"floats.curv_sampled": 4 * 1.134e-06} for rule in CENTER + SPECTRAL for attack in ATTACKS}
for _combination, _worst in ((("geomed", "hidden-last"), 5.963e-07), (("caf", "little"), 4.576e-07),
                             (("dnc", "anticge"), 4.321e-07)):
  MEASURED_BARS.setdefault(_combination, {}).update(dict.fromkeys(_D_SIZED, 4 * _worst))


def vector_error(got, want, measure, scale):
  """Error of a d-sized output in the rule's measure, over the coordinates where the expectation is finite; inf where
  the two are not non-finite at exactly the same coordinates."""
  got, want = got.detach().cpu().double(), want.double()
  if not torch.equal(torch.isfinite(got), torch.isfinite(want)):
    return math.inf
  mask = torch.isfinite(want)
  if not bool(mask.any()):
    return 0.0
  diff = (got - want)[mask]
  if measure == "norm":
    return float(diff.norm() / want[mask].norm())
  return float(diff.abs().max()) / scale


def errors(case, step, got_defense, exp):
  """{quantity: (error, bar)} of one step of an AggregationStep against the loop's Expected, every compared quantity:
  defense, update_gradient(), last_byzantine, buffers / server_momentum, cclip_start, every key of floats(), gamma."""
  measure, bar = rule_bar(case.rule)
  out = {}

  def vec(name, got, want):
    b = MEASURED_BARS.get((case.rule, case.attack), {}).get(name, bar)
    out[name] = (vector_error(got, want, measure, exp.scale), b)

  # (minmax / minsum: their allowance holds the Byzantine vector and gamma below; the rule's outputs keep the rule's own
  # bar — measured, every such combination is inside it)
  vec("defense", got_defense, exp.defense)
  vec("update", step.update_gradient(), exp.update)
  byz = step.last_byzantine
  if exp.byzantine is None:
    out["byzantine"] = (0.0 if byz is None else math.inf, 0.0)
  elif byz is None:
    out["byzantine"] = (math.inf, 0.0)
  elif exp.allowance is not None:  # per coordinate, in units of the allowance (tests/test_gpu_minmax.py (10))
    allowed = BAR_GAMMA * exp.allowance[0] + exp.allowance[1]
    excess = (byz.detach().cpu().double() - exp.byzantine).abs() / allowed.clamp_min(1e-300)
    out["byzantine"] = (float(excess.max()), MEASURED_BARS.get((case.rule, case.attack), {}).get("byzantine", 1.0))
  else:
    out["byzantine"] = (vector_error(byz, exp.byzantine, "abs", exp.scale),
                        MEASURED_BARS.get((case.rule, case.attack), {}).get("byzantine", BAR_RULE))
  if exp.gamma is not None:
    info = byz.attack_info.detach().cpu().tolist()
    factor = float(step.last_factor.reshape(-1)[0]) if isinstance(step.last_factor, torch.Tensor) else float(step.last_factor)
    err = max(abs(info[0] - exp.gamma), abs(factor - exp.gamma)) / exp.gamma if exp.gamma > 0 else math.inf
    if info[5] != 0.0 or (exp.info["binding"] >= 0 and exp.margins.get("minmax", 0) >= MARGINS["minmax"]
                          and info[2] != exp.info["binding"]):
      err = math.inf
    out["gamma"] = (err, MEASURED_BARS.get((case.rule, case.attack), {}).get("gamma", BAR_GAMMA))
  if exp.honests is not None:
    worst = max(vector_error(g, w, "abs", exp.scale) for g, w in zip(step.buffers, exp.honests))
    out["buffers"] = (worst if len(step.buffers) == len(exp.honests) else math.inf, BAR_RULE)
  else:
    vec("server_momentum", step.server_momentum, exp.server)
  if exp.cclip_start is not None:
    vec("cclip_start", step.cclip_start, exp.cclip_start)
  else:
    out["cclip_start"] = (0.0 if step.cclip_start is None else math.inf, 0.0)
  # (the stand-in tests/test_step_matrix_cpu.py makes of a twin's Expected has no aggregator)
  if exp.decisions is not None and hasattr(step, "agg"):  # the filter's decisions: rounds run, round kept, rows left out
    info = step.agg.last_spectral_info.detach().cpu().tolist()
    zero = [bool(w == 0) for w in step.agg.last_weights.detach().cpu().tolist()[:case.n]]
    agree = (int(info[0]), int(info[3])) == (exp.decisions["rounds"], exp.decisions["kept"]) and zero == exp.decisions["zero"]
    out["decisions"] = (0.0 if agree else math.inf, 0.0)
  got = step.floats()
  fbar = floats_bar(case.rule)
  assert set(exp.floats) == set(got), (sorted(exp.floats), sorted(got))
  for key, value in cc.float_errors(got, exp.floats).items():
    out["floats." + key] = (value, MEASURED_BARS.get((case.rule, case.attack), {}).get("floats." + key, fbar))
  if math.isnan(exp.floats["l2_origin"]):
    out["floats.l2_origin"] = (0.0 if math.isnan(got["l2_origin"]) else math.inf, 0.0)
  want = exp.floats["accept_ratio"]
  same = (math.isnan(want) and math.isnan(got["accept_ratio"])) or got["accept_ratio"] == want
  out["floats.accept_ratio"] = (0.0 if same else math.inf, 0.0)
  return out


def failures(errs):
  return {key: pair for key, pair in errs.items() if not pair[0] <= pair[1]}


# ---------------------------------------------------------------------------------------------------------------------
# Running a case

_EXPECTED = {}
KEEP_BELOW = 1 << 20   # coordinates a row above which the loop's expectations of a case are not kept


def expected_of(case):
  """The loop's Expected of every step of a case, computed once and shared by whoever runs the case."""
  if case.name not in _EXPECTED:
    loop = MatrixLoop(case)
    _EXPECTED[case.name] = [loop.step(*step_inputs) for step_inputs in inputs(case)]
  return _EXPECTED[case.name]


def same_bits(a, b):
  """The same bits (a NaN equals the same NaN); None equals None."""
  if a is None or b is None:
    return a is None and b is None
  view = torch.int32 if a.dtype == torch.float32 else torch.int64
  return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def can_take_the_single_call(case):
  """Whether plan.single_call is true with the HIP backend when the case asks for it (step._make_plan, written out in
  tests/test_step_matrix_cpu.expected_plan)."""
  return case.attack in FIRST_PASS_ATTACKS and case.placement == "worker" and case.rule in DISTANCE + COLWISE


def snapshot(step, defense):
  """What two forms of one step must share bit for bit: outputs, buffers and the study row (NaN equal to NaN)."""
  def cpu(t):
    return None if t is None else t.detach().cpu().clone()
  floats = {key: (None if isinstance(value, float) and math.isnan(value) else value) for key, value in step.floats().items()}
  return dict(defense=cpu(defense), update=cpu(step.update_gradient()), byzantine=cpu(step.last_byzantine),
              buffers=None if step.buffers is None else [cpu(b) for b in step.buffers], floats=floats)


def run_case(case, aggregator, device=None, worst=None, record=None, expect_single=None, expectations=None):
  """The case's steps through AggregationStep on `aggregator` (None: the step's own default) against the loop:
  {(step, quantity): (error, bar)} of what misses its bar.  Asserts that no decision of the loop is under its margin
  and that a clipping norm clips some but not all rows.  worst: {quantity: (largest error, its bar)} is updated; record: a list
  that receives a snapshot() per step.  CGE against anticge takes the observed defense (MatrixLoop._cge): that loop
  runs in step with the device.  expect_single: what plan.single_call must be.  expectations: a list — empty, it receives
  the Expected of every step; filled by an earlier form of the same case, it is used instead of running the loop again
  (the long cases, whose loop takes seconds a step)."""
  from byzantinemomentum_amd.step import AggregationStep
  step = AggregationStep(aggregator=aggregator, **constructor_kwargs(case))
  assert expect_single is None or step.plan.single_call is expect_single, (case.name, step.plan.single_call)
  # (in step with the device, nothing kept: CGE against anticge reads the observed defense; a case of millions of
  # coordinates a row would hold gigabytes of expectations)
  in_step = (case.rule == "cge" and case.attack == "anticge" and case.f_real > 0) or case.d > KEEP_BELOW
  loop = MatrixLoop(case) if in_step else None
  bad = {}
  move = (lambda t: t.to(device)) if device is not None else (lambda t: t.clone())
  for it, (sampled, params, origin) in enumerate(inputs(case)):
    got = step.run([move(g) for g in sampled], None if params is None else move(params), None if origin is None else move(origin))
    if expectations is not None and len(expectations) > it:
      exp = expectations[it]
    elif in_step:
      exp = loop.step(sampled, params, origin, observed=got.detach().cpu())
      if expectations is not None:
        expectations.append(exp)
    else:
      exp = expected_of(case)[it]
    under = below_margin(exp.margins)
    assert not under, (case.name, it, under)
    if case.clip is not None:
      assert any(exp.clipped) and not all(exp.clipped), (case.name, it, exp.clipped)
    # (NaN where and only where the expectation is NaN, the rest within 1e-5: the project's own comparison of study rows)
    assert_floats_close_nan(step.floats(), exp.floats, tag=(case.name, it), tol=FLOATS_TOL)
    errs = errors(case, step, got, exp)
    if worst is not None:
      for key, pair in errs.items():
        if key not in worst or pair[0] > worst[key][0]:
          worst[key] = pair
    bad.update({(it, key): pair for key, pair in failures(errs).items()})
    if record is not None:
      record.append(snapshot(step, got))
  return bad
