"""One aggregation step of the simulation loop on the HIP path (mirror of attack.py:757-878).

Given the sampled honest gradients of a step it performs, without leaving the GPU (run() calls one method per step:
0 _clip_factors, 1 _first_pass, 2 _byzantine, 3 _defense, 4 _update_momentum, 5 _study; what each attack needs of them
is one row of the _ATTACK table, what the constructor's arguments decide is the StepPlan):
  0. gradient clipping             g_i <- g_i * clip/||g_i|| where ||g_i|| > clip   attack.py:776-779,791-794
  1. momentum, by placement        worker: buf_i <- mu*buf_i + (1-damp)*g_i            attack.py:800-804
                                   server: hon_i  = (1-damp)*g_i + mu*M                attack.py:805-808
                                   update / none: hon_i = g_i                          attack.py:809-810
  2. the "empire" / "little" attack  byz = avg_h + factor*dir, repeated f_real times   attacks/identical.py:63-86,129-141
                                   factor fixed, or searched within `attack_evals` evaluations of
                                   |GAR(honests + [avg_h + t*dir]*f) - avg_h|^2         attacks/identical.py:67-77
     or the "anticge" attack       byz = -(sum of the h - f_decl smallest honests), scaled to just below the next norm,
                                   repeated f_real times; no factor                     attacks/anticge.py:49-78
     or "minmax" / "minsum"        byz = avg_h + gamma*p, gamma the closed form of the Min-Max / Min-Sum attacks
                                   (Shejwalkar & Houmansadr, NDSS 2021; include/bm_gar.h), p one of three perturbations;
                                   no factor to give or search                          ShardedAggregator.minmax
     or "nan" / "hidden" / "empire-strict"  byz = all NaN | avg_h + factor*(ones or e_target) | avg_h*(-eps), ONE streaming
                                   kernel behind the plain first pass (bm_attack_vector); "hidden" is the reference's
                                   `bulyan` attack, factor and eps fixed or searched   attacks/nan.py:36-40,
                                   attacks/identical.py:114-127, attacks/empire.py:46-64
  3. the aggregation rule          defense = GAR(honests + [byz]*f, f)                 attack.py:821
  4. the momentum of the update    server: M <- defense; update: M <- mu*M + (1-damp)*defense   attack.py:832-839
  5. the study statistics          sampled / honest / attack stacks, defense norm and max, six cosines,
                                   previous-step cosine and curvature, l2 distance from the origin   attack.py:828-868
                                   and the attack acceptation ratio, `defense.influence(honests, attacks, f)`: of the rows
                                   the rule averaged, the fraction that are Byzantine copies          attack.py:822
With worker momentum, steps 0-2 and the sampled/honest statistics of step 5 are ONE kernel
(bm_momentum_stats): every sampled gradient and every momentum buffer is read once.

The step shards along the coordinates like the rules do (sharded.ShardedAggregator): every rank
passes its slice of every tensor; scalars are exchanged in at most three small collectives per
step (row norms if clipping, the n x n squared distances if the rule needs them, and one packed
vector of every statistic), never a d-sized one.  With one rank no collective is issued.
The model update itself (optimizer step) belongs to the caller: `update_gradient()` returns what
attack.py hands to `model.update`.  Everything is asynchronous on the current stream until
`floats()` fetches the scalars (one sync) — except for the factor search, sequential by nature: one
synchronisation per evaluation, or ONE for the whole search when the rule is krum, brute or average
(linesearch.py: every evaluation is then a function of (h+2)^2 scalars of one distance pass).

The acceptation ratio (`floats()["accept_ratio"]`) costs no second ranking and no copy of its own: the rule left its
selection in device memory (krum: the first m of the ranking; brute: the subset; aksel: the first c of the distance
order; cge: the first n - f_decl of the norm order), ONE wavefront counts the entries >= h there (bm_accept_count;
gradients = honests + [byz] * f_real), the integer travels with the scalars above and `floats()` divides it by the
rule's denominator — the reference's own `int / int`.  average: f_real / n on the host; bulyan, median, trmean, phocas,
meamed have no `influence` in the reference: the object math.nan.
"""

import collections
import dataclasses
import math
from typing import Any, NamedTuple, Optional

import torch

from . import _lib, graphs, linesearch, pipelines

__all__ = ["AggregationStep"]

_RULES = ("krum", "bulyan", "median", "trmean", "phocas", "meamed", "aksel", "brute", "average", "cge", "geomed", "cclip",
          "caf", "dnc")
_CENTER = {"geomed": ("nu", "iters", "tol"), "cclip": ("tau", "iters", "tol")}  # rule -> the `gar_args` it takes
_SPECTRAL = {"caf": ("power_iters",), "dnc": ("power_iters", "c")}               # the same for the spectral filters
_COLWISE = ("median", "trmean", "phocas", "meamed")
_DISTANCE = ("krum", "bulyan")
_PRE = {"nnm": ("form",), "bucketing": ("s", "seed", "form")}  # pre-aggregation -> the `pre_args` it takes
MAX_PAST = 4096  # past sampled averages kept for the curvature term (each is one d-vector of device memory)


class _Attack(NamedTuple):
  """What the step needs to know of an attack: one row of _ATTACK per name, read by the constructor, _make_plan, the
  factor search and _byzantine — none of them compares names."""
  formed: str               # who forms the vector: "first_pass" (in its kernel), or behind the PLAIN first pass "chain"
                            # (_CHAIN[first_pass]: ShardedAggregator.anticge / .minmax) / "kernel" (ShardedAggregator.attack_vector)
  kind: Optional[str]       # "kernel": the kind attack_vector is handed ("shift_one": "shift_all" with target_idx "all")
  first_pass: str           # the attack the first pass is handed: what it forms, for empire-strict the direction it forms
                            # for a search (a first pass that forms nothing is handed the name, unread)
  factor: bool              # it has a factor, fixed (`attack_factor`) or searched: it takes `attack_evals`
  negative: bool            # it has the reference's `negative`
  args: frozenset           # the `attack_args` it accepts
  direction: Optional[str]  # what a search moves along: "first_pass" = the first pass in its "direction" form,
                            # "kernel" = the 0 / 1 vector attack_vector leaves at factor 1; None: nothing to search
  shift: float              # added to every abscissa of a search (avg * (-x) is avg + (1 + x) * (-avg): empire.py:51-59)
  apply: Optional[str]      # the found factor: "fma" = multi_fma3 along the direction (identical.py:82-84), "scale" =
                            # attack_vector("scale", avg, -epsilon), the factor being a positive integer epsilon (empire.py:61-62)
  needs: Optional[str] = None  # "chain": what it asks of the worker counts — "f_decl" = 1 <= nb_decl_byz <= honest
                               # workers (anticge.py:67-68), "pair" = at least two honest workers (a distance between two)


_ATTACK = {
  "empire": _Attack("first_pass", None, "empire", True, True, frozenset(), "first_pass", 0.0, "fma"),
  "little": _Attack("first_pass", None, "little", True, True, frozenset(), "first_pass", 0.0, "fma"),
  "anticge": _Attack("chain", None, "anticge", False, True, frozenset(), None, 0.0, None, "f_decl"),
  "nan": _Attack("kernel", "nan", "nan", False, True, frozenset(), None, 0.0, None),
  "hidden": _Attack("kernel", "shift_one", "hidden", True, True, frozenset({"target_idx"}), "kernel", 0.0, "fma"),
  "empire-strict": _Attack("kernel", "scale", "empire", True, False, frozenset(), "first_pass", 1.0, "scale"),
}
_ATTACKS = tuple(_ATTACK)
# The attacks the reference does not ship, in a table of their own (the one above is the reference's, attack for attack):
# the closed-form Min-Max / Min-Sum attacks, chains like anticge.  The constructor looks a name up in both.
_ATTACK_BEYOND = {
  "minmax": _Attack("chain", None, "minmax", False, True, frozenset({"perturbation"}), None, 0.0, None, "pair"),
  "minsum": _Attack("chain", None, "minsum", False, True, frozenset({"perturbation"}), None, 0.0, None, "pair"),
}
_PERTURBATIONS = tuple(_lib.PERTURB_KINDS)
# "chain": the short sequence behind the plain first pass, by the name the row carries as `first_pass` (the first pass
# itself forms nothing and does not read it): (step, honest rows) -> the f_real references to the Byzantine vector
_CHAIN = {
  "anticge": lambda step, honests: step.agg.anticge(honests, step.f_decl, step.f_real),
  "minmax": lambda step, honests: step.agg.minmax(honests, step.f_real, "minmax", step.perturbation),
  "minsum": lambda step, honests: step.agg.minmax(honests, step.f_real, "minsum", step.perturbation),
}


def _attack_row(name):
  return _ATTACK.get(name) or _ATTACK_BEYOND.get(name)


class StepPlan(NamedTuple):
  """The forms a step takes, decided ONCE from the constructor's arguments and the backend's `capabilities`
  (AggregationStep._make_plan).  The stages of run() and _search_factor() read it; they add three run-time facts only,
  each where it matters: ks == h (update placement), whether the vectors are on a GPU, and d
  (bulyan_pass2_eval_supported).  The VALUE of a fixed factor is read from the step when it runs."""
  only_m: bool            # no argument of the rule but "m"
  analytic: bool          # line_search "auto" / "host": the search may use a rule's special form
  first_pass: str         # "rule" / "sqdist": the coordinate-wise rule / the distance pass of Krum, Bulyan rides along;
                          # "plain"; "direction": a factor search follows, the first pass forms the attack direction only
                          # (searched "hidden" stays "plain": its direction comes from bm_attack_vector)
  search: Optional[str]   # None (fixed factor), "scalar_device", "scalar_host", "bulyan", "median", "colwise_eval", "generic"
  device_cursor: bool     # the exploration's cursor (for Bulyan, the ranking too) lives in device memory
  single_call: bool       # run() is one bm_step_worker call
  capabilities: frozenset  # the optional legs the backend declared
  accept: Optional[str] = None  # the acceptation ratio (attack.py:822): "count" = counted on the device from the rule's
                                # selection (krum, brute, aksel, cge), "average" = f_real / n on the host, None = the rule
                                # has no `influence` in the reference (math.nan)
  searches: bool = False        # a factor search runs each step: attack_evals, and somebody to attack (f_real >= 1)
  forms_vector: bool = True     # the first pass forms an attack vector — the direction alone when first_pass is
                                # "direction" — at scale 1 with attack_evals, else at the fixed factor; False: a chain or
                                # a kernel behind it forms the vector
  attack: Optional[_Attack] = None  # the row of _ATTACK
  pre: Optional[str] = None         # the pre-aggregation in front of the rule: "nnm", "bucketing" or None


# every scalar of the study row, from the packed vector of bm_step_worker or from the exchange of the sequence
# (gram: 4 x 4, row-major, of sampled avg, honest avg, defense, attack avg; ex0 / ex1: <s, newest past>, <s, C>)
# accept: Byzantine rows among those the rule averaged (an integer as a float; nan where nothing was counted)
_StudyRecord = collections.namedtuple("_StudyRecord",
                                      "s2 sd smax h2 hd hmax a2 ad amax d2 dmax l2 gram ex0 ex1 prev_s2 accept")
_ACCEPT_COUNTED = ("krum", "brute", "aksel", "cge")  # the rules whose `influence` counts over a selection


class _FirstPass(NamedTuple):
  """What AggregationStep._first_pass leaves for the stages behind it."""
  honests: list       # the rows the rule sees (worker placement: the momentum buffers)
  s_avg: Any          # sampled / honest averages
  h_avg: Any
  byz: Any            # the attack vector, or its direction before a search; None where the first pass forms none
  s_out3: Any         # device fp64[3] each: |avg|^2, sum of squared deviations, max |avg|
  h_out3: Any
  fused_defense: Any  # first pass "rule": the coordinate-wise rule's output
  fused_sq: Any       # first pass "sqdist": the n x n squared distances of the rule's stack


@dataclasses.dataclass
class _Pending:
  """What a run() leaves for floats(): the device scalars of the step, not yet fetched.  `packed` is set by the single
  call (the statistics vector of bm_step_worker; `prev`: the previous step's), the fields from `s` on by the sequence."""
  ks: int                     # sampled gradients of the step
  npast: int                  # 2 when the dots with the past were formed
  has_l2: bool
  accept_of: Optional[int]    # the denominator of the acceptation ratio (rows the rule averaged)
  packed: Any = None
  prev: Any = None
  s: Any = None               # out3 of the sampled and of the honest stack
  h: Any = None
  study: Any = None           # the slots of bm_study_stats
  prev_s2: Any = None         # device fp64[1]: |newest past average|^2
  accept: Any = None          # device fp64[1]: Byzantine rows among those the rule averaged
  floats: Optional[dict] = None  # the study row, once fetched ...
  epoch: int = -1                # ... under this graphs.replay_epoch(): a replay rewrites the tensors above in place


def _ieee_div(a, b):
  """a / b as the reference's tensor division has it (attack.py:854-859): a zero divisor gives NaN or an infinity."""
  try:
    return a / b
  except ZeroDivisionError:
    return math.nan if a != a or a == 0 else math.copysign(math.inf, a) * math.copysign(1.0, b)


class AggregationStep:
  def __init__(self, nb_workers, nb_decl_byz, nb_real_byz, gar="krum", gar_args=None, momentum=0.99,
               dampening=0.99, momentum_at="worker", attack="empire", attack_factor=1.1, nb_past=25,
               gradient_clip=None, aggregator=None, single_call=True, attack_evals=None, attack_negative=False,
               line_search="auto", attack_args=None, pre=None, pre_args=None):
    """aggregator: a sharded.ShardedAggregator (default: one over the default process group, or a
    single-rank one when torch.distributed is not initialised).
    single_call: with the HIP backend, worker-side momentum and a rule the C entry point knows
    (krum, bulyan, median, trmean, phocas, meamed), run() is ONE call into libbm_gar.so (bm_step_worker),
    collectives included; False keeps the kernel-by-kernel Python sequence (same kernels, same results).
    gar: a rule of the reference, or "geomed" (gar_args nu / iters / tol) / "cclip" (gar_args tau — required — / iters /
    tol): one distance pass, the iteration on scalars, one weighted sum (ShardedAggregator.geomed / .cclip); plain first
    pass, the generic factor search, no acceptation ratio, never the single call.  Centered clipping starts from the
    previous step's defense vector (`cclip_start`; the mean of the rows on the first step).  "caf" (gar_args power_iters)
    / "dnc" (gar_args power_iters / c), the spectral filters (ShardedAggregator.caf / .dnc), are handled exactly like
    geomed: f is nb_decl_byz.
    attack: "empire" / "little" (attacks/identical.py), or "anticge" (attacks/anticge.py: no factor — `attack_factor` is
    ignored, `attack_evals` must be None, and 1 <= nb_decl_byz <= honest workers); it runs as its own short chain behind
    the plain first pass (ShardedAggregator.anticge), with every momentum placement, clipping and rule.
    "nan" (attacks/nan.py: no factor either, `attack_evals` must be None), "hidden" (the reference's `bulyan` attack,
    attacks/identical.py:114-127 — "bulyan" names a rule here: factor, evaluations and `attack_negative` as for empire
    and little; attack_args={"target_idx": int | "all"}, default -1, a Python index into the whole vector) and
    "empire-strict" (attacks/empire.py: `attack_factor` is epsilon, a positive int, or `attack_evals` = E its
    `epsilon:-E`; it has no `negative`) are one streaming kernel behind the plain first pass
    (ShardedAggregator.attack_vector); never the single call.
    "minmax" / "minsum" (Shejwalkar & Houmansadr, NDSS 2021, not in the reference): the closed-form factor of
    include/bm_gar.h on the honest rows the rule is about to see — no factor: `attack_factor` is ignored as for anticge,
    `attack_evals` must be None; attack_args={"perturbation": "unit" | "std" | "sign"}, default "std"; at least two
    honest workers.  A chain behind the plain first pass like anticge (ShardedAggregator.minmax): every rule, momentum
    placement and clipping, never the single call.  `last_factor` is then the DEVICE tensor holding gamma (no read, no
    synchronisation), `last_byzantine.attack_info` the six numbers of bm_minmax_factor.
    attack_args: further arguments of the attack, for "hidden" and "minmax" / "minsum" alone.
    attack_evals: None = the fixed `attack_factor`; a positive integer E = the reference's `factor:-E` (its
    default is -16): the factor is searched each step with tools.line_maximize's exploration
    (identical.py:67-77), `attack_negative` being the attack's `negative` argument during the search.
    line_search: "auto" evaluates the search from scalars when the rule allows it (krum, brute, average) — on the
    device for krum / average (bm_attack_line_search_device) — and otherwise keeps the exploration's cursor in device
    memory (bm_search_device_next: median, trmean, phocas, meamed, aksel, cge ...): the step then has no synchronisation
    but `floats()`; Bulyan (its candidates are ranked on the host) and Brute keep the host's cursor.  "host": the same
    forms with scalars and cursor on the host (one synchronisation per evaluation).  "generic" always runs the rule on
    the device once per evaluation like the reference does, the cursor on the host.
    pre: a pre-aggregation in front of the rule, with every rule, momentum placement, clipping and attack: "nnm" — the
    defense is agg.nnm(stack, nb_decl_byz, rule=gar, **gar_args), every row replaced by the mean of its n - nb_decl_byz
    nearest (ShardedAggregator.nnm) — or "bucketing": the rule runs with f = nb_decl_byz on the ceil(n / s) means of random
    buckets of s rows (ShardedAggregator.bucketing).  pre_args: {"form": "rows" | "scalars"} for either ("scalars":
    pipelines.SCALAR_RULES alone, no mixed row written), and for bucketing {"s": bucket size within 1..n, required,
    "seed": default 0}.  The buckets are drawn ONCE per run(), before anything aggregates, from the step's own counter
    (0, 1, 2 ... by step; bm_bucket_masks_device where the backend has it: the counter then lives in device memory and
    a step replayed from a HIP graph draws the next permutation each time) — every evaluation of a factor search and the
    final defense read the same masks, `last_masks`.  With a pre-aggregation the step is never the single call, the first
    pass is "sqdist" where the pre-aggregated rule starts from the distances of the whole stack (nnm; bucketing with
    form "scalars" and a rule other than average: the matrix goes in as `local_sq`) under the conditions of Krum's, else
    "plain"; a factor search is the generic one (with the device cursor where line_search="auto" has it); there is no
    acceptation ratio (a selection over mixed rows is not one over workers: NaN).  Unknown names, foreign keys, a form
    the rule does not serve, pre_args without pre and a coordinate-wise rule left with fewer than 2 f + 1 rows raise
    ValueError here."""
    if gar not in _RULES:
      raise ValueError(f"unknown aggregation rule {gar!r}")
    if pre is None:
      if pre_args is not None:
        raise ValueError(f"pre_args without pre: got {pre_args!r}")
    else:
      if pre not in _PRE:
        raise ValueError(f"unknown pre-aggregation {pre!r} ({', '.join(_PRE)}, or None)")
      if gar not in pipelines.NNM_RULES:
        raise ValueError(f"pre={pre!r} serves {', '.join(sorted(pipelines.NNM_RULES))}, got rule {gar!r}")
      if pre_args is not None and (not isinstance(pre_args, dict) or set(pre_args) - set(_PRE[pre])):
        raise ValueError(f"pre_args of {pre} holds {_PRE[pre]} and nothing else, got {pre_args!r}")
      pre_args = dict(pre_args or {})
      pipelines.check_rule_form(f"pre={pre!r}", gar, pre_args.get("form", "rows"))
      n_out = nb_workers
      if pre == "bucketing":
        s = pre_args.get("s")
        if isinstance(s, bool) or not isinstance(s, int) or not 1 <= s <= nb_workers:
          raise ValueError(f"bucketing: pre_args must hold s, a bucket size within 1..{nb_workers}, got {s!r}")
        seed = pre_args.get("seed", 0)
        if isinstance(seed, bool) or not isinstance(seed, int):
          raise ValueError(f"bucketing: seed must be an integer, got {seed!r}")
        n_out = -(-nb_workers // s)
      if gar in _COLWISE and n_out < 2 * nb_decl_byz + 1:
        raise ValueError(f"{gar} behind pre={pre!r} runs on {n_out} rows and needs at least 2 f + 1 = "
                         f"{2 * nb_decl_byz + 1} of them")
    if gar in _CENTER:
      # geomed: nu / iters / tol; cclip: tau (required) / iters / tol — checked here, not at the first step
      from . import gars
      args, (radius, _, _) = dict(gar_args or {}), _CENTER[gar]
      if set(args) - set(_CENTER[gar]):
        raise ValueError(f"gar_args of {gar} holds {_CENTER[gar]} and nothing else, got {sorted(args)}")
      if gar == "cclip" and "tau" not in args:
        raise ValueError("cclip: gar_args must hold tau (the clipping radius)")
      gars.check_center_args(gar, args.get(radius, 1e-6), args.get("iters", 1), args.get("tol", 0.0))
    if gar in _SPECTRAL:
      # caf: power_iters; dnc: power_iters / c — checked here like geomed's, with the row count the rule will see
      from . import gars
      args, n = dict(gar_args or {}), nb_workers
      if set(args) - set(_SPECTRAL[gar]):
        raise ValueError(f"gar_args of {gar} holds {_SPECTRAL[gar]} and nothing else, got {sorted(args)}")
      c = args.get("c", 1.0)
      if isinstance(c, bool) or not isinstance(c, (int, float)) or not (0 <= c < float("inf")):
        raise ValueError(f"dnc: c must be a finite number >= 0, got {c!r}")
      count = nb_decl_byz if gar == "caf" else min(int(math.ceil(c * nb_decl_byz)), max(n - 1, 0))
      gars.check_spectral_args(gar, n, count, args.get("power_iters", 16))
    if momentum_at not in ("worker", "server", "update"):
      raise ValueError(f"momentum_at must be 'worker', 'server' or 'update', got {momentum_at!r}")
    if _attack_row(attack) is None:
      hint = "; the reference's `bulyan` attack is \"hidden\" here (bulyan names a rule)" if attack == "bulyan" else ""
      raise ValueError(f"unknown attack {attack!r} (empire, little, hidden: factor, use a negative one for negative:True; "
                       f"empire-strict: epsilon; anticge, nan: no factor){hint}")  # (and minmax, minsum: no factor)
    if attack_evals is not None and (not isinstance(attack_evals, int) or attack_evals < 1):
      raise ValueError(f"attack_evals must be a positive number of evaluations, got {attack_evals!r}")
    att = _attack_row(attack)
    if not att.factor and attack_evals is not None:
      raise ValueError(f"the {attack} attack has no factor to search: attack_evals must be None")
    if att.needs == "f_decl" and nb_real_byz >= 1 and not 1 <= nb_decl_byz <= nb_workers - nb_real_byz:
      raise ValueError(f"the anticge attack needs 1 <= nb_decl_byz <= {nb_workers - nb_real_byz} honest workers "
                       f"(attacks/anticge.py:67-68 indexes the sorted norms at h - f_decl), got {nb_decl_byz}")
    if att.needs == "pair" and nb_real_byz >= 1 and nb_workers - nb_real_byz < 2:
      raise ValueError(f"the {attack} attack needs at least 2 honest workers (a distance between two of them), got "
                       f"{nb_workers - nb_real_byz}")
    if "perturbation" in att.args:
      if attack_args is not None and (not isinstance(attack_args, dict) or set(attack_args) - att.args):
        raise ValueError(f"attack_args holds {{'perturbation': {' | '.join(map(repr, _PERTURBATIONS))}}} for the {attack} "
                         f"attack and nothing else, got {attack_args!r}")
      if (attack_args or {}).get("perturbation", "std") not in _PERTURBATIONS:
        raise ValueError(f"perturbation must be one of {', '.join(map(repr, _PERTURBATIONS))}, got "
                         f"{attack_args['perturbation']!r}")
    elif attack_args is not None and (not att.args or not isinstance(attack_args, dict) or set(attack_args) - att.args):
      raise ValueError(f"attack_args holds {{'target_idx': int | 'all'}} for the hidden attack and nothing else, "
                       f"got {attack_args!r} with attack {attack!r}")
    target_idx = (attack_args or {}).get("target_idx", -1)
    if "target_idx" in att.args and target_idx != "all" and (not isinstance(target_idx, int) or isinstance(target_idx, bool)):
      raise ValueError(f"target_idx must be an integer or \"all\" (attacks/identical.py:121-124), got {target_idx!r}")
    if attack_negative and not att.negative:
      raise ValueError("the empire-strict attack has no `negative` (attacks/empire.py:29): attack_negative must be False")
    if att.apply == "scale" and attack_evals is None and (not isinstance(attack_factor, int) or isinstance(attack_factor, bool)
                                                         or attack_factor < 1):
      raise ValueError(f"the empire-strict attack takes a positive integer epsilon as attack_factor "
                       f"(attacks/empire.py:82), got {attack_factor!r}")
    if line_search not in ("auto", "host", "generic"):
      raise ValueError(f"line_search must be 'auto', 'host' or 'generic', got {line_search!r}")
    if not 0 <= nb_past <= MAX_PAST:
      raise ValueError(f"nb_past must be within 0..{MAX_PAST}")
    if aggregator is None:
      from .sharded import ShardedAggregator
      aggregator = ShardedAggregator()
    self.agg = aggregator
    self.ops = aggregator.backend
    self.n = nb_workers
    self.f_decl = nb_decl_byz
    self.f_real = nb_real_byz
    self.h = nb_workers - nb_real_byz
    self.gar = gar
    self.gar_args = dict(gar_args or {})
    self.pre = pre
    self.pre_args = pre_args if pre is not None else {}
    self.pre_form = self.pre_args.get("form", "rows")
    self.last_masks = None        # bucketing: the masks of the last step (int64[MAX_ROWS] where the rows live)
    self._bucket_counter = None   # ... the draw's counter: a device int64[1] the kernel advances, or a Python integer
    self.mu = momentum
    self.damp = dampening
    self.omd = 1.0 - dampening
    self.momentum_at = momentum_at
    self.attack = attack
    self.target_idx = target_idx
    self.perturbation = (attack_args or {}).get("perturbation", "std") if "perturbation" in att.args else None
    self.factor = attack_factor
    self.clip = gradient_clip
    self.attack_evals = attack_evals
    self.attack_negative = bool(attack_negative)
    self.line_search = line_search
    self._factor_now = attack_factor  # last_factor / last_search (below): a number and a list, or what the device
    self._search_now = None           # search left in device memory (fetched when somebody asks)
    self.last_byzantine = None        # the Byzantine vector of the last step (aliased f_real times by the rule)
    self.buffers = None        # worker placement: one momentum buffer per honest worker (attack.py:676)
    self.server_momentum = None  # server / update placements: grad_momentum_server (attack.py:678)
    self.pasts = collections.deque(maxlen=max(nb_past, 1))  # past sampled averages, newest first (attack.py:868)
    self.nb_past = nb_past
    self._prev_s2 = None       # device fp64[1]: (this rank's part of) the squared norm of pasts[0]
    # C = sum_i mu^i * pasts[i]: the curvature term mu * sum_i mu^i <s, pasts[i]> (attack.py:863-865) is
    # mu * <s, C>, ONE dot product instead of nb_past of them; C is updated in place each step
    # (C <- s + mu * (C - mu^(P-1) * oldest) once the deque is full), 6 row passes instead of nb_past
    self._curv = None
    self._pending = None
    self._update = None
    self._prev_stats = None    # single-call form: the previous step's reduced statistics (slot 0 = ||avg_s||^2)
    # cclip: the vector the clipping starts from, the previous step's defense vector (None before the first step: the
    # mean of the rows).  Advanced by _defense alone — the evaluations of a factor search read it and leave it
    self.cclip_start = None
    # A step warmed up or recorded by graphs.GraphedCall (`_keeps_state`, from then on) keeps the server momentum and
    # cclip's start in buffers of its own, filled by a copy at the end of the step: the recorded kernels then read what
    # the replay before them wrote.  A step that is never graphed rebinds both, as the reference does, and copies nothing
    self._keeps_state = False
    self._kept = {}                   # "server" / "cclip" -> the buffer
    self._search_dev = None           # the device search's result tensor once last_factor / last_search were fetched ...
    self._search_epoch = -1           # ... under this graphs.replay_epoch()
    self.plan = self._make_plan(single_call)
    self.single_call = self.plan.single_call
    self._refusal = self.graph_refusal()

  def _make_plan(self, single_call):
    """Every decision that depends on the constructor's arguments and the backend alone.  A backend names its optional
    legs in a `capabilities` set (sharded.HipBackend); one that declares none gets the plain first pass, the host's
    cursor and the forms of the search that need the common legs only."""
    caps = frozenset(getattr(self.ops, "capabilities", ()))
    gar, k, fixed = self.gar, self.f_real, self.attack_evals is None
    only_m = not (set(self.gar_args) - {"m"})
    analytic = self.line_search in ("auto", "host")
    # the first pass: momentum_stats* (worker placement) and stack_stats* (update placement) make the same choice
    stem = {"worker": "momentum_stats_", "update": "stack_stats_"}.get(self.momentum_at)
    att = _attack_row(self.attack)
    behind = att.formed != "first_pass"
    if not fixed and att.direction == "first_pass":  # (empire-strict: the empire direction, -avg)
      first_pass = "direction"
    elif behind:  # a chain or a kernel of its own behind the plain first pass, which forms no attack vector
      first_pass = "plain"
    elif stem and k >= 1 and not self.gar_args and gar in _COLWISE and stem + "colwise" in caps:
      first_pass = "rule"
    elif stem and k >= 1 and only_m and gar in _DISTANCE and stem + "sqdist" in caps:
      first_pass = "sqdist"
    else:
      first_pass = "plain"
    # the factor search; Brute keeps the host's cursor (its checked call synchronises per evaluation anyway), Bulyan
    # moves cursor and ranking to the device together
    small = self.h + 2 <= 64  # the (h+2) x (h+2) matrix of the scalar forms fits the kernels' 64 rows
    device_cursor = self.line_search == "auto" and "device_search" in caps and gar != "brute"
    if fixed:
      search, device_cursor = None, False
    elif analytic and gar in linesearch.ANALYTIC_RULES and small and only_m:
      # (the device form keeps its cursor inside the kernel: the abscissa 1 + x of empire-strict needs the host's)
      device_cursor = self.line_search == "auto" and gar in getattr(self.ops, "device_search_rules", ()) and not att.shift
      search = "scalar_device" if device_cursor else "scalar_host"
    elif analytic and gar == "bulyan" and k >= 1 and small and only_m:
      search, device_cursor = "bulyan", device_cursor and "attack_ranking_device" in caps
    elif analytic and gar == "median" and k >= 1:
      search = "median"
    elif analytic and gar in _COLWISE and k >= 1 and not self.gar_args and "colwise_eval" in caps:
      search = "colwise_eval"
    else:
      search = "generic"
    single = bool(single_call and fixed and not behind and self.momentum_at == "worker" and "step_worker" in caps
                  and gar in _DISTANCE + _COLWISE and only_m and (not self.agg.collective or self.agg.native is not None))
    accept = "count" if gar in _ACCEPT_COUNTED else ("average" if gar == "average" else None)
    if self.pre is not None:
      # a pre-aggregation stands in front of the rule: the rule never rides in the first pass, but the distance pass does
      # wherever the pre-aggregated rule starts from the distances of the whole stack, whatever the rule and its gar_args
      # (under the conditions of "sqdist" above: the chain of conditions before it is the same)
      from_sq = self.pre == "nnm" or (self.pre_form == "scalars" and gar != "average")
      if first_pass != "direction" and not behind:  # (the attack is formed in the first pass, at a fixed factor)
        first_pass = "sqdist" if stem and k >= 1 and from_sq and stem + "sqdist" in caps else "plain"
      if not fixed:
        search = "generic"
        device_cursor = self.line_search == "auto" and "device_search" in caps and gar != "brute"
      single, accept = False, None
    return StepPlan(only_m, analytic, first_pass, search, device_cursor, single, caps, accept,
                    searches=not fixed and k > 0, forms_vector=not behind or first_pass == "direction", attack=att,
                    pre=self.pre)

  # ------------------------------------------------------------------------ #

  @property
  def last_factor(self):
    """The factor of the last step (the searched one with attack_evals).  After a device search this is the read that
    synchronises; a step that never looks costs nothing."""
    self._unsettle_after_replay()
    if isinstance(self._factor_now, torch.Tensor) and isinstance(self._search_now, torch.Tensor):
      self._settle_search()
    return self._factor_now  # (minmax / minsum: the device tensor the chain left, handed out as it is)

  @last_factor.setter
  def last_factor(self, value):
    self._factor_now, self._search_dev = value, None

  @property
  def last_search(self):
    """[(x, objective)] of the last search, in evaluation order."""
    self._unsettle_after_replay()
    if isinstance(self._search_now, torch.Tensor):
      self._settle_search()
    return self._search_now

  @last_search.setter
  def last_search(self, value):
    self._search_now, self._search_dev = value, None

  def _settle_search(self):
    found = self._search_now
    values = self._fetch(found).tolist()
    self._factor_now = values[0]
    self._search_now = [(values[1 + 2 * i], values[2 + 2 * i]) for i in range((len(values) - 1) // 2)]
    self._search_dev, self._search_epoch = found, graphs.replay_epoch()

  def _unsettle_after_replay(self):
    """A replay of a recorded step runs the search again and leaves its result in the tensor the recording left: what
    was fetched from it before describes an earlier step."""
    if self._search_dev is not None and self._search_epoch != graphs.replay_epoch():
      self._factor_now = self._search_now = self._search_dev
      self._search_dev = None

  @staticmethod
  def _new_rows(count, like, zero=False):
    """`count` vectors shaped like `like`, one allocation each.  (Rows of one allocation at a skewed stride,
    layout.alloc_rows, help the column kernels; for the write-heavy first pass of the step they measured 0.3-5 %
    slower than separate allocations in every A/B, profiles/r03_h / r03_i, so the step keeps separate ones.)"""
    return [torch.zeros_like(like) if zero else torch.empty_like(like) for _ in range(count)]

  def _draw_masks(self, like):
    """bucketing: the masks of this run(), drawn before anything aggregates — from the device counter where the backend
    has the leg and the rows are on a GPU (the kernel advances it), else from a host counter advanced here."""
    s, seed, legs = self.pre_args["s"], self.pre_args.get("seed", 0), self.agg.legs
    if "bucket_masks" in self.plan.capabilities and like.is_cuda:
      if self._bucket_counter is None:
        self._bucket_counter = torch.zeros(1, dtype=torch.int64, device=like.device)
      self.last_masks = legs.bucket_masks(self.n, s, seed, self._bucket_counter, like)
    else:
      count = self._bucket_counter or 0
      self.last_masks = legs.bucket_masks(self.n, s, seed, count, like)
      self._bucket_counter = count + 1

  def _aggregate_pre(self, gradients, local_sq):
    """The rule behind the pre-aggregation (ShardedAggregator.nnm / .bucketing); local_sq: the squared distances of
    `gradients` on this rank where the first pass formed them."""
    agg, gar, args = self.agg, self.gar, dict(self.gar_args)
    if gar == "brute":
      args["check"] = True  # (as in _aggregate)
    if gar == "cclip":
      args["start"] = self.cclip_start
    if self.pre == "nnm":
      return agg.nnm(gradients, self.f_decl, rule=gar, form=self.pre_form, local_sq=local_sq, **args)
    if pipelines.NNM_RULES[gar]:
      args["f"] = self.f_decl
    return agg.bucketing(gradients, self.pre_args["s"], gar, masks=self.last_masks, form=self.pre_form, local_sq=local_sq,
                         **args)

  def _aggregate(self, gradients, local_sq=None):
    agg, f = self.agg, self.f_decl
    if self.pre is not None:
      return self._aggregate_pre(gradients, local_sq)
    if self.gar == "median":
      return agg.median(gradients)
    if self.gar == "average":
      return agg.average(gradients)
    if self.gar == "brute":
      # checked HERE, before anybody can apply the defense vector (one 4-byte synchronisation per step for this rule
      # alone): no admissible subset raises like brute.py:68, a device search that ran out of its node budget is
      # repeated on the host
      return agg.brute(gradients, f, check=True, **self.gar_args)
    if self.gar == "cclip":
      return agg.cclip(gradients, f, start=self.cclip_start, **self.gar_args)
    return getattr(agg, self.gar)(gradients, f, **self.gar_args)

  def _fetch(self, matrix):
    """A small device matrix on the host, through a pinned buffer this step keeps (one asynchronous copy + one stream
    synchronisation, no allocation per search).  Measured next to `.cpu()` into pageable memory: 0.019 against 0.017 ms
    for the 15 KB of a C3 search (bench.py, `attack_search_c3_krum.legs`) — the copy is not where a slow search loses
    its time (that was a stalled host, profiles/r06_search_each.txt); the buffer only keeps the path free of the
    runtime's staging allocations."""
    if not matrix.is_cuda:
      return matrix.contiguous()
    key = (tuple(matrix.shape), matrix.dtype)
    if getattr(self, "_pinned", None) is None or self._pinned[0] != key:
      self._pinned = (key, torch.empty(matrix.shape, dtype=matrix.dtype, pin_memory=True))
    host = self._pinned[1]
    host.copy_(matrix, non_blocking=True)
    torch.cuda.current_stream(matrix.device).synchronize()
    return host

  def _search_factor(self, honests, h_avg, direction):
    """attacks/identical.py:67-77: the factor maximising |GAR(honests + [avg + t*dir]*f_real) - avg|^2 under
    the evaluation budget.  Like the reference, `negative` flips the sign of the candidates DURING the
    search only; the factor returned (and then applied) is the positive abscissa the search settled on.
    Returns a number, or the device tensor whose [0] is the factor; sets last_search.
    empire-strict (attacks/empire.py:51-59): `direction` is -avg and the candidate avg * (-x) is avg + (1 + x) * (-avg),
    so every form is evaluated at the abscissa 1 + x of what the cursor proposes; the result is x, epsilon."""
    plan = self.plan
    if plan.search in ("scalar_device", "scalar_host"):
      return self._search_scalar(honests, h_avg, direction)
    on_device = plan.device_cursor and h_avg.is_cuda
    form = {"bulyan": self._bulyan_objective, "median": self._median_objective,
            "colwise_eval": self._colwise_objective, "generic": self._generic_objective}[plan.search]
    return self._drive(form(honests, h_avg, direction, on_device), h_avg, on_device, shift=plan.attack.shift)

  def _drive(self, evaluate, h_avg, on_device, shift=0.0):
    """Run `evaluate(t) -> device fp64[1]` under the exploration of tools.line_maximize, its cursor in device memory
    or on the host.  shift: added to every proposal before it is evaluated (a number on the host, one small device
    addition with a device cursor: no synchronisation); the trace and the result keep the cursor's own abscissae."""
    def objective(t):
      sq = evaluate(t + shift if shift else t)
      self.agg.all_reduce_sum(sq)
      return sq

    if on_device:
      # every evaluation reads its factor in device memory and leaves its objective there: the host queues the whole
      # search and waits for none of it; last_factor / last_search fetch the result when asked
      cursor = self.ops.device_search(h_avg.device, self.attack_evals, self.attack_negative)
      y = None
      for _ in range(self.attack_evals):
        y = objective(cursor.next(y))
      found = self.last_search = cursor.finish(y)  # (not read back through the property: that would fetch it)
      return found
    factor, self.last_search = linesearch.line_maximize(
      lambda x: objective(-x if self.attack_negative else x).item(), evals=self.attack_evals)
    return factor

  def _unit_sqdist(self, honests, h_avg, direction):
    """The (h+2) x (h+2) squared distances among honests + [avg, avg + dir]: every distance of a candidate stack is a
    function of these inner products, so ONE distance pass serves a whole search."""
    unit = torch.empty_like(h_avg)
    self.ops.multi_fma3([unit], [h_avg], [direction], 1.0, 1.0)   # avg + dir: the candidate of factor 1
    return self.agg.global_sqdist(list(honests) + [h_avg, unit])

  def _search_scalar(self, honests, h_avg, direction):
    """krum / brute / average: every evaluation is a function of the scalars of one distance pass (linesearch.py)."""
    sq = self._unit_sqdist(honests, h_avg, direction)
    args = dict(evals=self.attack_evals, negative=self.attack_negative, m=self.gar_args.get("m"))
    if self.plan.search == "scalar_device":
      # evaluated where the distances are: no copy, no synchronisation; the factor stays on the device (a tensor:
      # multi_fma3 reads it there)
      found = self.last_search = self.ops.attack_search_device(sq, self.h, self.f_real, self.f_decl, self.gar, **args)
      return found
    ext = self._fetch(sq)  # the search's only synchronisation
    shift = self.plan.attack.shift
    if shift:  # the exploration over the scalar objective at 1 + x
      factor, self.last_search = linesearch.line_maximize(
        lambda x: linesearch.attack_objective(ext, self.h, self.f_real, self.f_decl, self.gar, shift + x, args["m"])[0],
        evals=self.attack_evals)
      return factor
    factor, self.last_search = linesearch.attack_line_search(ext, self.h, self.f_real, self.f_decl, self.gar, **args)
    return factor

  def _written_objective(self, rule, h_avg, direction):
    """evaluate(t) that writes the candidate, runs `rule(cand, t)` on it and measures the output against the average."""
    ops = self.ops

    def evaluate(t):
      cand = torch.empty_like(h_avg)
      ops.multi_fma3([cand], [h_avg], [direction], 1.0, t)
      out = rule(cand, t)
      # aggregated.sub_(grad_avg); dot with itself: one pass over the two vectors where the backend has it
      if "sqdist2" in self.plan.capabilities:
        return ops.sqdist2(out, h_avg)
      return ops.pairwise_sqdist([out, h_avg])[0, 1].reshape(1)
    return evaluate

  def _generic_objective(self, honests, h_avg, direction, on_device=False):
    """The rule itself on the n rows, once per evaluation, like the reference."""
    return self._written_objective(lambda cand, t: self._aggregate(list(honests) + [cand] * self.f_real), h_avg, direction)

  def _colwise_objective(self, honests, h_avg, direction, on_device=False):
    """trmean / phocas / meamed: candidate, rule and objective in ONE pass over the honest rows, nothing written
    (bm_colwise_eval: h + 2 row passes instead of h + 5 read and 2 written); the same value at every column."""
    ops, k = self.ops, self.f_real
    if not ops.colwise_eval_supported(self.gar, self.h + k):
      return self._generic_objective(honests, h_avg, direction)
    return lambda t: ops.colwise_eval(self.gar, honests, k, self.f_decl, h_avg, direction, t)

  def _median_objective(self, honests, h_avg, direction, on_device=False):
    """The lower median of the h honest values and k copies of ONE value b is monotone in b, equals b while b lies
    between two order statistics of the honest values and stays at them outside: median(honests + [b] * k) = middle
    of (b, lo, hi) per coordinate, with lo / hi the medians of the honest values and k copies of -inf / +inf.  Two
    passes over the honest rows for the whole search, then every candidate is the median of THREE rows (4 row passes
    instead of n + 1): the same value of the rule at every coordinate — it returns one of its inputs, no arithmetic —
    hence the same objective, bit for bit, as evaluating the rule on the n rows."""
    ops, agg, h, k = self.ops, self.agg, self.h, self.f_real
    n, caps = h + k, self.plan.capabilities
    if "order_pair" in caps and ops.order_pair_supported(h):
      lo, hi = ops.order_pair(honests, (n - 1) // 2 - k, (n - 1) // 2)   # both in one pass over the honest rows
    else:
      lo = agg.median(list(honests) + [torch.full_like(h_avg, -math.inf)] * k)
      hi = agg.median(list(honests) + [torch.full_like(h_avg, math.inf)] * k)
    if "colwise_eval" in caps:
      # evaluate-only instances (bm_colwise_eval), nothing written: the middle of (lo, hi, candidate), else the median
      # of the n rows themselves where the library has that instance
      whole = not self.gar_args and ops.colwise_eval_supported("median", n)
      if ops.colwise_eval_supported("median", 3):
        return lambda t: ops.colwise_eval("median", [lo, hi], 1, 0, h_avg, direction, t)
      if whole:
        return lambda t: ops.colwise_eval("median", honests, k, self.f_decl, h_avg, direction, t)
    return self._written_objective(lambda cand, t: agg.median([cand, lo, hi]), h_avg, direction)

  def _bulyan_objective(self, honests, h_avg, direction, on_device):
    """Bulyan's second pass needs the vectors, its ranking does not: every candidate is ranked from the scalars of ONE
    distance pass and costs pass 2 alone (m + 1 row passes instead of n + m + 1) — ranked where the matrix is, from
    the factor the device cursor left there (bm_attack_ranking_device: no copy, no synchronisation), or on the host
    from the number the host's cursor proposed (one copy of the matrix per search)."""
    ops, h, k, f = self.ops, self.h, self.f_real, self.f_decl
    n = h + k
    m = self.gar_args.get("m") or n - f - 2
    sq_dev = self._unit_sqdist(honests, h_avg, direction)
    ext = None if on_device else self._fetch(sq_dev)

    def ranking(t):
      if on_device:
        return ops.attack_ranking_device(sq_dev, h, k, f, "bulyan", t, m)
      order = linesearch.attack_ranking(ext, h, k, f, "bulyan", t, m)
      return ops.index_tensor(order + [0] * (64 - n), h_avg)

    if "bulyan_pass2_eval" in self.plan.capabilities and ops.bulyan_pass2_eval_supported(n, f, m, h_avg.shape[0]):
      # pass 2 has an evaluate-only form for the shapes of the reference's experiments: the candidate in registers,
      # the objective accumulated in the same kernel, nothing written (bm_bulyan_pass2_eval)
      return lambda t: ops.bulyan_pass2_eval(honests, k, ranking(t), f, m, h_avg, direction, t)
    return self._written_objective(lambda cand, t: ops.bulyan_pass2(list(honests) + [cand] * k, ranking(t), f, m),
                                   h_avg, direction)

  def nesterov_lookahead(self, params, lr, worker=None):
    """params <- params - mu*lr*momentum in place (attack.py:760-767): the parameter shift before
    the gradients of a Nesterov step are computed.  worker: index of the worker momentum buffer
    (worker placement), else the server momentum."""
    # (before the first step every momentum is zero, attack.py:676-678: the shift is then the identity)
    mom = (self.buffers[worker] if self.buffers is not None else None) if worker is not None else self.server_momentum
    if mom is not None:
      self.ops.multi_fma3([params], [params], [mom], 1.0, -(self.mu * lr))
    return params

  def graph_refusal(self):
    """Why a replay of run() from a HIP graph (graphs.GraphedCall) would not be the step, or None: a replay runs the
    recorded kernels and none of this file's Python.  run() raises graphs.GraphRefusal with it, before it launches
    anything, while a GraphedCall warms the step up or a stream capture is in progress."""
    plan = self.plan
    if self.nb_past > 0:
      return ("nb_past > 0: the deque of past sampled averages, the curvature mode and the previous step's norm advance "
              "on the host, a recording would freeze one step's (use nb_past=0)")
    if plan.searches and not plan.device_cursor:
      return (f"the factor search's cursor is on the host (search {plan.search!r}, line_search={self.line_search!r}, "
              f"rule {self.gar}, attack {self.attack}): it reads the device at every evaluation, or once per search")
    if self.pre == "bucketing" and "bucket_masks" not in plan.capabilities:
      return "bucketing on a backend without the device counter: the draw's counter is a Python integer"
    return None

  def _carried(self, key, vector):
    """`vector` where the next step reads it: the vector itself, or — in a step a GraphedCall has warmed up or recorded
    — this step's own buffer for `key` after one d-sized copy, an address the recorded kernels read and write alike."""
    if not self._keeps_state:
      return vector
    own = self._kept.get(key)
    if own is None or own.shape != vector.shape or own.device != vector.device:
      own = self._kept[key] = torch.empty_like(vector)
    own.copy_(vector)
    return own

  def run(self, grad_sampleds, params=None, origin=None):
    """grad_sampleds: list of >= h flat fp32 GPU tensors (this rank's slice of the step's sampled
    gradients).  params/origin: optional flat parameter vectors for `l2_origin` (attack.py:830).
    Returns the aggregated gradient (slice); statistics stay on the device until floats()."""
    sampled = list(grad_sampleds)
    if getattr(grad_sampleds, "d_total", None) is not None:  # sharded.Shards: keep the stated total length
      from .sharded import Shards
      sampled = Shards(sampled, d_total=grad_sampleds.d_total)
    if len(sampled) < self.h:
      raise ValueError(f"{len(sampled)} sampled gradients for {self.h} honest workers")
    warming = graphs.preparing()
    if self._refusal is not None and (warming or graphs.capturing()):
      raise graphs.GraphRefusal(f"this step cannot be replayed from a HIP graph: {self._refusal}")
    if warming:
      self._keeps_state = True
    if self.single_call:
      return self._run_single_call(sampled, len(sampled), self.omd, params, origin)
    if self.pre == "bucketing":
      self._draw_masks(sampled[0])
    factors = self._clip_factors(sampled)                   # 0.
    first = self._first_pass(sampled, factors)              # 1. and what it does of 2.
    byz = self._byzantine(first, sampled)                   # 2.
    defense = self._defense(first, [byz] * self.f_real)     # 3.
    # (attack.py:822) the Byzantine rows among those the rule has just averaged, counted where its selection is
    accept = self._accept_count() if self.plan.accept == "count" else (None, None)
    self._update_momentum(defense)                          # 4.
    self._study(first, defense, byz, params, origin, len(sampled), accept)  # 5.
    return defense

  def _clip_factors(self, sampled):
    """Step 0 (attack.py:776-779,791-794): the clipping factors as device scalars, None without clipping; the all-reduce
    makes the norms global under sharding."""
    if self.clip is None:
      return None
    sq = self.ops.row_sqnorms(sampled)
    self.agg.all_reduce_sum(sq)
    return self.ops.clip_factors_from_sq(sq, len(sampled), self.clip)

  def _first_pass(self, sampled, factors):
    """Step 1 (attack.py:800-810) and what the first pass does of step 2: momentum by placement, the statistics of the
    sampled and the honest stacks, and — in the form the plan chose — the attack vector or its direction
    (attacks/identical.py:63-86,129-141), the coordinate-wise rule ("rule") or the rule's distance pass ("sqdist")."""
    plan = self.plan
    # None: the first pass forms no attack vector; with a search, the direction at factor 1
    scale = (1.0 if plan.search is not None else self.factor) if plan.forms_vector else None
    if self.momentum_at == "worker":
      return self._first_pass_worker(sampled, factors, scale)
    return self._first_pass_stack(sampled, factors, scale)

  def _first_pass_worker(self, sampled, factors, scale):
    """buf_i <- mu*buf_i + (1-damp)*g_i (attack.py:800-804), clipping included, in ONE kernel with the statistics."""
    ops, plan, att = self.ops, self.plan, self.plan.attack
    fused_defense, fused_sq = None, None
    if self.buffers is None:
      self.buffers = self._new_rows(self.h, sampled[0], zero=True)
    if plan.first_pass == "rule":  # first pass + coordinate-wise rule in one call (one kernel for median / trmean at h = 20)
      s_avg, h_avg, byz, fused_defense, out6 = ops.momentum_stats_colwise(
        sampled, self.buffers, self.mu, self.omd, factors, self.factor, att.first_pass, self.gar, self.f_decl, self.f_real)
    elif plan.first_pass == "sqdist":
      # first pass + the distance pass of the rule in one call (one kernel at h = 20 for long gradients)
      s_avg, h_avg, byz, fused_sq, out6 = ops.momentum_stats_sqdist(
        sampled, self.buffers, self.mu, self.omd, factors, self.factor, att.first_pass, self.f_real,
        d_total=self.agg._total_of(sampled))
    else:  # ("direction": the attack direction alone; the Byzantine vector follows the factor search)
      s_avg, h_avg, byz, out6 = ops.momentum_stats(sampled, self.buffers, self.mu, self.omd, factors, scale,
                                                   att.first_pass, direction=plan.first_pass == "direction")
    return _FirstPass(self.buffers, s_avg, h_avg, byz, out6[:3], out6[3:], fused_defense, fused_sq)

  def _first_pass_stack(self, sampled, factors, scale):
    """server: hon_i = (1-damp)*g_i + mu*M (attack.py:805-808); update / none: hon_i = g_i (attack.py:809-810)."""
    ops, att, h, ks = self.ops, self.plan.attack, self.h, len(sampled)
    first_pass, fused_defense, fused_sq = self.plan.first_pass, None, None
    if factors is not None:
      ops.multi_scale(sampled, factors)  # in place, like the reference's grad.mul_
    if self.momentum_at == "server":
      # (first step: grad_momentum_server is zero, attack.py:678: hon_i = (1-damp)*g_i)
      mom = self.server_momentum if self.server_momentum is not None else torch.zeros_like(sampled[0])
      honests = self._new_rows(h, sampled[0])
      ops.multi_fma3(honests, sampled[:h], [mom] * h, self.omd, self.mu)
    else:
      honests = sampled[:h]
    # momentum at the update with every sampled gradient honest: the rule, or its distance pass, is fed from the pass
    # that forms the statistics and the Byzantine vector (one pass over the rows at h = 20 / 14)
    if ks != h and first_pass in ("rule", "sqdist"):
      first_pass = "plain"
    if first_pass == "rule":
      h_avg, byz, fused_defense, o6 = ops.stack_stats_colwise(honests, self.factor, att.first_pass, self.gar, self.f_decl,
                                                              self.f_real)
      h_out3 = o6[3:]
    elif first_pass == "sqdist":
      h_avg, byz, fused_sq, o6 = ops.stack_stats_sqdist(honests, self.factor, att.first_pass, self.f_real,
                                                        d_total=self.agg._total_of(sampled))
      h_out3 = o6[3:]
    else:
      h_avg, h_out3, *byz = ops.stack_stats(honests, scale=scale, attack=att.first_pass,
                                            direction=first_pass == "direction")
      byz = byz[0] if byz else None
    if self.momentum_at == "update" and ks == h:
      # the honest stack IS the sampled stack (attack.py:809-810): one pass gives both sets of statistics
      s_avg, s_out3 = h_avg, h_out3
    else:
      s_avg, s_out3 = ops.stack_stats(sampled)
    return _FirstPass(honests, s_avg, h_avg, byz, s_out3, h_out3, fused_defense, fused_sq)

  def _byzantine(self, first, sampled):
    """The rest of step 2: the chain or the kernel behind the plain first pass, the factor search and the found factor
    applied.  Returns the Byzantine vector (the rule sees f_real references to it); sets last_byzantine, and with a
    search last_factor / last_search."""
    agg, plan, att = self.agg, self.plan, self.plan.attack
    honests, h_avg, byz = first.honests, first.h_avg, first.byz
    searched = plan.search is not None
    if att.formed == "chain" and self.f_real > 0:
      # on the honest gradients the rule is about to see (the updated buffers under worker placement).  anticge
      # (attacks/anticge.py:49-78): row norms, ranking, sum and scaling on the device, two small collectives under
      # sharding; minmax / minsum: one pass for the scalars, the distance pass, the closed form, one collective
      byz = _CHAIN[att.first_pass](self, honests)[0]
      if hasattr(byz, "attack_factor"):
        self.last_factor, self.last_search = byz.attack_factor, None
    if att.formed == "kernel" and self.f_real > 0:
      # one streaming kernel on the honest average (bm_attack_vector); with a search, `hidden` takes its 0 / 1 direction
      # from the same kernel at factor 1 and empire-strict waits for its epsilon
      if not att.factor:  # attacks/nan.py:36-40
        byz = agg.attack_vector(att.kind, h_avg)
      elif att.direction == "kernel":  # attacks/identical.py:114-127
        where = dict(target_idx=self.target_idx, d_total=agg._total_of(sampled)) if self.target_idx != "all" else {}
        made = agg.attack_vector("shift_all" if self.target_idx == "all" else att.kind, h_avg,
                                 1.0 if searched else self.factor, want_direction=searched, **where)
        byz = made[1] if searched else made
      elif not searched:  # attacks/empire.py:61-62 at the fixed epsilon
        byz = agg.attack_vector(att.kind, h_avg, -self.factor)
    if plan.searches:
      direction = byz
      factor = self._search_factor(honests, h_avg, direction)  # a number, or the device search's tensor ([0]: the factor)
      self.last_factor = factor
      if att.apply == "scale":  # byz_grad.mul_(-epsilon) with the epsilon found (empire.py:61-62)
        byz = agg.attack_vector("scale", h_avg, -factor[:1] if isinstance(factor, torch.Tensor) else -factor)
      else:
        byz = torch.empty_like(h_avg)  # grad_att.mul_(factor); byz_grad = grad_avg.add_(grad_att)  (identical.py:82-84)
        self.ops.multi_fma3([byz], [h_avg], [direction], 1.0, factor)
    self.last_byzantine = byz if self.f_real > 0 else None  # the Byzantine vector of this step (callers, tests)
    return byz

  def _defense(self, first, attacks):
    """Step 3 (attack.py:821): what the first pass fused, the rule from the distances it left, or the rule itself."""
    if first.fused_defense is not None:
      return first.fused_defense
    if first.fused_sq is not None and self.pre is None:
      return self.agg.rule_from_sq(self.gar, first.honests + attacks, first.fused_sq, self.f_decl, self.gar_args.get("m"))
    defense = self._aggregate(first.honests + attacks, first.fused_sq)
    if self.gar == "cclip":
      # the next step clips around this one's aggregate (never written again: no clone; a graphed step keeps a copy)
      self.cclip_start = self._carried("cclip", defense)
    return defense

  def _update_momentum(self, defense):
    """Step 4 (attack.py:832-839): what update_gradient() hands out."""
    if self.momentum_at == "server":
      self.server_momentum = self._carried("server", defense)  # no clone, as attack.py:835 (a graphed step: a copy)
      self._update = defense
    elif self.momentum_at == "update":
      # M <- mu * M + (1 - damp) * defense (attack.py:836-838) rides along with the study block, which reads the defense
      # vector anyway (bm_study_stats_update): no pass of its own
      if self.server_momentum is None:
        self.server_momentum = torch.zeros_like(defense)
      self._update = self.server_momentum
    else:
      self._update = defense

  def _study(self, first, defense, byz, params, origin, ks, accept):
    """Step 5 (attack.py:828-868): the remaining statistics in ONE pass over the vectors (bm_study_stats) — attack stack,
    defense vector, the Gram matrix behind the cosines, the dots with the past, l2 from the origin, and the curvature
    combination for the next step — left with the first pass's as the pending record of floats().
    grad_pasts.appendleft(PastGrad(sampled_grad_avg, sampled_norm_avg)) (attack.py:868) happens every step, whether or
    not the scalars are fetched."""
    s_avg = first.s_avg
    count = len(self.pasts) if self.nb_past > 0 else 0
    mode = 0
    if self.nb_past > 0:
      if self._curv is None:
        self._curv = torch.empty_like(s_avg)  # written by the first step (C <- s)
      mode = 1 if count == 0 else (3 if count == self.nb_past else 2)  # 3: the oldest entry leaves the deque
    has_l2 = params is not None and origin is not None
    study = self.ops.study_stats(s_avg, first.h_avg, defense, byz if self.f_real > 0 else None, self.f_real,
                                 past_newest=self.pasts[0] if count > 0 else None, curv=self._curv,
                                 past_oldest=self.pasts[-1] if mode == 3 else None, curv_mode=mode, mu=self.mu,
                                 oldest_weight=-(self.mu ** (self.nb_past - 1)) if self.nb_past > 0 else 0.0,
                                 params=params if has_l2 else None, origin=origin if has_l2 else None,
                                 **(dict(update_momentum=self.server_momentum, update_mu=self.mu, update_omd=self.omd)
                                    if self.momentum_at == "update" else {}))
    self._pending = _Pending(ks=ks, npast=2 if count > 0 else 0, has_l2=has_l2, accept_of=accept[1], s=first.s_out3,
                             h=first.h_out3, study=study, prev_s2=self._prev_s2 if count > 0 else None, accept=accept[0])
    if self.nb_past > 0:
      self.pasts.appendleft(s_avg)
      self._prev_s2 = first.s_out3[:1]

  def _accept_count(self):
    """(device fp64[1], denominator): how many of the rows the aggregator's latest rule averaged are Byzantine copies —
    index >= h, gradients being honests + [byz] * f_real — and how many it averaged.  One wavefront where the backend
    has the kernel, else plain torch on the index tensor, on its device; no synchronisation either way."""
    order, count = self.agg.last_selection
    if "accept_count" in self.plan.capabilities:
      return self.ops.accept_count(order, count, self.h), count
    return (order[:count] >= self.h).sum().to(torch.float64).reshape(1), count

  def _run_single_call(self, sampled, ks, omd, params, origin):
    h = self.h
    if self.buffers is None:
      self.buffers = self._new_rows(h, sampled[0], zero=True)
    count = len(self.pasts) if self.nb_past > 0 else 0
    if self.nb_past > 0 and self._curv is None:
      self._curv = torch.empty_like(sampled[0])  # written by the first step (C <- s)
    full = count == self.nb_past and count > 0
    defense, s_avg, h_avg, byz, stats = self.ops.step_worker(
      self.agg.native, sampled, self.buffers, self.n, self.f_decl, self.f_real, self.gar, self.gar_args.get("m"),
      self.mu, omd, self.clip, self.attack, self.factor, self.nb_past, count,
      self.pasts[0] if count > 0 else None, self._curv, self.pasts[-1] if full else None, params, origin,
      d_total=self.agg._total_of(sampled))
    self._update = defense
    self.last_byzantine = byz
    self._pending = _Pending(ks=ks, npast=2 if count > 0 else 0, has_l2=params is not None and origin is not None,
                             # (krum: slot STEP_ACCEPT of the packed vector counts over the m rows it averaged)
                             accept_of=self.gar_args.get("m") or self.n - self.f_decl - 2,
                             packed=stats, prev=self._prev_stats if count > 0 else None)
    if self.nb_past > 0:
      self.pasts.appendleft(s_avg)
      self._prev_stats = stats
    return defense

  def update_gradient(self):
    """What attack.py:832-839 passes to model.update(): the defense gradient (worker / server
    placements) or the updated server momentum (update placement)."""
    return self._update

  # ------------------------------------------------------------------------ #

  def _exchange(self, pend):
    """One packed exchange of every scalar of the sequence (sums and maxima, all ranks), as a _StudyRecord."""
    s3, h3, st, prev = pend.s, pend.h, pend.study, pend.prev_s2
    last = [prev] if prev is not None else []
    acc = [pend.accept] if pend.accept is not None else []  # (every rank holds the same count: a maximum)
    if not self.agg.collective:
      # ONE copy to the host, ONE synchronisation: the whole tensors travel — three or four of them in one concatenation
      # — to be taken apart on the host (two `tolist()` were two copies with a host round trip between them: ~30 us of a
      # 0.95 ms step, profiles/r05_c_full_kernel_trace.csv; eight slices were two batched-copy launches)
      flat = torch.cat([s3, h3, st] + last + acc).tolist()
      s3, h3, st, rest = flat[0:3], flat[3:6], flat[6:6 + _lib.STUDY_SLOTS], flat[6 + _lib.STUDY_SLOTS:]
      last, acc = rest[:len(last)], rest[len(last):]
      sums = s3[_lib.OUT3_SUMS] + h3[_lib.OUT3_SUMS] + st[_lib.STUDY_SUMS] + st[_lib.STUDY_L2] + last
      maxes = s3[_lib.OUT3_MAX] + h3[_lib.OUT3_MAX] + st[_lib.STUDY_MAXES] + acc
    else:
      sums, maxes = self.agg.exchange(
        torch.cat([s3[_lib.OUT3_SUMS], h3[_lib.OUT3_SUMS], st[_lib.STUDY_SUMS], st[_lib.STUDY_L2]] + last),
        torch.cat([s3[_lib.OUT3_MAX], h3[_lib.OUT3_MAX], st[_lib.STUDY_MAXES]] + acc))
      ns = int(sums.numel())
      flat = torch.cat([sums, maxes]).tolist()
      sums, maxes = flat[:ns], flat[ns:]
    s2, sd, h2, hd = sums[0:4]
    st = sums[4:24]  # STUDY_SUMS: the slots of bm_study_stats keep their places
    gram, (ex0, ex1), (a2, ad) = st[_lib.STUDY_GRAM], st[_lib.STUDY_EX], st[_lib.STUDY_ATTACK]
    smax, hmax, amax, dmax = maxes[:4]
    return _StudyRecord(s2, sd, smax, h2, hd, hmax, a2, ad, amax, gram[4 * 2 + 2], dmax, sums[24], gram, ex0, ex1,
                        sums[25] if prev is not None else math.nan, maxes[4] if acc else math.nan)

  @staticmethod
  def _unpack(pend):
    """The statistics vector of bm_step_worker as a _StudyRecord."""
    vec = pend.packed if pend.prev is None else torch.cat([pend.packed, pend.prev[:1]])
    v = vec.tolist()  # the only synchronisation
    L = _lib
    return _StudyRecord(v[L.STEP_S2], v[L.STEP_SD], v[L.STEP_SMAX], v[L.STEP_H2], v[L.STEP_HD], v[L.STEP_HMAX],
                        v[L.STEP_A2], v[L.STEP_AD], v[L.STEP_AMAX], v[L.STEP_D2], v[L.STEP_DMAX], v[L.STEP_L2],
                        v[L.STEP_GRAM], v[L.STEP_EX.start], v[L.STEP_EX.start + 1],
                        v[len(pend.packed)] if pend.prev is not None else math.nan, v[L.STEP_ACCEPT])

  def _study_floats(self, rec, pend):
    """The study row (attack.py:828-868) from the scalars of either path."""
    nan = math.nan
    att, k_s, k_h, k_a = self.f_real > 0, pend.ks, self.h, self.f_real
    g = rec.gram

    def dev(x, k):
      return math.sqrt(x / (k - 1)) if k >= 2 else nan

    def cos(i, j):
      if not att and 3 in (i, j):  # (no attack: no fourth vector)
        return nan
      # (a vector of norm 0 — empire at a factor that cancels the average — divides like the reference's tensors: NaN)
      return _ieee_div(_ieee_div(g[4 * i + j], math.sqrt(g[5 * i])), math.sqrt(g[5 * j]))

    past = pend.npast > 0
    if self.plan.accept == "count":  # the reference's own `count / m`, int / int (krum.py:144-151 and its likes)
      accept = int(rec.accept) / pend.accept_of
    else:  # math.nan ITSELF where the rule has no `influence`: two steps' dictionaries then compare equal
      accept = self.f_real / self.n if self.plan.accept == "average" else nan
    return {
      "l2_origin": math.sqrt(rec.l2) if pend.has_l2 else nan,
      "sampled_norm_avg": math.sqrt(rec.s2), "sampled_norm_dev": dev(rec.sd, k_s), "sampled_norm_max": rec.smax,
      "honest_norm_avg": math.sqrt(rec.h2), "honest_norm_dev": dev(rec.hd, k_h), "honest_norm_max": rec.hmax,
      "attack_norm_avg": math.sqrt(rec.a2) if att else nan, "attack_norm_dev": dev(rec.ad, k_a) if att else nan,
      "attack_norm_max": rec.amax if att else nan,
      "defense_norm_avg": math.sqrt(rec.d2), "defense_norm_max": rec.dmax,
      "cosin_splhon": cos(0, 1), "cosin_spldef": cos(0, 2), "cosin_hondef": cos(1, 2),
      "cosin_splatt": cos(0, 3), "cosin_honatt": cos(1, 3), "cosin_attdef": cos(3, 2),
      "cosin_sampled": _ieee_div(_ieee_div(rec.ex0, math.sqrt(rec.s2)), math.sqrt(rec.prev_s2)) if past else nan,
      "curv_sampled": self.mu * rec.ex1 if past else nan,
      "accept_ratio": accept,
    }

  def floats(self):
    """Python floats of the study row (attack.py:822,828-868) for the last run(); synchronises once.
    Idempotent: a second call returns the same dictionary without touching the device — until a HIP graph is replayed
    (graphs.replay_epoch): a replay of this step rewrites the scalars where they are and creates no record, so the row
    is fetched again."""
    pend = self._pending
    if pend is None:
      raise RuntimeError("floats() needs a run() first")
    epoch = graphs.replay_epoch()
    if pend.floats is None or pend.epoch != epoch:
      if self.gar == "brute":
        self.agg.check_brute()  # (a step replayed from a HIP graph could not check inside run(): here at the latest)
      pend.floats = self._study_floats(self._unpack(pend) if pend.packed is not None else self._exchange(pend), pend)
      pend.epoch = epoch
    return pend.floats
