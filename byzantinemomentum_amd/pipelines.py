"""The rules whose whole decision is made on an n x n matrix of squared distances, written once for the two front ends:
gars (one device) and sharded.ShardedAggregator (a coordinate slice, the matrix all-reduced).

Every pipeline is a plain function over
  legs    the launching functions: center_weights, spectral_weights, weighted_sum, mixed_sqdist, mix_weights with the
          signatures of gars; rank(sq, n, f, m, mode) -> order; brute_select_device(sq, n, f) -> (sel, status), or None
          where there is no device search; host_selection(sq, n, f, like) -> the host search's selection as an index
          tensor where `like` lives (gars._Legs looks them up in its module at call time, torch_legs.Legs resolves a
          backend's once);
  sq_of   points -> their squared distances (gars: the distance pass; the aggregator: the pass with the total length,
          then the all-reduce)
and returns (out, Record): what the front end publishes in its own way (attributes of the result there, `last_*` here).
This module launches nothing itself and owns the tables and the argument checks both front ends share."""

import math
from typing import NamedTuple

import torch

from . import _lib

__all__ = ["GarInputError", "Record", "NNM_RULES", "SCALAR_RULES", "FORMS", "check_rule_form", "check_center_args",
           "check_spectral_args", "dnc_count", "center", "spectral", "on_scalars", "brute_resolve", "brute_search"]


class GarInputError(ValueError):
  """The gradients cannot be served by the HIP path (wrong device, dtype, layout or count)."""


class Record(NamedTuple):
  """What a pipeline decided, beside its output."""
  masks_made: object = None    # the masks as the callback made them (nnm_masks: int64[MAX_ROWS])
  masks_read: object = None    # the words mixed_sqdist / mix_weights read: the n_out made, then a start's own word
  weights: object = None       # fp64[MAX_ROWS] of the ORIGINAL rows (and the start): what the weighted sum read
  selection: object = None     # (index tensor, count) of krum / brute
  brute_status: object = None  # int32[1] where the search ran; None without a device search or after a host re-search
  info: object = None          # bm_center_weights' fp64[3] or bm_spectral_weights' fp64[4]


# the rules nnm / bucketing can run on the mixed rows, and whether they take f
NNM_RULES = {"median": False, "trmean": True, "phocas": True, "meamed": True, "krum": True, "bulyan": True, "brute": True,
             "aksel": True, "cge": True, "average": False, "geomed": False, "cclip": False, "caf": True, "dnc": True}
# the rules form="scalars" serves: their output on mixed rows needs the distances between mixed rows and a weighted sum
# of the original rows, nothing else
SCALAR_RULES = ("krum", "brute", "geomed", "cclip", "average")
FORMS = ("rows", "scalars")
BRUTE_NO_SUBSET = "brute: too many non-finite gradients, no subset of n-f rows has a finite diameter"


def check_rule_form(where, rule, form):
  """An unknown rule or form, or a rule form="scalars" does not serve: refused before anything looks at the tensors."""
  if rule not in NNM_RULES:
    raise ValueError(f"{where}: unknown rule {rule!r} ({', '.join(sorted(NNM_RULES))})")
  if form not in FORMS:
    raise ValueError(f"{where}: unknown form {form!r} ({', '.join(FORMS)})")
  if form == "scalars" and rule not in SCALAR_RULES:
    raise ValueError(f"{where}: form='scalars' serves {', '.join(SCALAR_RULES)} only, got rule {rule!r}")


def check_center_args(mode, param, iters, tol):
  """The arguments bm_center_weights refuses, refused here with their names (a ValueError)."""
  name = {"geomed": "nu", "cclip": "tau"}.get(mode)
  if name is None:
    raise ValueError(f"unknown mode {mode!r} (geomed, cclip)")
  if isinstance(param, bool) or not isinstance(param, (int, float)) or not (0 < param < float("inf")):
    raise ValueError(f"{mode}: {name} must be a positive finite number, got {param!r}")
  if isinstance(iters, bool) or not isinstance(iters, int) or not 1 <= iters <= _lib.CENTER_MAX_ITERS:
    raise ValueError(f"{mode}: iters must be an integer within 1..{_lib.CENTER_MAX_ITERS}, got {iters!r}")
  if isinstance(tol, bool) or not isinstance(tol, (int, float)) or not (0 <= tol < float("inf")):
    raise ValueError(f"{mode}: tol must be a finite number >= 0, got {tol!r}")


def check_spectral_args(mode, n, count, power_iters):
  """The arguments bm_spectral_weights refuses, refused here with their names (a ValueError)."""
  name = {"caf": "f", "dnc": "k"}.get(mode)
  if name is None:
    raise ValueError(f"unknown mode {mode!r} (caf, dnc)")
  if isinstance(count, bool) or not isinstance(count, int) or count < 0:
    raise ValueError(f"{mode}: {name} must be an integer >= 0, got {count!r}")
  if mode == "caf" and not 2 * count < n:
    raise ValueError(f"caf: 2 f < n is needed, got f = {count} with n = {n}")
  if mode == "dnc" and not count < n:
    raise ValueError(f"dnc: k < n is needed, got k = {count} with n = {n}")
  if (isinstance(power_iters, bool) or not isinstance(power_iters, int)
      or not 1 <= power_iters <= _lib.SPECTRAL_MAX_POWER_ITERS):
    raise ValueError(f"{mode}: power_iters must be an integer within 1..{_lib.SPECTRAL_MAX_POWER_ITERS}, "
                     f"got {power_iters!r}")


def dnc_count(n, f, c):
  """DnC's k = min(ceil(c f), n - 1), the rows it removes; f and c refused with their names."""
  if isinstance(f, bool) or not isinstance(f, int) or f < 0:
    raise ValueError(f"dnc: f must be an integer >= 0, got {f!r}")
  if isinstance(c, bool) or not isinstance(c, (int, float)) or not (0 <= c < float("inf")):
    raise ValueError(f"dnc: c must be a finite number >= 0, got {c!r}")
  return min(int(math.ceil(c * f)), max(n - 1, 0))


def _check_center(mode, param, iters, tol):
  if mode == "cclip" and param is None:
    raise ValueError("cclip: tau (the clipping radius) is required")
  check_center_args(mode, param, iters, tol)


def center(legs, sq_of, mode, rows, param, iters, tol, start):
  """geomed (param = nu) / cclip (param = tau, required; start or None): the squared distances of rows + [start], the
  weights of the iterate from them, the weighted sum of the points.  Record: weights (the start's being entry n), info."""
  _check_center(mode, param, iters, tol)
  rows = list(rows)
  points = rows + ([start] if start is not None else [])
  if not rows or len(points) > _lib.MAX_ROWS:
    raise GarInputError(f"{mode}: 1..{_lib.MAX_ROWS} gradients are supported"
                        f"{' (one fewer with a start vector)' if start is not None else ''}, got {len(rows)}")
  weights, info = legs.center_weights(sq_of(points), len(rows), mode, param, iters, tol, start is not None)
  return legs.weighted_sum(points, weights), Record(weights=weights, info=info)


def spectral(legs, sq_of, mode, rows, count, power_iters):
  """caf (count = f) / dnc (count = k): the squared distances of the rows, the weights of the filter from them, the
  weighted sum of the rows.  Record: weights, info."""
  rows = list(rows)
  if not rows or len(rows) > _lib.MAX_ROWS:
    raise GarInputError(f"{mode}: 1..{_lib.MAX_ROWS} gradients are supported, got {len(rows)}")
  check_spectral_args(mode, len(rows), count, power_iters)
  weights, info = legs.spectral_weights(sq_of(rows), len(rows), mode, count, power_iters)
  return legs.weighted_sum(rows, weights), Record(weights=weights, info=info)


def brute_resolve(sel, status, sq, n, f, check, host_search):
  """The status protocol of the device Brute search, once: (selection to average, status to publish) from the search's
  (sel, status).  The status is read — one 4-byte synchronisation — only when `check` is set and no capture is in
  progress on a device tensor: -1 raises like the reference (brute.py:68); -2, the node budget, repeats the search with
  host_search(sq, n, f), which has none, and publishes no status (None)."""
  if not check or (status.is_cuda and torch.cuda.is_current_stream_capturing()):
    return sel, status
  code = int(status.item())
  if code == -2:
    return host_search(sq, n, f), None
  if code != 0:
    raise RuntimeError(BRUTE_NO_SUBSET)
  return sel, status


def brute_search(legs, sq, n, f, check, like):
  """(selection, status) of the Brute rule on the squared distances `sq`: the device search through brute_resolve, or
  the host search where the legs have no device search (status None)."""
  def host_search(sq, n, f):
    return legs.host_selection(sq, n, f, like)
  if legs.brute_select_device is None:
    return host_search(sq, n, f), None
  return brute_resolve(*legs.brute_select_device(sq, n, f), sq, n, f, check, host_search)


def on_scalars(legs, sq_of, rows, rule, f, n_out, masks_from, need_sq, rule_args):
  """`rule` (one of SCALAR_RULES, its f being `f`) on the n_out mixed rows of `rows` without writing one: the squared
  distances of the ORIGINAL rows (and of a cclip start, point n) -> masks_from(the n x n matrix of the rows, or None when
  neither the masks (need_sq) nor the rule read distances) -> mixed_sqdist -> the rule's own scalar stage -> mix_weights
  -> weighted_sum.  The one synchronisation is brute's with check=True.  Record: everything but `info` for krum / brute,
  the centre info for geomed / cclip."""
  rows, args = list(rows), dict(rule_args)
  n, start, selection, status, info = len(rows), None, None, None, None
  if rule == "geomed":
    param, iters = args.pop("nu", 1e-6), args.pop("iters", 8)
  elif rule == "cclip":
    param, iters, start = args.pop("tau", None), args.pop("iters", 3), args.pop("start", None)
  if rule in ("geomed", "cclip"):
    tol = args.pop("tol", 0.0)
    _check_center(rule, param, iters, tol)
  points = rows + ([start] if start is not None else [])
  n_in, n_mixed = len(points), n_out + (start is not None)
  if n_in > _lib.MAX_ROWS:
    raise GarInputError(f"cclip: at most {_lib.MAX_ROWS - 1} gradients are supported with a start vector, got {n}")
  sq = sq_of(points) if need_sq or rule != "average" else None
  made = masks = masks_from(sq if start is None or sq is None else sq[:n, :n].contiguous())
  if start is not None:  # the start is point n of the pass and mixed row n_out, alone in its mask
    own = torch.full((1,), (1 << n) - (1 << 64 if n == 63 else 0), dtype=torch.int64, device=masks.device)
    masks = torch.cat((masks[:n_out], own))
  if rule == "average":
    even = torch.full((_lib.MAX_ROWS,), 1.0 / n_out, dtype=torch.float64, device=masks.device)
    w = legs.mix_weights(masks, n_in, n_out, weights=even)
  else:
    mixed = legs.mixed_sqdist(sq, n_in, masks, n_mixed)
    if rule == "krum":
      m = args.pop("m", None)
      if m is None:
        m = n_out - f - 2
      selection = (legs.rank(mixed, n_out, f, m, _lib.RANK_KRUM), m)
    elif rule == "brute":
      sel, status = brute_search(legs, mixed, n_out, f, args.pop("check", False), rows[0])
      selection = (sel, n_out - f)
    if selection is not None:
      w = legs.mix_weights(masks, n_in, n_out, selection=selection[0], m=selection[1])
    else:
      weights, info = legs.center_weights(mixed, n_out, rule, param, iters, tol, start is not None)
      w = legs.mix_weights(masks, n_in, n_mixed, weights=weights)
  return legs.weighted_sum(points, w), Record(made, masks, w, selection, status, info)
