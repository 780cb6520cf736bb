"""Per-step gradient statistics and momentum of the simulation loop, on the HIP path.

Mirrors tools/pytorch.py:97-125 (`compute_avg_dev_max`), the study block of attack.py:842-868
(norms, max-abs, six cosines, past-gradient cosine and curvature) and the worker-side momentum
update of attack.py:800-804.  One fused pass per stack and one fused pass for all the dot
products; results stay on the device until the caller asks for Python floats (one sync).
"""

import ctypes
import os
import math

import torch

from . import _lib
from . import gars

__all__ = ["compute_avg_dev_max", "stack_stats_async", "study_dots", "study_stats", "multi_axpby", "row_sqnorms", "momentum_stats", "momentum_stats_colwise", "momentum_stats_sqdist", "stack_stats_colwise", "stack_stats_sqdist",
           "multi_fma3", "clip_factors", "clip_factors_from_sq", "multi_scale", "clip_gradients", "l2_distance",
           "step_worker", "anticge_sum", "anticge_scale", "anticge_attack", "accept_count",
           "attack_vector", "nan_attack", "bulyan_attack", "empire_strict_attack",
           "perturb_stats", "minmax_factor", "minmax_attack", "minsum_attack"]

_ptr = gars._ptr


def _opt(t):
  return _ptr(t) if t is not None else None


def _require_scalar_on(t, device, message):  # a factor or a cursor handed over in DEVICE memory
  if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == device and t.dtype == torch.float64
          and t.numel() >= 1 and t.is_contiguous()):
    raise gars.GarInputError(message)


def _require_ext(ext, h):  # the squared distances among honests + [avg, avg + att] of the search's scalar forms
  if not (isinstance(ext, torch.Tensor) and ext.is_cuda and ext.dtype == torch.float64 and ext.is_contiguous()
          and tuple(ext.shape) == (h + 2, h + 2)):
    raise gars.GarInputError(f"ext must be a contiguous float64 device tensor of shape ({h + 2}, {h + 2})")


def _attack_id(attack, direction):
  kind = _lib.ATTACK_LITTLE if attack == "little" else _lib.ATTACK_EMPIRE
  return kind | (_lib.ATTACK_DIRECTION if direction else 0)


def stack_stats_async(samples, scale=None, attack="empire", want_avg=True, direction=False):
  """avg vector + device tensor [sum avg^2, sum_i ||s_i-avg||^2, max|avg|] (fp64), no sync.

  With `scale`, also returns the Byzantine vector of an "identical" attack computed in the same pass
  (third element of the tuple): attack="empire" -> avg + scale*(-avg); attack="little" ->
  avg + scale*sqrt(unbiased column variance) (attacks/identical.py:63-86,129-141).
  direction=True: the third element is scale * (attack direction) alone, without the average
  (`grad_att` of identical.py:65, what the factor search combines with the average).
  """
  k, d, device = gars._validate(samples)
  lib = _lib.load()
  avg = torch.empty(d, dtype=torch.float32, device=device) if want_avg else None  # None: statistics only
  scaled = torch.empty(d, dtype=torch.float32, device=device) if scale is not None else None
  out3 = torch.empty(3, dtype=torch.float64, device=device)
  ws = gars._workspace(device, _lib.WS_STATS, k, d, "ws_stats")
  with torch.cuda.device(device):
    _lib.check(lib.bm_stack_stats(_lib.pointer_table(samples), k, d, _opt(avg), _opt(scaled),
                                  ctypes.c_float(scale if scale is not None else 0.0),
                                  _attack_id(attack, direction), _ptr(out3),
                                  _ptr(ws), gars._stream(device)), "bm_stack_stats")
  if scale is not None:
    return avg, out3, scaled
  return avg, out3


def compute_avg_dev_max(samples):
  """Drop-in for tools.compute_avg_dev_max (tools/pytorch.py:97-125).

  Returns (average gradient or None, norm of the average, norm standard deviation, max |coord|).
  """
  if len(samples) == 0:
    return None, math.nan, math.nan, math.nan
  avg, out3 = stack_stats_async(samples)
  norm2, dev2, amax = out3.tolist()  # the only synchronisation
  k = len(samples)
  norm_dev = math.sqrt(dev2 / (k - 1)) if k >= 2 else math.nan
  return avg, math.sqrt(norm2), norm_dev, amax


def study_dots(core, extra=()):
  """Gram matrix (fp64, nc x nc) of up to 4 vectors and dot(core[0], e) for up to 32 more.

  Covers every `torch.dot`/`norm` of attack.py:851-868 in one pass over the vectors.
  Returns (gram tensor nc x nc, extras tensor ne), both on the device.
  """
  core = list(core)
  extra = list(extra)
  nc, d, device = gars._validate(core)
  if extra:
    gars._validate(extra + [core[0]])
  lib = _lib.load()
  out = torch.empty(nc * nc + len(extra), dtype=torch.float64, device=device)
  ws = gars._workspace(device, _lib.WS_DOT, 1, d, "ws_dot")
  with torch.cuda.device(device):
    _lib.check(lib.bm_multi_dot(_lib.pointer_table(core), nc,
                                _lib.pointer_table(extra) if extra else None, len(extra), d, _ptr(out),
                                _ptr(ws), gars._stream(device)), "bm_multi_dot")
  return out[:nc * nc].view(nc, nc), out[nc * nc:]


_EVAL_OPS = {"trmean": _lib.OP_TRMEAN, "phocas": _lib.OP_PHOCAS, "meamed": _lib.OP_MEAMED, "median": _lib.OP_MEDIAN}


def colwise_eval_supported(rule, n):
  """Does the evaluate-only form of the factor search exist for this rule and worker count (bm_colwise_eval)?"""
  return rule in _EVAL_OPS and bool(_lib.load().bm_colwise_eval_supported(_EVAL_OPS[rule], n))


def colwise_eval(rule, honests, copies, f, h_avg, direction, t):
  """| RULE(honests + [h_avg + t * direction] * copies) - h_avg |^2 as a device fp64[1] tensor, the candidate and the
  rule's output formed in registers only (bm_colwise_eval): one candidate of attacks/identical.py:67-77. No sync.
  t: a number, or the DEVICE float64 tensor a DeviceSearch left its candidate in (bm_colwise_eval_tdev)."""
  honests = list(honests)
  h, d, device = gars._validate(honests)
  gars._validate([h_avg, direction] + honests[:1])
  lib = _lib.load()
  out = torch.empty(1, dtype=torch.float64, device=device)
  ws = gars._Scratch.get(device, "ws_eval", nbytes=int(lib.bm_colwise_eval_workspace_bytes()))
  with torch.cuda.device(device):
    if isinstance(t, torch.Tensor):
      _require_scalar_on(t, device, "colwise_eval: a tensor t must be a contiguous float64 tensor on the vectors' device")
      _lib.check(lib.bm_colwise_eval_tdev(_EVAL_OPS[rule], _lib.pointer_table(honests), h, copies, d, f, _ptr(h_avg),
                                          _ptr(direction), _ptr(t), _ptr(out), _ptr(ws), gars._stream(device)),
                 "bm_colwise_eval_tdev")
    else:
      _lib.check(lib.bm_colwise_eval(_EVAL_OPS[rule], _lib.pointer_table(honests), h, copies, d, f, _ptr(h_avg),
                                     _ptr(direction), float(t), _ptr(out), _ptr(ws), gars._stream(device)),
                 "bm_colwise_eval")
  return out


def sqdist2(a, b):
  """|a - b|^2 as a device fp64[1] tensor in one pass over the two vectors (bm_sqdist2): the objective of a candidate of
  the factor search (identical.py:75-76).  No sync."""
  _, d, device = gars._validate([a, b])
  lib = _lib.load()
  out = torch.empty(1, dtype=torch.float64, device=device)
  ws = gars._Scratch.get(device, "ws_eval", nbytes=int(lib.bm_colwise_eval_workspace_bytes()))
  with torch.cuda.device(device):
    _lib.check(lib.bm_sqdist2(_ptr(a), _ptr(b), d, _ptr(out), _ptr(ws), gars._stream(device)), "bm_sqdist2")
  return out


def bulyan_pass2_eval_supported(n, f, m, d=0):
  """Is there an evaluate-only instance of Bulyan's second pass for this shape (bm_bulyan_pass2_eval)?"""
  return d <= (1 << 29) and bool(_lib.load().bm_bulyan_pass2_eval_supported(int(n), int(f), int(m)))


def bulyan_pass2_eval(honests, copies, order, f, m, h_avg, direction, t):
  """| pass2(honests + [h_avg + t * direction] * copies, order) - h_avg |^2 as a device fp64[1] tensor, the candidate in
  registers only (bm_bulyan_pass2_eval): one candidate of attacks/identical.py:67-77 against Bulyan, given the ranking of
  the stack (device int32 tensor; indices >= len(honests) name a copy of the candidate).  t: a number, or a DEVICE
  float64 tensor.  No sync."""
  honests = list(honests)
  h, d, device = gars._validate(honests)
  gars._validate([h_avg, direction] + honests[:1])
  lib = _lib.load()
  out = torch.empty(1, dtype=torch.float64, device=device)
  ws = gars._Scratch.get(device, "ws_eval", nbytes=int(lib.bm_colwise_eval_workspace_bytes()))
  t_dev = None
  if isinstance(t, torch.Tensor):
    _require_scalar_on(t, device, "bulyan_pass2_eval: a tensor t must be a contiguous float64 tensor on the vectors' device")
    t_dev, t = t, 0.0
  with torch.cuda.device(device):
    _lib.check(lib.bm_bulyan_pass2_eval(_lib.pointer_table(honests), h, int(copies), _ptr(order), int(f), int(m), d,
                                        _ptr(h_avg), _ptr(direction), ctypes.c_float(float(t)), _opt(t_dev), _ptr(out),
                                        _ptr(ws), gars._stream(device)), "bm_bulyan_pass2_eval")
  return out


def order_pair_supported(h):
  """Is there a one-pass form of two order statistics of h rows (bm_order_pair)?"""
  return bool(_lib.load().bm_order_pair_supported(int(h)))


def order_pair(rows, il, ih):
  """(lo, hi): per coordinate the values of rank il and ih (0-based, ascending) among the rows; -inf below rank 0, +inf
  beyond the last rank, NaN where the column holds one (bm_order_pair).  One pass over the rows, no sync: the two
  vectors of the median's factor search (median.py:31-39 on the rows with k copies of -inf / +inf)."""
  rows = list(rows)
  h, d, device = gars._validate(rows)
  lib = _lib.load()
  lo, hi = torch.empty_like(rows[0]), torch.empty_like(rows[0])
  with torch.cuda.device(device):
    _lib.check(lib.bm_order_pair(_lib.pointer_table(rows), h, d, int(il), int(ih), _ptr(lo), _ptr(hi),
                                 gars._stream(device)), "bm_order_pair")
  return lo, hi


class DeviceSearch:
  """The cursor of tools.line_maximize (tools/misc.py:468-514) kept in device memory (bm_search_device_next): `next(y)`
  takes the objective the last evaluation left on the device (None the first time) and returns the DEVICE float64[1]
  tensor holding the next candidate's signed factor — hand it to multi_fma3 / colwise_eval as b / t —, `finish(y)`
  returns the float64 device tensor [factor, x0, y0, x1, y1, ...] of attack_search_device.  Nothing is awaited: the
  host queues the whole search."""

  def __init__(self, device, evals, negative=False, start=0., delta=1., ratio=0.8):
    if not isinstance(evals, int) or evals < 1:
      _lib.check(_lib.EINVAL, "DeviceSearch (evals must be a positive integer)")
    self.device, self.evals, self.negative, self.shape = device, evals, bool(negative), (start, delta, ratio)
    self.state = torch.zeros(8, dtype=torch.float64, device=device)   # sizeof(bm_search) = 56 bytes
    self.t = torch.zeros(1, dtype=torch.float64, device=device)
    self.out = torch.zeros(1 + 2 * evals, dtype=torch.float64, device=device)
    self.proposed = 0
    self._keep = None

  def _call(self, y, last):
    if y is not None and not (isinstance(y, torch.Tensor) and y.is_cuda and y.device == self.device
                              and y.dtype == torch.float64 and y.numel() >= 1):
      raise gars.GarInputError("DeviceSearch: the objective must be a float64 tensor on the search's device")
    lib = _lib.load()
    self._keep = y  # (alive until the kernel that reads it has been queued behind its producer)
    with torch.cuda.device(self.device):
      _lib.check(lib.bm_search_device_next(_ptr(self.state), _opt(y), 1 if self.negative else 0,
                                           1 if last else 0, *self.shape, _ptr(self.t) if not last else None,
                                           _ptr(self.out), gars._stream(self.device)), "bm_search_device_next")

  def next(self, y=None):
    if self.proposed >= self.evals or (y is None) != (self.proposed == 0):
      raise RuntimeError("DeviceSearch.next: one objective per candidate, `evals` candidates")
    self._call(y, False)
    self.proposed += 1
    return self.t

  def finish(self, y):
    if self.proposed != self.evals:
      raise RuntimeError("DeviceSearch.finish: the search has candidates left")
    self._call(y, True)
    return self.out


def study_stats(s_avg, h_avg, defense, byz, f_real, past_newest=None, curv=None, past_oldest=None, curv_mode=0, mu=0.0,
                oldest_weight=0.0, params=None, origin=None, attack_avg_out=None, update_momentum=None, update_mu=0.0,
                update_omd=0.0):
  """The study block of a step in ONE pass (bm_study_stats, include/bm_gar.h): statistics of the attack stack
  (f_real copies of `byz`) and of the defense vector, the Gram matrix of (sampled avg, honest avg, defense, attack
  avg), <s, past_newest>, <s, C>, |params - origin|^2, and the in-place update of the curvature combination C =
  `curv` for the next step (curv_mode: 0 none, 1 C <- s, 2 C <- s + mu C, 3 the same after taking
  oldest_weight * past_oldest out of C).  update_momentum: the momentum of the update (attack.py:836-838), updated in
  place in the same pass: M <- update_omd * defense + update_mu * M (bm_study_stats_update).
  Returns the device fp64 vector of STUDY_SLOTS statistics; no sync."""
  vecs = [t for t in (s_avg, h_avg, defense, byz if f_real > 0 else None, past_newest if curv_mode >= 2 else None,
                      curv if curv_mode >= 1 else None, past_oldest if curv_mode == 3 else None, params, origin,
                      attack_avg_out, update_momentum) if t is not None]
  _, d, device = gars._validate(vecs)
  if (params is None) != (origin is None):
    raise gars.GarInputError("study_stats needs both params and origin, or neither")
  lib = _lib.load()
  out = torch.empty(_lib.STUDY_SLOTS, dtype=torch.float64, device=device)
  ws = gars._workspace(device, _lib.WS_STUDY, 1, d, "ws_study")
  with torch.cuda.device(device):
    _lib.check(lib.bm_study_stats_update(_ptr(s_avg), _ptr(h_avg), _ptr(defense), _opt(byz if f_real > 0 else None),
                                         int(f_real), _opt(attack_avg_out), _opt(past_newest), _opt(curv), _opt(past_oldest),
                                         int(curv_mode), ctypes.c_float(mu), ctypes.c_float(oldest_weight), _opt(params),
                                         _opt(origin), _opt(update_momentum), ctypes.c_float(update_mu),
                                         ctypes.c_float(update_omd), d, _ptr(out), _ptr(ws), gars._stream(device)),
               "bm_study_stats_update")
  if update_momentum is not None:
    gars.invalidate_rank_cache()  # (a user tensor was written)
  return out


def row_sqnorms(gradients):
  """Squared L2 norm of every gradient (fp64, on the device): one read of the stack, one call (bm_row_sqnorms)."""
  n, d, device = gars._validate(gradients)
  lib = _lib.load()
  res = torch.empty(_lib.MAX_ROWS, dtype=torch.float64, device=device)
  ws = gars._workspace(device, _lib.WS_DOT, 1, d, "ws_dot")
  with torch.cuda.device(device):
    _lib.check(lib.bm_row_sqnorms(_lib.pointer_table(gradients), n, d, _ptr(res), _ptr(ws), gars._stream(device)),
               "bm_row_sqnorms")
  return res[:n]


def anticge_sum(gradients, f_decl, row_sq):
  """First leg of the `anticge` attack (attacks/anticge.py:64-72, bm_anticge_sum) from the honest gradients and their
  squared norms `row_sq` (device fp64, what row_sqnorms returns; the global ones under sharding): the rows are ranked by
  norm on the device and the selected ones summed in the reference's order.  Returns (S, order, scal): the unscaled
  attack vector (a fresh tensor), the ranking (int32[MAX_ROWS]) and the device fp64 pair [sum S^2 over these
  coordinates, squared norm of the first row left out] that anticge_scale reads.  No sync."""
  h, d, device = gars._validate(gradients)
  if not 1 <= f_decl <= h:
    raise gars.GarInputError(f"anticge needs 1 <= f_decl <= {h} honest gradients, got f_decl = {f_decl}")
  if not (isinstance(row_sq, torch.Tensor) and row_sq.device == device and row_sq.dtype == torch.float64
          and row_sq.numel() >= h and row_sq.is_contiguous()):
    raise gars.GarInputError("anticge_sum: row_sq must be a contiguous float64 tensor of h squared norms on the gradients' device")
  lib = _lib.load()
  out = torch.empty(d, dtype=torch.float32, device=device)
  order = torch.empty(_lib.MAX_ROWS, dtype=torch.int32, device=device)
  scal = torch.empty(2, dtype=torch.float64, device=device)
  ws = gars._Scratch.get(device, "ws_anticge", nbytes=int(lib.bm_anticge_workspace_bytes(d)))
  with torch.cuda.device(device):
    _lib.check(lib.bm_anticge_sum(_lib.pointer_table(gradients), h, d, int(f_decl), _ptr(row_sq), _ptr(out), _ptr(order),
                                  _ptr(scal), _ptr(ws), gars._stream(device)), "bm_anticge_sum")
  return out, order, scal


def anticge_scale(vec, scal):
  """Second leg (attacks/anticge.py:68,74-76, bm_anticge_scale): vec *= -nextafter(norm_(maxpos), 0) / |S| in place, the
  multiplier formed on the device from `scal` of anticge_sum (scal[0] all-reduced first under sharding).  No sync."""
  _, d, device = gars._validate([vec])
  _require_scalar_on(scal, device, "anticge_scale: scal must be a contiguous float64 tensor on the vector's device")
  if scal.numel() < 2:
    raise gars.GarInputError("anticge_scale: scal must hold the two scalars anticge_sum left")
  lib = _lib.load()
  gars.invalidate_rank_cache()
  with torch.cuda.device(device):
    _lib.check(lib.bm_anticge_scale(_ptr(vec), d, _ptr(scal), gars._stream(device)), "bm_anticge_scale")
  return vec


def anticge_attack(grad_honests, f_decl, f_real, **kwargs):
  """Drop-in for the reference's `anticge` attack (attacks/anticge.py:49-78): `f_real` references to ONE new tensor,
  the negated sum of the h - f_decl honest gradients of smallest norm (the smallest counted twice, as the reference
  does), scaled to just below the norm of the next one.  f_real > f_decl: the all-NaN vector of anticge.py:60-63.
  Row norms, ranking, sum, norm and scaling all run on the device, on the current stream, without a synchronisation.
  **kwargs: ignored, like the keyword arguments the reference's attacks are handed and do not know (attacks/__init__.py:15-17)."""
  grad_honests = list(grad_honests)
  h, d, device = gars._validate(grad_honests)
  if f_real <= 0:
    return []
  if f_real > f_decl:
    return [torch.full_like(grad_honests[0], math.nan)] * f_real
  byz, _, scal = anticge_sum(grad_honests, f_decl, row_sqnorms(grad_honests).contiguous())
  return [anticge_scale(byz, scal)] * f_real


def _perturbation_id(perturbation):
  if perturbation not in _lib.PERTURB_KINDS:
    raise gars.GarInputError(f"unknown perturbation {perturbation!r} (one of {sorted(_lib.PERTURB_KINDS)})")
  return _lib.PERTURB_KINDS[perturbation]


def _minmax_mode_id(mode):
  if mode not in _lib.MINMAX_MODES:
    raise gars.GarInputError(f"unknown mode {mode!r} (one of {sorted(_lib.MINMAX_MODES)})")
  return _lib.MINMAX_MODES[mode]


def _require_honests(h, what):
  if not 2 <= h <= _lib.MAX_ROWS:
    raise gars.GarInputError(f"{what} needs 2 <= h <= {_lib.MAX_ROWS} honest gradients, got h = {h}")


def perturb_stats(grad_honests, perturbation):
  """What the closed form of the Min-Max / Min-Sum attacks needs from the vectors, in ONE pass over the h honest rows
  (bm_perturb_stats, include/bm_gar.h): (avg, dir, scal) — the sequential fp32 average (the bits of stack_stats_async's),
  the perturbation direction p ("unit": -avg, "std": -sqrt(unbiased column variance), "sign": -sign(avg)) and the
  device fp64[PERTURB_SLOTS] scalars [b_0 .. b_{h-1}, zeros, |p|^2, |avg|^2], b_i = <p, avg - g_i>, over THESE
  coordinates (all are sums: under sharding they are all-reduced).  Fresh tensors; no sync."""
  kind = _perturbation_id(perturbation)
  grad_honests = list(grad_honests)
  _require_honests(len(grad_honests), "perturb_stats")
  h, d, device = gars._validate(grad_honests)
  lib = _lib.load()
  avg = torch.empty(d, dtype=torch.float32, device=device)
  direction = torch.empty(d, dtype=torch.float32, device=device)
  scal = torch.empty(_lib.PERTURB_SLOTS, dtype=torch.float64, device=device)
  ws = gars._Scratch.get(device, "ws_perturb", nbytes=int(lib.bm_perturb_workspace_bytes(d)))
  with torch.cuda.device(device):
    _lib.check(lib.bm_perturb_stats(_lib.pointer_table(grad_honests), h, d, kind, _ptr(avg), _ptr(direction), _ptr(scal),
                                    _ptr(ws), gars._stream(device)), "bm_perturb_stats")
  return avg, direction, scal


def minmax_factor(sq, scal, h, mode):
  """The closed-form factor of the Min-Max ("minmax") or Min-Sum ("minsum") attack (bm_minmax_factor, include/bm_gar.h)
  from the h x h squared distances of the honest rows and the scalars of perturb_stats — both possibly all-reduced.
  `sq` on the device: one workgroup, no copy, no synchronisation; `sq` on the host: the host form, same bits.  Returns
  fp64[6] where `sq` lives: [gamma, the bound R or S, the binding row or -1, |p|^2, |avg|^2, degenerate 0 / 1]."""
  mode_id = _minmax_mode_id(mode)
  h = int(h)
  _require_honests(h, mode)
  for t, count, what in ((sq, h * h, f"a matrix of {h} x {h} squared distances"),
                         (scal, _lib.PERTURB_SLOTS, f"the {_lib.PERTURB_SLOTS} scalars of perturb_stats")):
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.numel() >= count and t.is_contiguous()):
      raise gars.GarInputError(f"{mode}: expected a contiguous float64 tensor holding {what}")
  if scal.device != sq.device:
    raise gars.GarInputError(f"{mode}: the distances and the scalars must live on one device")
  lib = _lib.load()
  out = torch.empty(_lib.MINMAX_OUT, dtype=torch.float64, device=sq.device)
  args = (_ptr(sq), _ptr(scal), h, mode_id, _ptr(out))
  if not sq.is_cuda:
    _lib.check(lib.bm_minmax_factor(*args), "bm_minmax_factor")
    return out
  with torch.cuda.device(sq.device):
    _lib.check(lib.bm_minmax_factor_device(*args, gars._stream(sq.device)), "bm_minmax_factor_device")
  return out


def _minmax_attack(mode, grad_honests, f_real, perturbation):
  _perturbation_id(perturbation)
  grad_honests = list(grad_honests)
  _require_honests(len(grad_honests), f"the {mode} attack")
  h = gars._validate(grad_honests)[0]
  if f_real <= 0:
    return []
  avg, direction, scal = perturb_stats(grad_honests, perturbation)
  info = minmax_factor(gars.pairwise_sqdist(grad_honests), scal, h, mode)
  byz = torch.empty_like(avg)
  multi_fma3([byz], [avg], [direction], 1.0, info)  # avg + gamma * p, gamma read where the kernel left it
  byz.attack_factor, byz.attack_info = info[:1], info
  return [byz] * f_real


def minmax_attack(grad_honests, f_real, perturbation="std", **kwargs):
  """The Min-Max attack of Shejwalkar & Houmansadr (NDSS 2021), in the shape of the reference's attacks: `f_real`
  references to ONE new tensor avg + gamma * p, gamma the largest factor that keeps the vector no farther from any
  honest gradient than the two farthest honest gradients are from each other.  gamma is the closed form of
  include/bm_gar.h, not the paper's halving search: one pass over the rows for the scalars (perturb_stats), the distance
  pass, one workgroup on scalars (minmax_factor) and one streaming kernel for the vector, all on the current stream
  without a synchronisation.  perturbation: "unit", "std" (default) or "sign".  The tensor carries `.attack_factor`
  (device fp64[1]) and `.attack_info` (device fp64[6], minmax_factor's).  2 <= h <= 64 honest gradients.
  **kwargs: ignored, like the keyword arguments the reference's attacks are handed and do not know."""
  return _minmax_attack("minmax", grad_honests, f_real, perturbation)


def minsum_attack(grad_honests, f_real, perturbation="std", **kwargs):
  """The Min-Sum attack of the same paper: as minmax_attack, with gamma the largest factor that keeps the SUM of the
  vector's squared distances to the honest gradients within the largest such sum of an honest gradient."""
  return _minmax_attack("minsum", grad_honests, f_real, perturbation)


def attack_vector(kind, h_avg, factor=None, target=None, want_direction=False):
  """The Byzantine vector of the `nan`, `bulyan` and `empire-strict` attacks from the honest average, one streaming pass
  (bm_attack_vector): kind "nan" -> every coordinate NaN (attacks/nan.py:36-40; `h_avg` gives shape and device only),
  "shift_one" -> h_avg + factor * e_target, "shift_all" -> h_avg + factor (attacks/identical.py:114-127,82-84),
  "scale" -> h_avg * factor (attacks/empire.py:61-62 with factor = -epsilon).  factor: a number, or a DEVICE float64
  tensor whose first element the kernel reads (as multi_fma3 takes it).  target ("shift_one"): a coordinate of THIS
  tensor, or None / -1 when another rank holds it.  want_direction ("shift_*"): the 0 / 1 direction vector is stored by
  the same launch; returns (vector, direction) then, else the vector — fresh tensors, `h_avg` untouched.  No sync."""
  if kind not in _lib.ATTACK_VECTOR_KINDS:
    raise gars.GarInputError(f"attack_vector: unknown kind {kind!r} (one of {sorted(_lib.ATTACK_VECTOR_KINDS)})")
  _, d, device = gars._validate([h_avg])
  shift = kind in ("shift_one", "shift_all")
  if want_direction and not shift:
    raise gars.GarInputError(f"attack_vector: kind {kind!r} has no direction vector to store")
  if kind != "nan" and factor is None:
    raise gars.GarInputError(f"attack_vector: kind {kind!r} needs a factor")
  target = -1 if target is None or kind != "shift_one" else int(target)
  if not -1 <= target < d:
    raise gars.GarInputError(f"attack_vector: target must be a coordinate within [0, {d}) or -1, got {target}")
  lib = _lib.load()
  out = torch.empty_like(h_avg)
  direction = torch.empty_like(h_avg) if want_direction else None
  with torch.cuda.device(device):
    if isinstance(factor, torch.Tensor):
      _require_scalar_on(factor, device, "attack_vector: a tensor factor must be a contiguous float64 tensor on the vector's device")
      host, dev = 0.0, _ptr(factor)
    else:
      host, dev = (0.0 if factor is None else float(factor)), None
    _lib.check(lib.bm_attack_vector(_lib.ATTACK_VECTOR_KINDS[kind], _ptr(h_avg), d, target, ctypes.c_float(host), dev,
                                    _ptr(out), _opt(direction), gars._stream(device)), "bm_attack_vector")
  return (out, direction) if want_direction else out


def _searched(grad_honests, avg, candidate, f_real, f_decl, defense, evals, kwargs):
  """tools.line_maximize of |defense(honests + [candidate(x)] * f_real) - avg|^2 (attacks/identical.py:67-77,
  attacks/empire.py:51-59): the generic search through the caller's rule, one synchronisation per evaluation."""
  from . import linesearch
  if not callable(defense):
    raise gars.GarInputError(f"a searched attack needs the aggregation rule to defeat as `defense`, got {defense!r}")

  def scape(x):
    aggregated = defense(gradients=(grad_honests + [candidate(x)] * f_real), f=f_decl, model=kwargs.get("model"))
    return sqdist2(aggregated, avg).item()
  return linesearch.line_maximize(scape, evals=evals)[0]


def nan_attack(grad_honests, f_real, **kwargs):
  """Drop-in for the reference's `nan` attack (attacks/nan.py:24-40): `f_real` references to ONE new all-NaN tensor."""
  grad_honests = list(grad_honests)
  gars._validate(grad_honests)
  if f_real <= 0:
    return []
  return [attack_vector("nan", grad_honests[0])] * f_real


def bulyan_attack(grad_honests, f_real, f_decl=None, defense=None, factor=-16, negative=False, target_idx=-1, **kwargs):
  """Drop-in for the reference's `bulyan` attack (attacks/identical.py:45-86,114-127): `f_real` references to ONE new
  tensor avg + factor * dir, dir = all ones for target_idx "all", else one-hot at target_idx (a Python index, negative
  ones count from the end).  factor > 0: fixed (negated by `negative`); factor < 0: searched within ceil(-factor)
  evaluations of `defense(gradients=..., f=f_decl, model=...)`, `negative` flipping the candidates during the search
  only, as the reference does.  The inputs are left untouched."""
  grad_honests = list(grad_honests)
  _, d, device = gars._validate(grad_honests)
  if f_real <= 0:
    return []
  if target_idx == "all":
    kind, target = "shift_all", None
  else:
    if not isinstance(target_idx, int) or isinstance(target_idx, bool):
      raise gars.GarInputError(f"expected an integer or \"all\" for 'target_idx', got {target_idx!r}")
    if not -d <= target_idx < d:
      raise IndexError(f"index {target_idx} is out of bounds for dimension 0 with size {d}")
    kind, target = "shift_one", target_idx % d
  avg = stack_stats_async(grad_honests)[0]
  if factor < 0:
    sign = -1.0 if negative else 1.0
    factor = _searched(grad_honests, avg, lambda x: attack_vector(kind, avg, sign * x, target), f_real, f_decl, defense,
                       math.ceil(-factor), kwargs)
  elif negative:
    factor = -factor
  return [attack_vector(kind, avg, factor, target)] * f_real


def empire_strict_attack(grad_honests, f_real, f_decl=None, defense=None, epsilon=1, **kwargs):
  """Drop-in for the reference's `empire-strict` attack (attacks/empire.py:29-64): `f_real` references to ONE new tensor
  avg * (-epsilon).  epsilon > 0: fixed; epsilon < 0: searched within ceil(-epsilon) evaluations of
  `defense(gradients=..., f=f_decl, model=...)`.  The inputs are left untouched."""
  grad_honests = list(grad_honests)
  gars._validate(grad_honests)
  if f_real <= 0:
    return []
  avg = stack_stats_async(grad_honests)[0]
  if epsilon < 0:
    epsilon = _searched(grad_honests, avg, lambda x: attack_vector("scale", avg, -x), f_real, f_decl, defense,
                        math.ceil(-epsilon), kwargs)
  return [attack_vector("scale", avg, -epsilon)] * f_real


def accept_count(order, count, h):
  """How many of the first `count` entries of `order` (DEVICE int32 row indices: the ranking or the subset a rule left)
  are >= h, as a device fp64[1] tensor holding that integer (bm_accept_count, one wavefront).  With gradients = honests
  + attacks and h honests it is the numerator of the rule's `influence` (attack.py:822).  No sync."""
  if not (isinstance(order, torch.Tensor) and order.is_cuda and order.dtype == torch.int32 and order.dim() == 1
          and order.is_contiguous()):
    raise gars.GarInputError("accept_count: order must be a contiguous 1-D int32 tensor on a GPU")
  if not 0 <= count <= min(_lib.MAX_ROWS, order.numel()) or h < 0:
    raise gars.GarInputError(f"accept_count: count must be within 0..{min(_lib.MAX_ROWS, order.numel())} and h >= 0, "
                             f"got count = {count}, h = {h}")
  device = order.device
  out = torch.empty(1, dtype=torch.float64, device=device)
  with torch.cuda.device(device):
    _lib.check(_lib.load().bm_accept_count(_ptr(order), int(count), int(h), _ptr(out), gars._stream(device)),
               "bm_accept_count")
  return out


def multi_axpby(ys, xs, a, b):
  """In place y_i <- a*y_i + b*x_i for every pair: `gmtm.mul_(mu).add_(grad, alpha=1-damp)`."""
  k, d, device = gars._validate(list(ys))
  gars._validate(list(xs) + [ys[0]])
  if len(xs) != k:
    raise gars.GarInputError("multi_axpby needs as many x as y vectors")
  lib = _lib.load()
  gars.invalidate_rank_cache()
  with torch.cuda.device(device):
    _lib.check(lib.bm_multi_axpby(_lib.pointer_table(ys), _lib.pointer_table(xs), k, d,
                                  ctypes.c_float(a), ctypes.c_float(b), gars._stream(device)),
               "bm_multi_axpby")


def momentum_stats(sampled, buffers, mu, one_minus_damp, clip_factors_dev=None, attack_scale=None, attack="empire",
                   direction=False):
  """First pass of a step in one kernel (attack.py:791-804,846-847 and attacks/identical.py:63-86):
  worker momentum in place on `buffers` (which then ARE the honest gradients), statistics of the
  sampled stack and of the honest stack, and the Byzantine vector of an "identical" attack.

  Returns (sampled_avg, honest_avg, byz or None, out6) with out6 a device fp64 tensor
  [sum avg_s^2, sum_i |s_i-avg_s|^2, max|avg_s|, sum avg_h^2, sum_i |b_i-avg_h|^2, max|avg_h|]. No sync.
  """
  ks, d, device = gars._validate(list(sampled))
  h = gars._validate(list(buffers) + [sampled[0]])[0] - 1
  if h < 1 or ks < h:
    raise gars.GarInputError("momentum_stats needs 1 <= len(buffers) <= len(sampled)")
  lib = _lib.load()
  s_avg = torch.empty(d, dtype=torch.float32, device=device)
  h_avg = torch.empty(d, dtype=torch.float32, device=device)
  byz = torch.empty(d, dtype=torch.float32, device=device) if attack_scale is not None else None
  out6 = torch.empty(6, dtype=torch.float64, device=device)
  ws = gars._workspace(device, _lib.WS_STEP, 1, d, "ws_step")
  gars.invalidate_rank_cache()
  with torch.cuda.device(device):
    _lib.check(lib.bm_momentum_stats(
      _lib.pointer_table(sampled), ks, _lib.pointer_table(buffers), h, d, ctypes.c_float(mu),
      ctypes.c_float(one_minus_damp), _opt(clip_factors_dev), _ptr(s_avg), _ptr(h_avg), _opt(byz),
      ctypes.c_float(attack_scale if attack_scale is not None else 0.0),
      _attack_id(attack, direction), _ptr(out6), _ptr(ws),
      gars._stream(device)), "bm_momentum_stats")
  return s_avg, h_avg, byz, out6


def momentum_stats_colwise(sampled, buffers, mu, one_minus_damp, clip_factors_dev, attack_scale, attack, rule, f, n_byz):
  """momentum_stats followed by a coordinate-wise rule over the updated buffers and `n_byz` copies of the Byzantine
  vector — for the four rules over 20 buffers and 5 copies, or 14 buffers and 11 copies, INSIDE the same kernel; any
  other shape runs the two kernels, same results (bm_momentum_stats_colwise).  Returns (sampled_avg, honest_avg, byz, defense, out6). No sync."""
  ks, d, device = gars._validate(list(sampled))
  h = gars._validate(list(buffers) + [sampled[0]])[0] - 1
  if h < 1 or ks < h or n_byz < 1:
    raise gars.GarInputError("momentum_stats_colwise needs 1 <= len(buffers) <= len(sampled) and n_byz >= 1")
  lib = _lib.load()
  s_avg, h_avg, byz, defense = (torch.empty(d, dtype=torch.float32, device=device) for _ in range(4))
  out6 = torch.empty(6, dtype=torch.float64, device=device)
  ws = gars._workspace(device, _lib.WS_STEP, 1, d, "ws_step")
  gars.invalidate_rank_cache()
  with torch.cuda.device(device):
    _lib.check(lib.bm_momentum_stats_colwise(
      _lib.pointer_table(sampled), ks, _lib.pointer_table(buffers), h, d, ctypes.c_float(mu),
      ctypes.c_float(one_minus_damp), _opt(clip_factors_dev),
      _ptr(s_avg), _ptr(h_avg), _ptr(byz), ctypes.c_float(attack_scale), _attack_id(attack, False),
      _EVAL_OPS[rule], int(f), int(n_byz), _ptr(defense), _ptr(out6), _ptr(ws), gars._stream(device)),
      "bm_momentum_stats_colwise")
  return s_avg, h_avg, byz, defense, out6


def momentum_stats_sqdist(sampled, buffers, mu, one_minus_damp, clip_factors_dev, attack_scale, attack, n_byz,
                          d_total=None):
  """momentum_stats together with the n x n squared distances (n = len(buffers) + n_byz) of the updated buffers and
  the Byzantine copies — contracted inside the same kernel at ks = h = 20 for long gradients
  (bm_momentum_stats_sqdist).  Returns (sampled_avg, honest_avg, byz, sq, out6). No sync."""
  ks, d, device = gars._validate(list(sampled))
  h = gars._validate(list(buffers) + [sampled[0]])[0] - 1
  if h < 1 or ks < h or n_byz < 1 or h + n_byz > _lib.MAX_ROWS:
    raise gars.GarInputError("momentum_stats_sqdist needs 1 <= len(buffers) <= len(sampled), n_byz >= 1, at most 64 rows")
  n = h + n_byz
  lib = _lib.load()
  s_avg, h_avg, byz = (torch.empty(d, dtype=torch.float32, device=device) for _ in range(3))
  sq = torch.empty((n, n), dtype=torch.float64, device=device)
  out6 = torch.empty(6, dtype=torch.float64, device=device)
  ws = gars._workspace(device, _lib.WS_STEP, 1, d, "ws_step")
  ws_pair = gars._workspace(device, _lib.WS_PAIRWISE, n, d, "ws_pair")
  gars.invalidate_rank_cache()
  with torch.cuda.device(device):
    _lib.check(lib.bm_momentum_stats_sqdist(
      _lib.pointer_table(sampled), ks, _lib.pointer_table(buffers), h, d, d if d_total is None else int(d_total),
      ctypes.c_float(mu), ctypes.c_float(one_minus_damp), _opt(clip_factors_dev), _ptr(s_avg), _ptr(h_avg), _ptr(byz),
      ctypes.c_float(attack_scale), _attack_id(attack, False), int(n_byz), _ptr(sq), _ptr(out6), _ptr(ws), _ptr(ws_pair),
      gars._stream(device)), "bm_momentum_stats_sqdist")
  return s_avg, h_avg, byz, sq, out6


def stack_stats_colwise(rows, attack_scale, attack, rule, f, n_byz):
  """stack_stats (average, Byzantine vector, statistics) followed by a coordinate-wise rule over the rows and `n_byz`
  copies of the Byzantine vector — ONE pass over the rows at k = 20 (5 copies) or 14 (11 copies)
  (bm_stack_stats_colwise: the honest rows of `--momentum-at update`).  Returns (avg, byz, defense, out6). No sync."""
  k, d, device = gars._validate(list(rows))
  if n_byz < 1:
    raise gars.GarInputError("stack_stats_colwise needs n_byz >= 1")
  lib = _lib.load()
  avg, byz, defense = (torch.empty(d, dtype=torch.float32, device=device) for _ in range(3))
  out6 = torch.empty(6, dtype=torch.float64, device=device)
  ws = gars._workspace(device, _lib.WS_STEP, 1, d, "ws_step")
  with torch.cuda.device(device):
    _lib.check(lib.bm_stack_stats_colwise(_lib.pointer_table(rows), k, d, _ptr(avg), _ptr(byz),
                                          ctypes.c_float(attack_scale), _attack_id(attack, False), _EVAL_OPS[rule],
                                          int(f), int(n_byz), _ptr(defense), _ptr(out6), _ptr(ws),
                                          gars._stream(device)), "bm_stack_stats_colwise")
  return avg, byz, defense, out6


def stack_stats_sqdist(rows, attack_scale, attack, n_byz, d_total=None):
  """stack_stats together with the n x n squared distances (n = len(rows) + n_byz) of the rows and the Byzantine
  copies, in one pass at k = 20 / 14 for long gradients (bm_stack_stats_sqdist).  Returns (avg, byz, sq, out6)."""
  k, d, device = gars._validate(list(rows))
  if n_byz < 1 or k + n_byz > _lib.MAX_ROWS:
    raise gars.GarInputError("stack_stats_sqdist needs n_byz >= 1 and at most 64 rows")
  n = k + n_byz
  lib = _lib.load()
  avg, byz = (torch.empty(d, dtype=torch.float32, device=device) for _ in range(2))
  sq = torch.empty((n, n), dtype=torch.float64, device=device)
  out6 = torch.empty(6, dtype=torch.float64, device=device)
  ws = gars._workspace(device, _lib.WS_STEP, 1, d, "ws_step")
  ws_pair = gars._workspace(device, _lib.WS_PAIRWISE, n, d, "ws_pair")
  with torch.cuda.device(device):
    _lib.check(lib.bm_stack_stats_sqdist(_lib.pointer_table(rows), k, d, d if d_total is None else int(d_total),
                                         _ptr(avg), _ptr(byz), ctypes.c_float(attack_scale), _attack_id(attack, False),
                                         int(n_byz), _ptr(sq), _ptr(out6), _ptr(ws), _ptr(ws_pair),
                                         gars._stream(device)), "bm_stack_stats_sqdist")
  return avg, byz, sq, out6


def multi_fma3(outs, ps, qs, a, b, p_scale_dev=None):
  """out_i = b*q_i + a*(p_scale_i*p_i) for every triple (outs may alias ps; qs may repeat one tensor):
  worker / server / update momentum and the Nesterov look-ahead of attack.py:757-810,832-839.
  b: a number, or a DEVICE float64 tensor whose first element is read by the kernel (bm_multi_fma3_bdev: the factor
  attack_search_device left on the device — no host round trip)."""
  outs, ps, qs = list(outs), list(ps), list(qs)
  k, d, device = gars._validate(outs)
  gars._validate(ps + [outs[0]])
  gars._validate(qs + [outs[0]])
  if len(ps) != k or len(qs) != k:
    raise gars.GarInputError("multi_fma3 needs as many p and q as out vectors")
  lib = _lib.load()
  gars.invalidate_rank_cache()
  scale = _opt(p_scale_dev)
  with torch.cuda.device(device):
    if isinstance(b, torch.Tensor):
      _require_scalar_on(b, device, "multi_fma3: a tensor b must be a contiguous float64 tensor on the vectors' device")
      _lib.check(lib.bm_multi_fma3_bdev(_lib.pointer_table(outs), _lib.pointer_table(ps), _lib.pointer_table(qs), k, d,
                                        ctypes.c_float(a), _ptr(b), scale, gars._stream(device)), "bm_multi_fma3_bdev")
    else:
      _lib.check(lib.bm_multi_fma3(_lib.pointer_table(outs), _lib.pointer_table(ps), _lib.pointer_table(qs), k, d,
                                   ctypes.c_float(a), ctypes.c_float(b), scale, gars._stream(device)), "bm_multi_fma3")


DEVICE_SEARCH_RULES = ("krum", "average")


def attack_search_device(ext, h, k, f, rule, evals=16, negative=False, m=None):
  """The factor search of attacks/identical.py:67-77 on the device (bm_attack_line_search_device) from the DEVICE
  (h+2) x (h+2) squared distances among honests + [avg, avg + att]: a float64 device tensor of 1 + 2 * evals values —
  [0] the factor, then (abscissa, objective) per evaluation — with the candidates and the bits of
  linesearch.attack_line_search.  Nothing is copied or awaited: hand `out[:1]` to multi_fma3 as b."""
  if rule not in DEVICE_SEARCH_RULES:
    raise ValueError(f"no device form of the search for rule {rule!r}")
  _require_ext(ext, h)
  if not isinstance(evals, int) or evals < 1:
    _lib.check(_lib.EINVAL, "attack_search_device (evals must be a positive integer)")
  lib = _lib.load()
  # (BM_SEARCH_TRACE=1, measurement only: the kernel appends 24 phase timestamps per candidate behind the results; the
  # library looks at the value's first character, search_device.hip, so the room is made on the same predicate)
  extra = 24 * evals if os.environ.get("BM_SEARCH_TRACE", "")[:1] == "1" else 0
  out = torch.zeros(1 + 2 * evals + extra, dtype=torch.float64, device=ext.device) if extra else \
      torch.empty(1 + 2 * evals, dtype=torch.float64, device=ext.device)
  with torch.cuda.device(ext.device):
    _lib.check(lib.bm_attack_line_search_device(_ptr(ext), h, k, f, _lib.RULE_IDS[rule], m or 0, evals,
                                                1 if negative else 0, _ptr(out), gars._stream(ext.device)),
               "bm_attack_line_search_device")
  return out


def attack_ranking_device(ext, h, k, f, mode, t_dev, m=None):
  """linesearch.attack_ranking on the device (bm_attack_ranking_device): the ranking of honests + [avg + t*att] * k as a
  device int32[64] tensor (the n rows by rank, then zeros) from the DEVICE (h+2) x (h+2) matrix and a factor in DEVICE
  memory (float64[1]) — what bm_bulyan_pass2 / bm_bulyan_pass2_eval take as `order`.  Nothing is copied or awaited."""
  _require_ext(ext, h)
  _require_scalar_on(t_dev, ext.device, "attack_ranking_device: the factor must be a contiguous float64 tensor on the matrix's device")
  lib = _lib.load()
  order = torch.empty(_lib.MAX_ROWS, dtype=torch.int32, device=ext.device)
  mode_id = {"krum": _lib.RANK_KRUM, "bulyan": _lib.RANK_BULYAN}[mode]
  with torch.cuda.device(ext.device):
    _lib.check(lib.bm_attack_ranking_device(_ptr(ext), h, k, f, mode_id, m or 0, _ptr(t_dev), _ptr(order),
                                            gars._stream(ext.device)), "bm_attack_ranking_device")
  return order


def clip_factors_from_sq(sq, k, clip):
  """Device float32 factors from a device fp64 tensor of k squared norms (possibly all-reduced)."""
  lib = _lib.load()
  device = sq.device
  if not sq.is_contiguous():
    sq = sq.contiguous()
  factors = torch.empty(_lib.MAX_ROWS, dtype=torch.float32, device=device)
  with torch.cuda.device(device):
    _lib.check(lib.bm_clip_factors(_ptr(sq), k, ctypes.c_float(clip), _ptr(factors), gars._stream(device)),
               "bm_clip_factors")
  return factors


def clip_factors(gradients, clip):
  """Device float32[k]: clip/||g_i|| where ||g_i|| > clip, else 1 (attack.py:791-794). No sync."""
  k, d, device = gars._validate(gradients)
  return clip_factors_from_sq(row_sqnorms(gradients), k, clip)


def multi_scale(ys, factors_dev):
  """y_i *= factors[i] in place; rows whose factor is exactly 1 are not touched."""
  ys = list(ys)
  k, d, device = gars._validate(ys)
  lib = _lib.load()
  gars.invalidate_rank_cache()
  with torch.cuda.device(device):
    _lib.check(lib.bm_multi_scale(_lib.pointer_table(ys), k, d, _ptr(factors_dev), gars._stream(device)),
               "bm_multi_scale")


def clip_gradients(gradients, clip):
  """In-place gradient clipping of attack.py:776-779,791-794 for a whole list, without a host sync."""
  factors = clip_factors(gradients, clip)
  multi_scale(gradients, factors)
  return factors


def l2_distance(a, b):
  """||a - b||_2 as a device fp64 scalar tensor (attack.py:830 `l2_origin`), no sync.  Two rows through
  the centred pairwise kernel: the centre is row 0, so the contraction sees a - b itself (no cancellation)."""
  return gars.pairwise_sqdist([a, b])[0, 1].sqrt()


def step_worker(comm, sampled, buffers, n, f_decl, f_real, rule, m, mu, one_minus_damp, clip, attack, attack_scale,
                nb_past, past_count, past_newest, curv, past_oldest, params=None, origin=None, d_total=None):
  """One simulation step with worker-side momentum as ONE C call (bm_step_worker, include/bm_gar.h).

  comm: sharded.NativeComm or None; d_total: length of the whole vectors over all shards (default: this shard's).
  Returns (defense, sampled_avg, honest_avg, byz, stats) with `stats` the
  device fp64 vector documented in the header (already reduced over the ranks). No sync."""
  ks, d, device = gars._validate(list(sampled))
  lib = _lib.load()
  new = lambda: torch.empty(d, dtype=torch.float32, device=device)  # noqa: E731
  defense, s_avg, h_avg = new(), new(), new()
  byz = new() if f_real > 0 else None  # (the attack average is not materialised: attack_avg_out = NULL)
  stats = torch.empty(lib.bm_step_stats_count(), dtype=torch.float64, device=device)
  ws = gars._Scratch.get(device, "ws_stepcall", nbytes=int(lib.bm_step_workspace_bytes(n, d)))
  par = _lib.StepParams(n=n, f_decl=f_decl, f_real=f_real, ks=ks, rule=_lib.RULE_IDS[rule], m=m or 0,
                        attack_kind=_lib.ATTACK_LITTLE if attack == "little" else _lib.ATTACK_EMPIRE, nb_past=nb_past,
                        past_count=past_count, attack_scale=attack_scale, mu=mu, one_minus_damp=one_minus_damp,
                        clip=clip if clip is not None else 0.0,
                        oldest_weight=-(mu ** (nb_past - 1)) if nb_past > 0 else 0.0)
  gars.invalidate_rank_cache()
  with torch.cuda.device(device):
    _lib.check(lib.bm_step_worker(comm.handle if comm is not None else None, ctypes.byref(par),
                                  _lib.pointer_table(sampled), _lib.pointer_table(buffers), d,
                                  int(d_total) if d_total is not None else d, _ptr(defense),
                                  _ptr(s_avg), _ptr(h_avg), _opt(byz), None, _opt(past_newest), _opt(curv),
                                  _opt(past_oldest), _opt(params), _opt(origin), _ptr(stats), _ptr(ws),
                                  gars._stream(device)), "bm_step_worker")
  return defense, s_avg, h_avg, byz, stats
