"""Host side of the gradient aggregation rules: argument plumbing around libbm_gar.so.

Mirrors the reference's plugin surface (aggregators/__init__.py:15-31): every rule takes a
Python `list` of n flat fp32 tensors living on one GPU (entries may alias) plus `f`, returns a
NEW tensor, never touches its inputs, and runs asynchronously on the caller's current stream.
All arithmetic happens in the HIP kernels; nothing here falls back to torch ops or to the CPU
oracle — on a machine without the library or without a GPU these functions raise.

Reference semantics, per rule:
  median   aggregators/median.py:31-39      trmean/phocas/meamed  aggregators/trmean.py:24-109
  krum     aggregators/krum.py:31-80        bulyan                aggregators/bulyan.py:31-84
  brute    aggregators/brute.py:32-80       aksel                 aggregators/aksel.py:24-64
  average  aggregators/average.py:21-29     cge                   aggregators/cge.py:28-57
"""

import ctypes
import weakref

import torch

from . import _lib, pipelines
from .pipelines import (BRUTE_NO_SUBSET, FORMS, NNM_RULES, SCALAR_RULES, GarInputError,  # noqa: F401  (theirs, kept here)
                        check_center_args, check_spectral_args)

__all__ = ["median", "trmean", "phocas", "meamed", "krum", "bulyan", "brute", "aksel", "average", "cge",
           "krum_selection", "bulyan_ranking", "brute_selection", "aksel_selection", "cge_selection",
           "pairwise_sqdist", "rank_from_sqdist", "selected_mean", "bulyan_pass2", "aksel_sqdist",
           "stable_argsort", "GarInputError", "geomed", "cclip", "center_weights", "weighted_sum",
           "nnm", "bucketing", "nnm_masks", "mix_rows", "nnm_rows", "colwise_mixed", "bucket_masks", "NNM_RULES",
           "mixed_sqdist", "mix_weights", "SCALAR_RULES", "caf", "dnc", "spectral_weights", "bucket_permutation",
           "bucket_masks_host", "bucket_masks_device", "colwise_bucketed", "colwise_bucketed_supported"]


# ---------------------------------------------------------------------------- #
# Input validation and scratch memory

def _validate(gradients):
  if not isinstance(gradients, (list, tuple)) or len(gradients) < 1:
    raise GarInputError(f"expected a non-empty list of gradients, got {type(gradients).__name__}")
  n = len(gradients)
  if n > _lib.MAX_ROWS:
    raise GarInputError(f"at most {_lib.MAX_ROWS} gradients are supported, got {n}")
  g0 = gradients[0]
  if not isinstance(g0, torch.Tensor):
    raise GarInputError("gradients must be torch tensors")
  if not g0.is_cuda:
    raise GarInputError(
      "the MI355X aggregation path needs gradients on a GPU (device 'cuda:N'); there is no CPU fallback")
  for g in gradients:
    if (g.device != g0.device or g.dtype != torch.float32 or g.dim() != 1 or g.shape != g0.shape
        or not g.is_contiguous()):
      raise GarInputError("gradients must be contiguous 1-D float32 tensors of equal length on one device")
  return n, g0.shape[0], g0.device


def _stream(device):
  return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class _Scratch:
  """Per-(device, stream) scratch tensors. The C library owns nothing; this is the caller side."""
  _cache = {}

  @classmethod
  def get(cls, device, name, nbytes=None, shape=None, dtype=torch.uint8):
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, name)
    buf = cls._cache.get(key)
    want = (nbytes,) if shape is None else tuple(shape)
    if buf is None or buf.dtype != dtype or tuple(buf.shape) != want:
      buf = torch.empty(want, dtype=dtype, device=device)
      cls._cache[key] = buf
    return buf


def _workspace(device, kind, n, d, name):
  nbytes = _lib.load().bm_workspace_bytes(kind, n, d)
  if nbytes < 0:
    raise RuntimeError(f"bm_workspace_bytes({kind}, {n}, {d}) failed")
  return _Scratch.get(device, name, nbytes=int(nbytes))


def _ptr(t):
  return ctypes.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------- #
# Coordinate-wise rules

def _colwise(op, gradients, f):
  n, d, device = _validate(gradients)
  lib = _lib.load()
  out = torch.empty(d, dtype=torch.float32, device=device)
  if d == 0:
    return out
  with torch.cuda.device(device):
    _lib.check(lib.bm_colwise(op, _lib.pointer_table(gradients), n, d, f, _ptr(out), _stream(device)),
               "bm_colwise")
  return out


def median(gradients, **kwargs):
  """Coordinate-wise lower median (aggregators/median.py:31-39)."""
  return _colwise(_lib.OP_MEDIAN, gradients, 0)


def trmean(gradients, f, **kwargs):
  """Coordinate-wise trimmed mean of sorted ranks f..n-f-1 (aggregators/trmean.py:69-79)."""
  return _colwise(_lib.OP_TRMEAN, gradients, f)


def phocas(gradients, f, **kwargs):
  """Mean of the n-f values closest to the trimmed mean (aggregators/trmean.py:81-94)."""
  return _colwise(_lib.OP_PHOCAS, gradients, f)


def meamed(gradients, f, **kwargs):
  """Mean of the n-f values closest to the median (aggregators/trmean.py:96-109)."""
  return _colwise(_lib.OP_MEAMED, gradients, f)


# ---------------------------------------------------------------------------- #
# Distance-based rules

def pairwise_sqdist(gradients, d_total=None):
  """n x n fp64 matrix of squared L2 distances, on the device, no host sync.  d_total: length of the whole
  vectors when `gradients` are one shard of a dimension-partitioned stack (the precision plan follows it)."""
  n, d, device = _validate(gradients)
  lib = _lib.load()
  sq = torch.empty((n, n), dtype=torch.float64, device=device)  # result: a fresh tensor per call
  ws = _workspace(device, _lib.WS_PAIRWISE, n, d, "ws_pair")
  with torch.cuda.device(device):
    _lib.check(lib.bm_pairwise_sqdist_shard(_lib.pointer_table(gradients), n, d, d if d_total is None else int(d_total),
                                            _ptr(sq), _ptr(ws), _stream(device)), "bm_pairwise_sqdist_shard")
  return sq


def rank_from_sqdist(sq, n, f, m, mode):
  """Scores + stable order from an n x n squared-distance matrix that is already on the device
  (possibly the all-reduced sum of per-shard partial matrices). Returns (order, scores)."""
  device = sq.device
  lib = _lib.load()
  order = torch.empty(_lib.MAX_ROWS, dtype=torch.int32, device=device)
  scores = torch.empty(_lib.MAX_ROWS, dtype=torch.float64, device=device)
  with torch.cuda.device(device):
    _lib.check(lib.bm_krum_rank(_ptr(sq), n, f, m, mode, _ptr(order), _ptr(scores), _stream(device)),
               "bm_krum_rank")
  return order, scores


def _rank(gradients, f, m, mode):
  """Distances -> scores -> stable order, all on the device, in the distance pass's own launches (bm_pairwise_rank:
  its last workgroups rank the rows).  Returns (order int32[MAX_ROWS], scores f64[MAX_ROWS])."""
  n, d, device = _validate(gradients)
  lib = _lib.load()
  sq = torch.empty((n, n), dtype=torch.float64, device=device)
  order = torch.empty(_lib.MAX_ROWS, dtype=torch.int32, device=device)
  scores = torch.empty(_lib.MAX_ROWS, dtype=torch.float64, device=device)
  ws = _workspace(device, _lib.WS_PAIRWISE, n, d, "ws_pair")
  with torch.cuda.device(device):
    _lib.check(lib.bm_pairwise_rank(_lib.pointer_table(gradients), n, d, d, f, m, mode, _ptr(sq), _ptr(order),
                                    _ptr(scores), _ptr(ws), _stream(device)), "bm_pairwise_rank")
  return order, scores


def selected_mean(gradients, idx, m):
  """Sequential fp32 mean of gradients[idx[0..m)], idx being a DEVICE int32 tensor."""
  n, d, device = _validate(gradients)
  lib = _lib.load()
  out = torch.empty(d, dtype=torch.float32, device=device)
  if d == 0:
    return out
  with torch.cuda.device(device):
    _lib.check(lib.bm_selected_mean(_lib.pointer_table(gradients), n, _ptr(idx), m, d, _ptr(out),
                                    _stream(device)), "bm_selected_mean")
  return out


# Last ranking per rule, so that `influence` right after `aggregate` (attack.py:821-822) does not
# recompute the distance matrix.  An entry is only reused for the SAME tensor objects (weak
# references: a freed gradient can never alias a new one) at the same in-place version.
_last_rank = {}


def invalidate_rank_cache():
  """Forget cached rankings; called by every routine of this package that writes user tensors."""
  _last_rank.clear()


def _rank_cache_get(tag, gradients, params):
  hit = _last_rank.get(tag)
  if hit is None or hit[0] != params or len(hit[1]) != len(gradients):
    return None
  for (ref, version), g in zip(hit[1], gradients):
    if ref() is not g or g._version != version:
      return None
  return hit[2]


def _rank_cache_put(tag, gradients, params, order):
  _last_rank[tag] = (params, [(weakref.ref(g), g._version) for g in gradients], order)


def _cached_rank(tag, gradients, f, m, mode):
  order = _rank_cache_get(tag, gradients, (f, m))
  if order is None:
    order, _ = _rank(gradients, f, m, mode)
    _rank_cache_put(tag, gradients, (f, m), order)
  return order


def krum(gradients, f, m=None, **kwargs):
  """Multi-Krum (aggregators/krum.py:65-80): mean, in score order, of the m best-scored rows."""
  n = len(gradients)
  if m is None:
    m = n - f - 2
  order = _cached_rank("krum", gradients, f, m, _lib.RANK_KRUM)
  return selected_mean(gradients, order, m)


def krum_selection(gradients, f, m=None, **kwargs):
  """Indices (score order) of the m rows Multi-Krum averages — host list, synchronises."""
  n = len(gradients)
  if m is None:
    m = n - f - 2
  order = _cached_rank("krum", gradients, f, m, _lib.RANK_KRUM)
  return order[:m].tolist()


def bulyan_ranking(gradients, f, m=None, **kwargs):
  """Initial stable score order used by every Bulyan iteration — host list, synchronises."""
  n = len(gradients)
  if m is None:
    m = n - f - 2
  order = _cached_rank("bulyan", gradients, f, m, _lib.RANK_BULYAN)
  return order[:n].tolist()


def bulyan_pass2(gradients, order, f, m):
  """Second pass of Bulyan given the device-resident ranking (aggregators/bulyan.py:64-84)."""
  n, d, device = _validate(gradients)
  lib = _lib.load()
  out = torch.empty(d, dtype=torch.float32, device=device)
  if d == 0:
    return out
  with torch.cuda.device(device):
    _lib.check(lib.bm_bulyan_pass2(_lib.pointer_table(gradients), n, _ptr(order), f, m, d, _ptr(out), _stream(device)),
               "bm_bulyan_pass2")
  return out


def bulyan(gradients, f, m=None, **kwargs):
  """Bulyan over Multi-Krum (aggregators/bulyan.py:31-84)."""
  n = len(gradients)
  if m is None:
    m = n - f - 2
  order = _cached_rank("bulyan", gradients, f, m, _lib.RANK_BULYAN)
  return bulyan_pass2(gradients, order, f, m)


def brute_select_host(dist_host, n, f):
  """Subset search of the Brute rule on a HOST fp64 n x n distance matrix (aggregators/brute.py:47-68)."""
  lib = _lib.load()
  sel = (ctypes.c_int32 * (n - f))()
  rc = lib.bm_brute_select(ctypes.c_void_p(dist_host.data_ptr()), n, f, ctypes.cast(sel, ctypes.c_void_p))
  if rc != 0:
    raise RuntimeError("brute: too many non-finite gradients, no subset of n-f rows has a finite diameter")
  return list(sel)


def brute_select_device(sq, n, f):
  """Subset search of the Brute rule on a DEVICE fp64 n x n matrix of SQUARED distances (bm_brute_select_device: one
  workgroup, no host round trip).  Returns (sel int32[MAX_ROWS]: the n - f rows ascending, status int32[1]: 0, -1 when
  every subset touches a non-finite distance, -2 when the search gave up on its node budget), both on the device."""
  lib = _lib.load()
  device = sq.device
  sel = torch.empty(_lib.MAX_ROWS, dtype=torch.int32, device=device)
  status = torch.empty(1, dtype=torch.int32, device=device)
  with torch.cuda.device(device):
    _lib.check(lib.bm_brute_select_device(_ptr(sq), n, f, _ptr(sel), _ptr(status), _stream(device)),
               "bm_brute_select_device")
  return sel, status


def _brute_sel(gradients, f):
  """(sel, status) of the stack, from the cache when `influence` follows `aggregate` on the same tensors
  (attack.py:821-822): the distance pass is then not repeated."""
  hit = _rank_cache_get("brute", gradients, (f,))
  if hit is None:
    n, d, device = _validate(gradients)
    # brute keeps non-finite distances as they are and skips the subsets that contain one (brute.py:45,56-57)
    hit = brute_select_device(pairwise_sqdist(gradients), n, f)
    _rank_cache_put("brute", gradients, (f,), hit)
  return hit


def brute_selection(gradients, f, **kwargs):
  """Index set (ascending) of the n-f rows of smallest diameter (aggregators/brute.py:32-68) — host list,
  synchronises; raises when no subset of n-f rows has a finite diameter (the reference then has no selection)."""
  sel, _ = _brute_resolved(gradients, f, *_brute_sel(gradients, f), True)
  return sel[:len(gradients) - f].tolist()


BRUTE_BUDGET = ("brute: the device search gave up after its budget of search-tree nodes (csrc/brute.hip; a distance matrix "
                "built against the search?) — gars.brute_select_host on the host has no such limit")
# (convenience only: the status of the latest brute() of this PROCESS, whatever its device or stream; the status of a
#  given call travels with its result, `result.brute_status`, and that is what callers with several devices, streams
#  or aggregators must read — ShardedAggregator keeps its own)
last_brute_status = None


def brute_check(status=None):
  """Raise when the given Brute search (default: the latest one of this process) found no admissible subset — the
  reference's assertion (brute.py:68) — or gave up on its node budget.  Synchronises (one 4-byte read); not to be
  called while a stream is being captured."""
  status = last_brute_status if status is None else status
  code = 0 if status is None else int(status.item())
  if code == -2:
    raise RuntimeError(BRUTE_BUDGET)
  if code != 0:
    raise RuntimeError(BRUTE_NO_SUBSET)


def brute_host_selection(gradients, f, sq=None):
  """The selection of the Brute rule by the HOST search (bm_brute_select: no node budget), as a device index tensor;
  one synchronisation.  What the checked paths fall back to when the device search reports status -2 — the reference
  would keep computing (brute.py:47-68), so does this."""
  n, d, device = _validate(gradients)
  if sq is None:
    sq = pairwise_sqdist(gradients)
  return _legs.host_selection(sq, n, f, gradients[0])


def _brute_resolved(gradients, f, sel, status, check):
  """The (sel, status) of _brute_sel through the status protocol (pipelines.brute_resolve); a host re-search replaces
  the cache entry, its status a zero."""
  sel, status = pipelines.brute_resolve(sel, status, None, len(gradients), f, check,
                                        lambda *_: brute_host_selection(gradients, f))
  if status is None:
    status = torch.zeros(1, dtype=torch.int32, device=sel.device)
    _rank_cache_put("brute", gradients, (f,), (sel, status))
  return sel, status


def brute(gradients, f, check=False, **kwargs):
  """Brute rule (aggregators/brute.py:70-80): mean of the minimum-diameter subset, index order.  Distances, subset
  search and average all run on the device, on the caller's stream: no host synchronisation (graph-capturable).
  The search's status (device int32[1]) travels with the result as `result.brute_status`:
    -1  no subset of n-f rows has a finite diameter — more than f gradients with non-finite coordinates, where the
        reference fails its assertion (brute.py:56-57,68): the result is the average of n-f copies of one bad
        gradient, i.e. non-finite where that gradient is;
    -2  the device search gave up on its budget of search-tree nodes: the result is NaN EVERYWHERE (the index table
        then holds -1, which the averaging kernel answers with NaN) — never an average of some rows.
  check=True (what the `native-brute` plugin passes) reads the status, at the price of one host synchronisation,
  unless the stream is being captured into a graph: -1 raises like the reference, -2 falls back to the host search,
  which has no budget, and returns ITS average — the reference would have kept computing."""
  global last_brute_status
  n, d, device = _validate(gradients)
  sel, status = _brute_sel(gradients, f)
  last_brute_status = status  # (what a refusal below leaves behind)
  sel, last_brute_status = _brute_resolved(gradients, f, sel, status, check)
  out = selected_mean(gradients, sel, n - f)
  out.brute_status = last_brute_status
  return out


def aksel_sqdist(gradients):
  """fp64[n] squared distances of every row to the coordinate-wise median (device, no sync)."""
  n, d, device = _validate(gradients)
  lib = _lib.load()
  sq = torch.empty(_lib.MAX_ROWS, dtype=torch.float64, device=device)
  ws = _workspace(device, _lib.WS_AKSEL, n, d, "ws_aksel")
  with torch.cuda.device(device):
    _lib.check(lib.bm_aksel_pass1(_lib.pointer_table(gradients), n, d, None, _ptr(sq), _ptr(ws),
                                  _stream(device)), "bm_aksel_pass1")
  return sq


def stable_argsort(keys, n):
  """Device-side stable argsort of the first n fp64 keys (NaN last). Returns int32[MAX_ROWS]."""
  device = keys.device
  lib = _lib.load()
  order = torch.empty(_lib.MAX_ROWS, dtype=torch.int32, device=device)
  with torch.cuda.device(device):
    _lib.check(lib.bm_stable_argsort(_ptr(keys), n, _ptr(order), _stream(device)), "bm_stable_argsort")
  return order


def _aksel_order(gradients):
  order = _rank_cache_get("aksel", gradients, ())
  if order is None:
    order = stable_argsort(aksel_sqdist(gradients), len(gradients))
    _rank_cache_put("aksel", gradients, (), order)
  return order


def _aksel_count(n, f, mode):
  if mode == "mid":
    return (n + 1) // 2
  if mode == "n-f":
    return n - f
  raise NotImplementedError(f"aksel mode {mode!r}")


def aksel_selection(gradients, f, mode="mid", **kwargs):
  c = _aksel_count(len(gradients), f, mode)
  return _aksel_order(gradients)[:c].tolist()


def aksel(gradients, f, mode="mid", **kwargs):
  """Aksel (aggregators/aksel.py:52-64): mean of the c rows closest to the coordinate-wise median."""
  c = _aksel_count(len(gradients), f, mode)
  return selected_mean(gradients, _aksel_order(gradients), c)


def average(gradients, **kwargs):
  """Arithmetic mean (aggregators/average.py:21-29), same sequential summation order."""
  n, d, device = _validate(gradients)
  idx = torch.arange(n, dtype=torch.int32, device=device)
  return selected_mean(gradients, idx, n)


# ---------------------------------------------------------------------------- #
# Geometric median and centered clipping: one distance pass, the iteration on scalars, one weighted sum

def center_weights(sq, n, mode, param, iters, tol=0.0, has_start=False):
  """The weights of the geometric median ("geomed", param = nu) or of centered clipping ("cclip", param = tau) from the
  N x N squared distances of the n rows (+ the start vector as point n when has_start), N = n + has_start <= 64 — the
  iteration of include/bm_gar.h (bm_center_weights) on scalars.  `sq` on the device (where pairwise_sqdist left it,
  possibly all-reduced): one workgroup, no copy, no synchronisation; `sq` on the host: the host form, same bits.
  Returns (weights fp64[MAX_ROWS]: the N weights then zeros, info fp64[3]: iterations run, move^2, usable rows), where
  `sq` lives."""
  check_center_args(mode, param, iters, tol)
  N = int(n) + (1 if has_start else 0)
  if n < 1 or N > _lib.MAX_ROWS:
    raise GarInputError(f"{mode}: at most {_lib.MAX_ROWS} points (rows + start vector) are supported, got {N}")
  if sq.dtype != torch.float64 or sq.numel() < N * N or not sq.is_contiguous():
    raise GarInputError(f"{mode}: expected a contiguous float64 matrix of {N} x {N} squared distances")
  lib = _lib.load()
  weights = torch.empty(_lib.MAX_ROWS, dtype=torch.float64, device=sq.device)
  info = torch.empty(3, dtype=torch.float64, device=sq.device)
  args = (_ptr(sq), int(n), 1 if has_start else 0, _lib.CENTER_MODES[mode], float(param), int(iters), float(tol),
          _ptr(weights), _ptr(info))
  if not sq.is_cuda:
    _lib.check(lib.bm_center_weights(*args), "bm_center_weights")
    return weights, info
  with torch.cuda.device(sq.device):
    _lib.check(lib.bm_center_weights_device(*args, _stream(sq.device)), "bm_center_weights_device")
  return weights, info


def weighted_sum(gradients, weights):
  """sum_i float32(weights[i]) * gradients[i], the weights a DEVICE float64 tensor (at least n entries): per coordinate
  one fused multiply-add per active row, in index order.  Aliased gradients are read once with their weights added;
  rows of weight 0 are not read; a NaN weight gives NaN everywhere (bm_weighted_sum)."""
  n, d, device = _validate(gradients)
  if weights.dtype != torch.float64 or weights.device != device or weights.numel() < n or not weights.is_contiguous():
    raise GarInputError(f"weights must be a contiguous float64 tensor of at least {n} entries on {device}")
  lib = _lib.load()
  out = torch.empty(d, dtype=torch.float32, device=device)
  if d == 0:
    return out
  with torch.cuda.device(device):
    _lib.check(lib.bm_weighted_sum(_lib.pointer_table(gradients), n, _ptr(weights), d, _ptr(out), _stream(device)),
               "bm_weighted_sum")
  return out


def _center(mode, gradients, param, iters, tol, start):
  return pipelines.center(_legs, pairwise_sqdist, mode, gradients, param, iters, tol, start)[0]


def geomed(gradients, f=None, nu=1e-6, iters=8, tol=0.0, **kwargs):
  """The geometric median by `iters` smoothed Weiszfeld iterations (RFA) from the mean of the rows:
  v <- sum_i w_i x_i / sum_i w_i, w_i = 1 / max(nu, |x_i - v|).  One distance pass over the n rows, the iteration on the
  n weights (bm_center_weights_device), one weighted sum — whatever `iters` is; no host synchronisation.  `f` is
  accepted and ignored (the registry's calling convention).  n <= 64."""
  return _center("geomed", gradients, nu, iters, tol, None)


def cclip(gradients, f=None, tau=None, iters=3, tol=0.0, start=None, **kwargs):
  """Centered clipping: v <- v + (1/n) sum_i (x_i - v) min(1, tau / |x_i - v|), `iters` times from `start` (a vector like
  the gradients, e.g. the previous aggregate; None: the mean of the rows).  One distance pass over the rows and the
  start, the iteration on scalars, one weighted sum.  `tau` is required; `f` is accepted and ignored.  n <= 64 without a
  start, 63 with one."""
  return _center("cclip", gradients, tau, iters, tol, start)


# ---------------------------------------------------------------------------- #
# Spectral filtering (CAF, DnC): one distance pass, the filter on scalars, one weighted sum

def spectral_weights(sq, n, mode, count, power_iters=16):
  """The weights of CAF ("caf", count = f) or DnC ("dnc", count = k rows to remove) from the n x n squared distances of
  the rows, n <= 64 — the filter of include/bm_gar.h (bm_spectral_weights) on scalars.  `sq` on the device (where
  pairwise_sqdist left it, possibly all-reduced): one workgroup, no copy, no synchronisation; `sq` on the host: the host
  form, same bits.  Returns (weights fp64[MAX_ROWS]: the n weights then zeros, info fp64[4]: evaluations run, the lambda
  of the weights kept, usable rows, the round whose weights were kept or -1), where `sq` lives."""
  n = int(n)
  if not 1 <= n <= _lib.MAX_ROWS:
    raise GarInputError(f"{mode}: at most {_lib.MAX_ROWS} rows are supported, got {n}")
  check_spectral_args(mode, n, count, power_iters)
  if sq.dtype != torch.float64 or sq.numel() < n * n or not sq.is_contiguous():
    raise GarInputError(f"{mode}: expected a contiguous float64 matrix of {n} x {n} squared distances")
  lib = _lib.load()
  weights = torch.empty(_lib.MAX_ROWS, dtype=torch.float64, device=sq.device)
  info = torch.empty(4, dtype=torch.float64, device=sq.device)
  args = (_ptr(sq), n, _lib.SPECTRAL_MODES[mode], int(count), int(power_iters), _ptr(weights), _ptr(info))
  if not sq.is_cuda:
    _lib.check(lib.bm_spectral_weights(*args), "bm_spectral_weights")
    return weights, info
  with torch.cuda.device(sq.device):
    _lib.check(lib.bm_spectral_weights_device(*args, _stream(sq.device)), "bm_spectral_weights_device")
  return weights, info


def _spectral(mode, gradients, count, power_iters):
  out, record = pipelines.spectral(_legs, pairwise_sqdist, mode, gradients, count, power_iters)
  out.spectral_weights, out.spectral_info = record.weights, record.info
  return out


def caf(gradients, f, power_iters=16, **kwargs):
  """CAF, the covariance-bound agnostic filter (Allouah, Guerraoui, Gupta, Rizk, Stephan, NeurIPS 2023): while the
  weights c sum to more than n - 2f, the rows are reweighted c_i <- c_i (1 - tau_i / tau_max), tau_i the squared
  projection of row i (centred on the weighted mean) on the top eigen-direction of the weighted covariance; the output
  is the weighted mean under the weights whose top eigenvalue was smallest.  The eigen-direction comes from
  `power_iters` power steps from the farthest row, a fixed count.  One distance pass, the whole filter on the n x n
  distances (bm_spectral_weights_device), one weighted sum — whatever the rounds; no host synchronisation.  2 f < n <= 64.
  The result carries `.spectral_weights` and `.spectral_info` (device tensors)."""
  return _spectral("caf", gradients, f, power_iters)


def dnc(gradients, f, c=1.0, power_iters=16, **kwargs):
  """DnC, the spectral outlier removal of Shejwalkar & Houmansadr (NDSS 2021) WITHOUT its coordinate sub-sampling and
  its repeated draws (every coordinate is used, once): the k = min(ceil(c f), n - 1) rows of largest squared projection
  on the top eigen-direction of the rows' covariance are removed, the output is the mean of the others.  One distance
  pass, the projections on the n x n distances, one weighted sum; no host synchronisation.  n <= 64.  The result carries
  `.spectral_weights` and `.spectral_info` (device tensors)."""
  return _spectral("dnc", gradients, pipelines.dnc_count(len(gradients), f, c), power_iters)


# ---------------------------------------------------------------------------- #
# Nearest-neighbour mixing and bucketing: one distance pass, the masks on the device, one mixing pass (or none: fused)

def _check_masks(masks, count, where):
  if (not isinstance(masks, torch.Tensor) or masks.dtype != torch.int64 or masks.dim() != 1 or masks.numel() < count
      or not masks.is_contiguous()):
    raise GarInputError(f"{where}: masks must be a contiguous int64 tensor of at least {count} words (bit j of word r: "
                        "row j is averaged into output row r)")


def nnm_masks(sq, n, f):
  """The neighbour masks of nearest-neighbour mixing from the n x n float64 squared distances (bm_nnm_masks): word i has
  bit j set iff row j is among the n - f rows nearest to row i, row i itself always included; ties to the lower index,
  NaN distances last.  `sq` on the device (where pairwise_sqdist left it, possibly all-reduced): one workgroup, no
  copy, no synchronisation; `sq` on the host: the host form, same masks.  Returns int64[MAX_ROWS] (the 64 bits of each
  mask; zeros beyond n) where `sq` lives."""
  n, f = int(n), int(f)
  if not 1 <= n <= _lib.MAX_ROWS or not 0 <= f < n:
    raise GarInputError(f"nnm: 1 <= n <= {_lib.MAX_ROWS} and 0 <= f < n are needed, got n = {n}, f = {f}")
  if sq.dtype != torch.float64 or sq.numel() < n * n or not sq.is_contiguous():
    raise GarInputError(f"nnm: expected a contiguous float64 matrix of {n} x {n} squared distances")
  lib = _lib.load()
  masks = torch.empty(_lib.MAX_ROWS, dtype=torch.int64, device=sq.device)
  if not sq.is_cuda:
    _lib.check(lib.bm_nnm_masks(_ptr(sq), n, f, _ptr(masks)), "bm_nnm_masks")
    return masks
  with torch.cuda.device(sq.device):
    _lib.check(lib.bm_nnm_masks_device(_ptr(sq), n, f, _ptr(masks), _stream(sq.device)), "bm_nnm_masks_device")
  return masks


def mix_rows(gradients, masks, n_out):
  """n_out averages over subsets of the gradients, from one read of them (bm_mix_rows): output row r is the sequential
  float32 sum, in index order, of the gradients whose bit is set in masks[r] (a DEVICE int64 tensor), divided by their
  count.  A gradient outside a mask is not read into that output; an empty mask gives a NaN row.  Returns a list of
  n_out fresh tensors."""
  n, d, device = _validate(gradients)
  n_out = int(n_out)
  if not 1 <= n_out <= _lib.MAX_ROWS:
    raise GarInputError(f"mix_rows: 1 <= n_out <= {_lib.MAX_ROWS} is needed, got {n_out}")
  _check_masks(masks, n_out, "mix_rows")
  if masks.device != device:
    raise GarInputError(f"mix_rows: the masks must be on {device}")
  # one allocation, every row on a 256-byte boundary whatever d is: the widest stores the inputs allow
  pool = torch.empty((n_out, -(-d // 64) * 64), dtype=torch.float32, device=device)
  outs = [pool[r, :d] for r in range(n_out)]
  if d == 0:
    return outs
  with torch.cuda.device(device):
    _lib.check(_lib.load().bm_mix_rows(_lib.pointer_table(gradients), n, _ptr(masks), n_out, d, _lib.pointer_table(outs),
                                       _stream(device)), "bm_mix_rows")
  return outs


def colwise_mixed(rule, gradients, masks, f=0):
  """`rule` ("median" or "trmean") of the rows mix_rows(gradients, masks, n) would write, without writing them
  (bm_colwise_mixed): same bits.  n <= bm_colwise_mixed_max_rows()."""
  n, d, device = _validate(gradients)
  _check_masks(masks, n, "colwise_mixed")
  out = torch.empty(d, dtype=torch.float32, device=device)
  if d == 0:
    return out
  op = {"median": _lib.OP_MEDIAN, "trmean": _lib.OP_TRMEAN}[rule]
  with torch.cuda.device(device):
    _lib.check(_lib.load().bm_colwise_mixed(op, _lib.pointer_table(gradients), n, _ptr(masks), d, int(f), _ptr(out),
                                            _stream(device)), "bm_colwise_mixed")
  return out


def nnm_rows(gradients, f):
  """The mixed rows of nearest-neighbour mixing: row i replaced by the mean of its n - f nearest rows, itself included
  (one distance pass, the masks on the device, one mixing pass; no host synchronisation)."""
  n, d, device = _validate(gradients)
  return mix_rows(gradients, nnm_masks(pairwise_sqdist(gradients), n, f), n)


def _rule_on(rule, rows, f, rule_args):
  fn = globals()[rule]
  return fn(rows, f=f, **rule_args) if NNM_RULES[rule] else fn(rows, **rule_args)


# ---------------------------------------------------------------------------- #
# The distance-based rules on mixed rows from scalars: no mixed row is written (form="scalars" of nnm / bucketing)

def _mask_words(masks, count, device, where):
  """`masks` as the int64 words the entry points read, where `device` is: a tensor is checked, a sequence of Python
  integers (bucket_masks) is converted."""
  if not isinstance(masks, torch.Tensor):
    masks = _masks_tensor([int(m) for m in masks], device)
  _check_masks(masks, count, where)
  if masks.device != device:
    raise GarInputError(f"{where}: the masks must be on {device}")
  return masks


def mixed_sqdist(sq, n_in, masks, n_out):
  """The n_out x n_out float64 squared distances between the rows mix_rows(gradients, masks, n_out) would write, from the
  n_in x n_in squared distances `sq` of the gradients alone (bm_mixed_sqdist): no mixed row exists.  Equal masks give
  exactly 0, an empty mask NaN in its row and column, a non-finite distance read for a pair NaN.  `sq` on the device
  (where pairwise_sqdist left it, possibly all-reduced): one workgroup, no copy, no synchronisation — a mask with a bit
  at or above n_in then gives NaN everywhere; `sq` on the host: the host form, same bits, and such a mask is refused.
  `masks`: an int64 tensor where `sq` lives (nnm_masks), or a sequence of Python integers (bucket_masks)."""
  n_in, n_out = int(n_in), int(n_out)
  if not 1 <= n_in <= _lib.MAX_ROWS or not 1 <= n_out <= _lib.MAX_ROWS:
    raise GarInputError(f"mixed_sqdist: 1 <= n_in, n_out <= {_lib.MAX_ROWS} is needed, got {n_in}, {n_out}")
  if (not isinstance(sq, torch.Tensor) or sq.dtype != torch.float64 or sq.numel() < n_in * n_in
      or not sq.is_contiguous()):
    raise GarInputError(f"mixed_sqdist: expected a contiguous float64 matrix of {n_in} x {n_in} squared distances")
  masks = _mask_words(masks, n_out, sq.device, "mixed_sqdist")
  lib = _lib.load()
  out = torch.empty((n_out, n_out), dtype=torch.float64, device=sq.device)
  if not sq.is_cuda:
    _lib.check(lib.bm_mixed_sqdist(_ptr(sq), n_in, _ptr(masks), n_out, _ptr(out)), "bm_mixed_sqdist")
    return out
  with torch.cuda.device(sq.device):
    _lib.check(lib.bm_mixed_sqdist_device(_ptr(sq), n_in, _ptr(masks), n_out, _ptr(out), _stream(sq.device)),
               "bm_mixed_sqdist_device")
  return out


def mix_weights(masks, n_in, n_out, weights=None, selection=None, m=None):
  """The weights of the ORIGINAL rows behind a weighted sum of mixed rows (bm_mix_weights): float64[MAX_ROWS], zeros
  beyond n_in — what weighted_sum reads.  Exactly one of
    weights    float64 tensor of at least n_out entries (center_weights), or
    selection  int32 tensor whose first m entries name the mixed rows that are averaged (a ranking, a Brute subset): 1 / m
               each, duplicates add up, an entry outside 0 .. n_out-1 gives NaN everywhere.
  `masks`: an int64 tensor (host or device: the host or the device form, same bits) or a sequence of Python integers,
  which goes where the weights / the selection live."""
  n_in, n_out = int(n_in), int(n_out)
  if not 1 <= n_in <= _lib.MAX_ROWS or not 1 <= n_out <= _lib.MAX_ROWS:
    raise GarInputError(f"mix_weights: 1 <= n_in, n_out <= {_lib.MAX_ROWS} is needed, got {n_in}, {n_out}")
  if (weights is None) == (selection is None):
    raise ValueError("mix_weights: exactly one of weights and selection is needed")
  given = weights if weights is not None else selection
  if not isinstance(given, torch.Tensor) or given.dim() != 1 or not given.is_contiguous():
    raise GarInputError("mix_weights: weights / selection must be a contiguous 1-D tensor")
  masks = _mask_words(masks, n_out, given.device, "mix_weights")
  if weights is not None:
    if weights.dtype != torch.float64 or weights.numel() < n_out:
      raise GarInputError(f"mix_weights: weights must be a float64 tensor of at least {n_out} entries")
    m = 0
  else:
    if m is None:
      raise ValueError("mix_weights: m (how many entries of the selection are averaged) is needed")
    m = int(m)
    if not 1 <= m <= _lib.MAX_ROWS:
      raise GarInputError(f"mix_weights: 1 <= m <= {_lib.MAX_ROWS} is needed, got {m}")
    if selection.dtype != torch.int32 or selection.numel() < m:
      raise GarInputError(f"mix_weights: selection must be an int32 tensor of at least {m} entries")
  lib = _lib.load()
  out = torch.empty(_lib.MAX_ROWS, dtype=torch.float64, device=given.device)
  args = (_ptr(masks), n_in, n_out, None if weights is None else _ptr(weights),
          None if selection is None else _ptr(selection), m, _ptr(out))
  if not given.is_cuda:
    _lib.check(lib.bm_mix_weights(*args), "bm_mix_weights")
    return out
  with torch.cuda.device(given.device):
    _lib.check(lib.bm_mix_weights_device(*args, _stream(given.device)), "bm_mix_weights_device")
  return out


class _Legs:
  """The launching functions of this module as the pipelines call them, looked up in the module at CALL time (a test
  that replaces one sees its calls)."""

  def __getattr__(self, name):
    return globals()[name]

  def rank(self, sq, n, f, m, mode):
    return rank_from_sqdist(sq, n, f, m, mode)[0]

  def host_selection(self, sq, n, f, like):
    """The host Brute search (no node budget) on the squared distances `sq`, as a device index table."""
    table = torch.zeros(_lib.MAX_ROWS, dtype=torch.int32)
    table[:n - f] = torch.tensor(brute_select_host(sq.sqrt().cpu().contiguous(), n, f), dtype=torch.int32)
    return table.to(like.device)


_legs = _Legs()


def _rule_on_scalars(where, gradients, rule, n_out, masks_from, need_sq, rule_args):
  """`rule` on the n_out mixed rows of `gradients` without writing one (pipelines.on_scalars): launches on the current
  stream only; the one synchronisation is brute's with check=True.  The result carries `mix_masks`, `mix_weights` and,
  for krum and brute, `mix_selection` = (index tensor, count)."""
  global last_brute_status
  n, d, device = _validate(gradients)
  if NNM_RULES[rule] and "f" not in rule_args:
    raise TypeError(f"{where}: {rule} needs f (the rule's f on the {n_out} mixed rows)")
  out, record = pipelines.on_scalars(_legs, pairwise_sqdist, gradients, rule, rule_args.get("f"), n_out, masks_from,
                                     need_sq, rule_args)
  out.mix_masks, out.mix_weights, out.mix_selection = record.masks_read, record.weights, record.selection
  if rule == "brute":
    status = record.brute_status
    if status is None:  # (a host re-search)
      status = torch.zeros(1, dtype=torch.int32, device=device)
    last_brute_status = out.brute_status = status
  return out


def nnm(gradients, f, rule="trmean", form="rows", **rule_args):
  """Nearest-neighbour mixing, then `rule` on the mixed rows (NNM o rule of "Fixing by Mixing"): one distance pass, the
  neighbour masks on the device, then
    median / trmean up to bm_colwise_mixed_max_rows() rows: ONE kernel that mixes in registers and applies the rule (the
      stack is read once, no mixed row is written);
    otherwise: mix_rows, then the rule's own function on the mixed rows (rule_args are handed to it; `f` is the rule's f
      as well).
  form="scalars" (krum, brute, geomed, cclip, average: SCALAR_RULES; any other rule raises ValueError) writes no mixed
  row either: the distances between mixed rows come from the distance matrix the masks were made of (mixed_sqdist), the
  rule's scalar stage runs on them, and its output is ONE weighted sum of the original rows (mix_weights, weighted_sum) —
  the same selection as form="rows" wherever the rule's decisions are not within the distance pass's error of a tie.
  No host synchronisation (graph-capturable) where the rule has none.  An unknown rule raises ValueError."""
  pipelines.check_rule_form("nnm", rule, form)
  n, d, device = _validate(gradients)
  if form == "scalars":
    if NNM_RULES[rule]:
      rule_args = dict(rule_args, f=f)
    return _rule_on_scalars("nnm", gradients, rule, n, lambda sq: nnm_masks(sq, n, f), True, rule_args)
  masks = nnm_masks(pairwise_sqdist(gradients), n, f)
  if rule in ("median", "trmean") and not rule_args and n <= _lib.load().bm_colwise_mixed_max_rows():
    return colwise_mixed(rule, gradients, masks, f if rule == "trmean" else 0)
  return _rule_on(rule, mix_rows(gradients, masks, n), f, rule_args)


def bucket_masks(n, s, perm):
  """The ceil(n / s) masks of bucketing: bucket b holds perm[b s .. b s + s) (the last one may be smaller).  Host list of
  Python integers."""
  masks = []
  for lo in range(0, n, s):
    m = 0
    for j in perm[lo:lo + s]:
      m |= 1 << int(j)
    masks.append(m)
  return masks


def _masks_tensor(masks, device):
  """Python integers (64-bit patterns) as the int64 words the kernels read."""
  return torch.tensor([m - (1 << 64) if m >= (1 << 63) else m for m in masks], dtype=torch.int64).to(device)


_U64 = (1 << 64) - 1


def _bucket_mix(x):
  x ^= x >> 30
  x = (x * 0xBF58476D1CE4E5B9) & _U64
  x ^= x >> 27
  x = (x * 0x94D049BB133111EB) & _U64
  return x ^ (x >> 31)


def bucket_permutation(n, seed, counter):
  """The permutation of 0 .. n-1 bucketing draws from a counter (include/bm_gar.h, bm_bucket_masks), in Python integers:
  u_i = mix(seed + 0x9E3779B97F4A7C15 * (64 * counter + i)), then for i = n-1 down to 1 swap perm[i] and
  perm[u_i mod (i + 1)]; uint64 and wrapping throughout.  A function of (n, seed, counter) alone: no generator, no state,
  the same list on every rank and what bm_bucket_masks / bm_bucket_masks_device cut into buckets."""
  n, seed, counter = int(n), int(seed) & _U64, int(counter) & _U64
  if not 1 <= n <= _lib.MAX_ROWS:
    raise ValueError(f"bucket_permutation: 1 <= n <= {_lib.MAX_ROWS} is needed, got {n}")
  perm = list(range(n))
  for i in range(n - 1, 0, -1):
    j = _bucket_mix((seed + 0x9E3779B97F4A7C15 * ((64 * counter + i) & _U64)) & _U64) % (i + 1)
    perm[i], perm[j] = perm[j], perm[i]
  return perm


def _check_bucket_args(n, s):
  n, s = int(n), int(s)
  if not 1 <= n <= _lib.MAX_ROWS or not 1 <= s <= n:
    raise ValueError(f"bucketing: 1 <= n <= {_lib.MAX_ROWS} and a bucket size within 1..n are needed, got n = {n}, s = {s}")
  return n, s


def bucket_masks_host(n, s, seed, counter):
  """The masks bm_bucket_masks writes for (n, s, seed, counter): a host int64[MAX_ROWS] tensor, zeros beyond ceil(n / s)."""
  n, s = _check_bucket_args(n, s)
  masks = torch.empty(_lib.MAX_ROWS, dtype=torch.int64)
  _lib.check(_lib.load().bm_bucket_masks(n, s, int(seed) & _U64, int(counter) & _U64, _ptr(masks)), "bm_bucket_masks")
  return masks


def bucket_masks_device(n, s, seed, counter_dev, out=None):
  """The bucket masks of the counter `counter_dev` holds (a DEVICE int64[1] tensor), drawn on the device
  (bm_bucket_masks_device: one wavefront, no synchronisation); the counter word is advanced by one, so a replayed graph
  draws the next permutation each time.  Returns int64[MAX_ROWS] (`out` when given: a graph needs a fixed address)."""
  n, s = _check_bucket_args(n, s)
  if (not isinstance(counter_dev, torch.Tensor) or not counter_dev.is_cuda or counter_dev.dtype != torch.int64
      or counter_dev.numel() < 1 or not counter_dev.is_contiguous()):
    raise GarInputError("bucket_masks_device: the counter must be a contiguous int64 tensor on a GPU")
  device = counter_dev.device
  if out is None:
    out = torch.empty(_lib.MAX_ROWS, dtype=torch.int64, device=device)
  _check_masks(out, _lib.MAX_ROWS, "bucket_masks_device")
  if out.device != device:
    raise GarInputError(f"bucket_masks_device: the masks must be on {device}")
  with torch.cuda.device(device):
    _lib.check(_lib.load().bm_bucket_masks_device(n, s, int(seed) & _U64, _ptr(counter_dev), _ptr(out), _stream(device)),
               "bm_bucket_masks_device")
  return out


def colwise_bucketed_supported(rule, n, n_out):
  """Whether bm_colwise_bucketed has an instance for `rule` on n rows mixed into n_out."""
  op = {"median": _lib.OP_MEDIAN, "trmean": _lib.OP_TRMEAN}.get(rule)
  return op is not None and bool(_lib.load().bm_colwise_bucketed_supported(op, int(n), int(n_out)))


def colwise_bucketed(rule, gradients, masks, n_out, f=0):
  """`rule` ("median" or "trmean", f the trimmed mean's on the n_out rows) of the rows mix_rows(gradients, masks, n_out)
  would write, without writing them (bm_colwise_bucketed): same bits.  Raises where colwise_bucketed_supported says no."""
  n, d, device = _validate(gradients)
  n_out = int(n_out)
  if not 1 <= n_out <= n:
    raise GarInputError(f"colwise_bucketed: 1 <= n_out <= {n} is needed, got {n_out}")
  _check_masks(masks, n_out, "colwise_bucketed")
  if masks.device != device:
    raise GarInputError(f"colwise_bucketed: the masks must be on {device}")
  out = torch.empty(d, dtype=torch.float32, device=device)
  op = {"median": _lib.OP_MEDIAN, "trmean": _lib.OP_TRMEAN}[rule]
  with torch.cuda.device(device):
    _lib.check(_lib.load().bm_colwise_bucketed(op, _lib.pointer_table(gradients), n, _ptr(masks), n_out, d, int(f),
                                               _ptr(out), _stream(device)), "bm_colwise_bucketed")
  return out


def _fused_bucketed(rule, n, n_out, rule_args):
  """The f bm_colwise_bucketed is handed when `rule` on n rows in n_out buckets takes the fused kernel, else None: median
  with no argument, trmean with `f` and nothing else, and an instance for the shape."""
  if rule == "median" and not rule_args:
    f = 0
  elif rule == "trmean" and set(rule_args) == {"f"} and isinstance(rule_args["f"], int) and 0 <= 2 * rule_args["f"] < n_out:
    f = rule_args["f"]
  else:
    return None
  return f if colwise_bucketed_supported(rule, n, n_out) else None


def bucketing(gradients, s, rule, seed=None, perm=None, form="rows", counter=None, **rule_args):
  """Bucketing (Karimireddy, He, Jaggi, ICLR 2022): the rows are shuffled, averaged in buckets of s, and `rule` runs on
  the ceil(n / s) bucket means.  The permutation is drawn on the host (torch generator seeded with `seed`; None: the
  global generator), given as `perm`, a sequence holding 0 .. n-1 once each, or — `counter` given — the counter-based
  draw bucket_permutation(n, seed or 0, counter), the one bm_bucket_masks and its device form define to the bit.
  median / trmean (rule_args holding nothing but trmean's `f`) where bm_colwise_bucketed has an instance: ONE kernel that
  forms the bucket means in registers and applies the rule, the same bits; otherwise one mixing pass (mix_rows), then the
  rule's own function.  The rule's `f` is the CALLER's business — pass it in rule_args: after bucketing at most f of the
  ceil(n / s) means contain a Byzantine row, so the rule has to be admissible for that f on that many rows.
  form="scalars" (SCALAR_RULES only) writes no bucket mean: one distance pass over the rows (none for "average"), the
  rule's scalar stage on the distances between the means (mixed_sqdist), one weighted sum of the rows."""
  pipelines.check_rule_form("bucketing", rule, form)
  n, d, device = _validate(gradients)
  s = int(s)
  if not 1 <= s <= n:
    raise ValueError(f"bucketing: the bucket size must be within 1..{n}, got {s}")
  if counter is not None:
    if perm is not None:
      raise ValueError("bucketing: perm and counter exclude one another")
    perm = bucket_permutation(n, 0 if seed is None else seed, counter)
  if perm is None:
    gen = None if seed is None else torch.Generator().manual_seed(int(seed))
    perm = torch.randperm(n, generator=gen).tolist()
  perm = [int(j) for j in perm]
  if sorted(perm) != list(range(n)):
    raise ValueError(f"bucketing: perm must hold 0..{n - 1} once each")
  masks = bucket_masks(n, s, perm)
  if form == "scalars":
    return _rule_on_scalars("bucketing", gradients, rule, len(masks), lambda sq: _masks_tensor(masks, device), False,
                            rule_args)
  fused_f = _fused_bucketed(rule, n, len(masks), rule_args) if d > 0 else None
  if fused_f is not None:
    return colwise_bucketed(rule, gradients, _masks_tensor(masks, device), len(masks), fused_f)
  means = mix_rows(gradients, _masks_tensor(masks, device), len(masks))
  return globals()[rule](means, **rule_args)


def cge_selection(gradients, f, **kwargs):
  """Device order of the gradients by increasing norm, non-finite last (aggregators/cge.py:28-38)."""
  from . import stats
  return stable_argsort(stats.row_sqnorms(gradients), len(gradients))


def cge(gradients, f, **kwargs):
  """Comparative gradient elimination (aggregators/cge.py:40-57)."""
  n = len(gradients)
  return selected_mean(gradients, cge_selection(gradients, f), n - f)
