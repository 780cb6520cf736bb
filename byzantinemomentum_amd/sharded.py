"""Dimension-sharded aggregation over several GPUs (one process per GPU, RCCL over xGMI).

The reference has no multi-GPU aggregation; this is the MI355X scaling axis of
the path.  Every rank holds the SAME n workers but only its slice [lo, hi) of the d coordinates:

  * coordinate-wise rules (median, trmean, phocas, meamed), Bulyan pass 2, selected means and
    momentum are independent per coordinate  -> no communication at all;
  * distance-based selection needs ONE exchange: each rank computes partial SQUARED distances over
    its slice, a single all-reduce(sum) of an n x n fp64 buffer (<= 32 KB, latency-bound on xGMI —
    never a d-sized collective) gives every rank the same matrix, and every rank runs the same
    deterministic score/rank kernel -> identical selections without further traffic;
  * Aksel: all-reduce of the n partial squared distances to the (local) median slices;
  * statistics: ONE all-gather of the packed per-rank scalars (sums and maxima together), reduced
    locally in rank order (`exchange`);
  * the full aggregated vector, when a consumer needs it on every rank, is ONE all-gather of the
    d/P slices (the only bandwidth collective: 7 peers on 7 links in parallel).

The compute legs are injected (`backend`): the product uses the HIP backend below; the CPU/gloo
tests of tests/test_sharded_gloo.py inject an oracle-backed one to exercise partitioning and
collectives without a GPU.  With world_size 1 no collective is ever issued.
"""

import ctypes
import math
import warnings

import torch
import torch.distributed as dist

from . import _lib

__all__ = ["shard_bounds", "owned_workers", "Shards", "ShardedAggregator", "HipBackend", "NativeComm"]


class Shards(list):
  """The n gradients restricted to this rank's coordinate slice, which KNOW the length of the whole vectors
  (`d_total`): what `ShardedAggregator.to_dim_sharded` and `shard_rows` return.  The distance-based rules read the
  total from it, so that an aggregator serves any sequence of vector lengths (per-layer aggregation, several
  models) without a collective to find the total out and without guessing."""

  def __init__(self, rows=(), d_total=None):
    super().__init__(rows)
    self.d_total = None if d_total is None else int(d_total)


def shard_bounds(d, world_size, rank, align=64):
  """Contiguous slice [lo, hi) of rank `rank`: ceil(d/P) rounded up to `align` coordinates
  (256 B, keeps every shard 16-byte aligned for the float4 kernels). Trailing ranks may be empty."""
  per = -(-d // world_size)
  per = -(-per // align) * align
  lo = min(rank * per, d)
  hi = min(lo + per, d)
  return lo, hi


def owned_workers(n, world_size, rank):
  """Workers whose gradients rank `rank` produces in the worker-parallel layout: rank, rank+P, ...
  (round robin, so that a worker count that P does not divide still spreads evenly)."""
  return list(range(rank, n, world_size))


class NativeComm:
  """RCCL communicator owned by libbm_gar.so (bm_comm_*): lets the sharded rules run as ONE C call
  per aggregation with the all-reduce issued from C on the caller's stream.  Bootstrapped through the
  existing torch.distributed group (rank 0's unique id is broadcast as a Python object)."""

  def __init__(self, group=None, vote=None):
    """vote(ok) -> bool: "did this step succeed on EVERY rank?" (a collective of the torch group).  With it, no rank
    can be left alone in a collective: the unique id is only broadcast once every rank knows rank 0 made one, and a
    failure of bm_comm_init on one rank is learnt by all (the caller's last vote).  Without it (vote=None) a failure
    simply raises on the rank it happens on."""
    lib = _lib.load()
    if not lib.bm_comm_available():
      raise RuntimeError("RCCL could not be bound by libbm_gar.so")
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    ident, failure = [None], None
    if rank == 0:
      try:
        buf = ctypes.create_string_buffer(128)
        _lib.check(lib.bm_comm_unique_id(buf), "bm_comm_unique_id")
        ident[0] = buf.raw
      except Exception as err:  # noqa: BLE001
        failure = err
    # rank 0 must not skip the broadcast its peers are about to enter: first everyone learns whether there is an id
    if vote is not None:
      if not vote(failure is None):
        raise RuntimeError(f"bm_comm_unique_id failed on rank 0: {failure}" if failure is not None else
                           "bm_comm_unique_id failed on rank 0")
    elif failure is not None:
      raise failure
    dist.broadcast_object_list(ident, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    handle = ctypes.c_void_p()
    _lib.check(lib.bm_comm_init(ctypes.byref(handle), world, rank, ctypes.c_char_p(ident[0])), "bm_comm_init")
    self.handle = handle
    self.world_size = world

  def close(self):
    if self.handle is not None and self.handle.value:
      _lib.load().bm_comm_destroy(self.handle)
      self.handle = None

  def __del__(self):
    try:
      self.close()
    except Exception:  # noqa: BLE001  (interpreter shutdown)
      pass


class HipBackend:
  """Compute legs on the local MI355X (libbm_gar.so).  No CPU fallback."""

  # the optional legs step.AggregationStep plans with (read once, in its constructor); each names a method below
  capabilities = frozenset((
    "step_worker", "momentum_stats_colwise", "momentum_stats_sqdist", "stack_stats_colwise", "stack_stats_sqdist",
    "device_search", "attack_ranking_device", "bulyan_pass2_eval", "order_pair", "colwise_eval", "sqdist2", "anticge",
    "accept_count", "attack_vector", "center_weights", "weighted_sum", "nnm_masks", "mix_rows", "colwise_mixed",
    "mixed_sqdist", "mix_weights", "spectral_weights", "perturb_stats", "minmax_factor"))

  def __init__(self):
    from . import gars, stats
    self.gars = gars
    self.stats = stats

  # -- aggregation rules ------------------------------------------------------ #

  def pairwise_sqdist(self, gradients, d_total=None):
    return self.gars.pairwise_sqdist(gradients, d_total)

  def rank(self, sq, n, f, m, mode):
    order, _ = self.gars.rank_from_sqdist(sq, n, f, m, mode)
    return order

  def selected_mean(self, gradients, order, m):
    return self.gars.selected_mean(gradients, order, m)

  def bulyan_pass2(self, gradients, order, f, m):
    return self.gars.bulyan_pass2(gradients, order, f, m)

  def colwise(self, rule, gradients, f):
    return getattr(self.gars, rule)(gradients, f=f) if rule != "median" else self.gars.median(gradients)

  def aksel_sqdist(self, gradients):
    return self.gars.aksel_sqdist(gradients)[:len(gradients)]

  def argsort(self, keys, n):
    return self.gars.stable_argsort(keys, n)

  def brute_select(self, dist_host, n, f):
    return self.gars.brute_select_host(dist_host, n, f)

  def brute_select_device(self, sq, n, f):
    """(sel, status) on the device; status -1 = no subset of n - f rows has a finite diameter (brute.py:68)."""
    return self.gars.brute_select_device(sq, n, f)

  def center_weights(self, sq, n, mode, param, iters, tol, has_start):
    """The weights of the geometric median / centered clipping from the (all-reduced) squared distances, where they
    are (bm_center_weights_device: one workgroup, no synchronisation): (weights fp64[MAX_ROWS], info fp64[3])."""
    return self.gars.center_weights(sq, n, mode, param, iters, tol, has_start)

  def spectral_weights(self, sq, n, mode, count, power_iters):
    """The weights of CAF / DnC from the (all-reduced) squared distances, where they are (bm_spectral_weights_device:
    one workgroup, no synchronisation): (weights fp64[MAX_ROWS], info fp64[4])."""
    return self.gars.spectral_weights(sq, n, mode, count, power_iters)

  def weighted_sum(self, gradients, weights):
    return self.gars.weighted_sum(gradients, weights)

  def nnm_masks(self, sq, n, f):
    """The neighbour masks of nearest-neighbour mixing from the (all-reduced) squared distances, where they are
    (bm_nnm_masks_device: one workgroup, no synchronisation): int64[MAX_ROWS]."""
    return self.gars.nnm_masks(sq, n, f)

  def mix_rows(self, gradients, masks, n_out):
    return self.gars.mix_rows(gradients, masks, n_out)

  def mixed_sqdist(self, sq, n_in, masks, n_out):
    """The squared distances between mixed rows from the (all-reduced) distances of the rows, where they are
    (bm_mixed_sqdist_device: one workgroup, no synchronisation): fp64 (n_out, n_out)."""
    return self.gars.mixed_sqdist(sq, n_in, masks, n_out)

  def mix_weights(self, masks, n_in, n_out, weights=None, selection=None, m=None):
    return self.gars.mix_weights(masks, n_in, n_out, weights=weights, selection=selection, m=m)

  def colwise_mixed_max_rows(self):
    return _lib.load().bm_colwise_mixed_max_rows()

  def colwise_mixed(self, rule, gradients, masks, f):
    return self.gars.colwise_mixed(rule, gradients, masks, f)

  def sharded_rule(self, name, comm, gradients, f, m, d_total=None, with_order=False):
    """Multi-Krum / Bulyan of the local slice in one C call (bm_sharded_krum / bm_sharded_bulyan);
    comm: NativeComm or None (one rank); d_total: length of the whole vectors (default: this shard's).
    with_order: return (out, ranking) — the ranking where the call left it, a view of this stream's workspace
    (bm_sharded_order_slot: no copy), valid on this stream until the next sharded rule reuses the workspace."""
    gars = self.gars
    n, d, device = gars._validate(gradients)
    lib = _lib.load()
    out = torch.empty(d, dtype=torch.float32, device=device)
    nbytes = lib.bm_sharded_workspace_bytes(n, d)
    ws = gars._Scratch.get(device, "ws_sharded", nbytes=int(nbytes))
    fn = lib.bm_sharded_krum if name == "krum" else lib.bm_sharded_bulyan
    with torch.cuda.device(device):
      _lib.check(fn(comm.handle if comm is not None else None, _lib.pointer_table(gradients), n, d,
                    int(d_total) if d_total is not None else d, f, m, gars._ptr(out), None, gars._ptr(ws), gars._stream(device)), "bm_sharded_" + name)
    if with_order:
      at = lib.bm_sharded_order_slot(gars._ptr(ws)) - ws.data_ptr()
      return out, ws[at:at + 4 * _lib.MAX_ROWS].view(torch.int32)
    return out

  def index_tensor(self, indices, like):
    return torch.tensor(indices, dtype=torch.int32, device=like.device)

  def sum_over_ranks(self, agg, value):
    """A host integer summed over the ranks (shard lengths: once per shape, not per call)."""
    t = torch.tensor([float(value)], dtype=torch.float64, device=torch.device("cuda", torch.cuda.current_device()))
    return int(agg.all_reduce_sum(t).item())

  # -- step statistics and momentum -------------------------------------------- #

  def stack_stats(self, samples, scale=None, attack="empire", want_avg=True, direction=False):
    return self.stats.stack_stats_async(samples, scale=scale, attack=attack, want_avg=want_avg, direction=direction)

  def momentum_stats(self, sampled, buffers, mu, omd, factors, scale, attack, direction=False):
    return self.stats.momentum_stats(sampled, buffers, mu, omd, factors, scale, attack, direction)

  def momentum_stats_colwise(self, *args, **kwargs):
    return self.stats.momentum_stats_colwise(*args, **kwargs)

  def stack_stats_colwise(self, *args, **kwargs):
    return self.stats.stack_stats_colwise(*args, **kwargs)

  def stack_stats_sqdist(self, *args, **kwargs):
    return self.stats.stack_stats_sqdist(*args, **kwargs)

  def momentum_stats_sqdist(self, *args, **kwargs):
    return self.stats.momentum_stats_sqdist(*args, **kwargs)

  def multi_fma3(self, outs, ps, qs, a, b, p_scale=None):
    return self.stats.multi_fma3(outs, ps, qs, a, b, p_scale)

  @property
  def device_search_rules(self):
    """Rules whose factor search runs on the device (step.AggregationStep, line_search="auto")."""
    return self.stats.DEVICE_SEARCH_RULES

  def attack_search_device(self, *args, **kwargs):
    return self.stats.attack_search_device(*args, **kwargs)

  def device_search(self, device, evals, negative=False):
    """The exploration's cursor in device memory (stats.DeviceSearch): the host queues every evaluation of a search."""
    return self.stats.DeviceSearch(device, evals, negative)

  def multi_scale(self, ys, factors):
    return self.stats.multi_scale(ys, factors)

  def row_sqnorms(self, gradients):
    return self.stats.row_sqnorms(gradients).contiguous()

  def clip_factors_from_sq(self, sq, k, clip):
    return self.stats.clip_factors_from_sq(sq, k, clip)

  def study_stats(self, *args, **kwargs):
    return self.stats.study_stats(*args, **kwargs)

  def accept_count(self, order, count, h):
    """Entries >= h among the first `count` of a device index table, as a device fp64[1] (stats.accept_count)."""
    return self.stats.accept_count(order, count, h)

  def anticge(self, honests, f_decl, reduce):
    """The vector of the `anticge` attack on this device's slice of the honest gradients (stats.anticge_sum /
    anticge_scale); reduce(t): the in-place sum over the ranks of a small device tensor, the identity with one rank."""
    byz, _, scal = self.stats.anticge_sum(honests, f_decl, reduce(self.row_sqnorms(honests)))
    reduce(scal[:1])
    return self.stats.anticge_scale(byz, scal)

  def attack_vector(self, kind, h_avg, factor=None, target=None, want_direction=False):
    return self.stats.attack_vector(kind, h_avg, factor, target, want_direction)

  def perturb_stats(self, honests, perturbation):
    """(avg, dir, scal) of the Min-Max / Min-Sum attacks on this device's slice of the honest gradients
    (stats.perturb_stats, bm_perturb_stats): one pass over the rows, no synchronisation."""
    return self.stats.perturb_stats(honests, perturbation)

  def minmax_factor(self, sq, scal, h, mode):
    """The closed-form factor from the (all-reduced) distances and scalars, where they are (bm_minmax_factor_device:
    one workgroup, no synchronisation): fp64[6]."""
    return self.stats.minmax_factor(sq, scal, h, mode)

  def colwise_eval_supported(self, rule, n):
    return self.stats.colwise_eval_supported(rule, n)

  def colwise_eval(self, *args, **kwargs):
    return self.stats.colwise_eval(*args, **kwargs)

  def sqdist2(self, a, b):
    return self.stats.sqdist2(a, b)

  def attack_ranking_device(self, *args, **kwargs):
    return self.stats.attack_ranking_device(*args, **kwargs)

  def bulyan_pass2_eval_supported(self, n, f, m, d=0):
    return self.stats.bulyan_pass2_eval_supported(n, f, m, d)

  def bulyan_pass2_eval(self, *args, **kwargs):
    return self.stats.bulyan_pass2_eval(*args, **kwargs)

  def order_pair_supported(self, h):
    return self.stats.order_pair_supported(h)

  def order_pair(self, rows, il, ih):
    return self.stats.order_pair(rows, il, ih)

  def study_dots(self, core, extra):
    return self.stats.study_dots(core, extra)

  def step_worker(self, comm, *args, **kwargs):
    """One whole step with worker-side momentum in one C call (bm_step_worker)."""
    return self.stats.step_worker(comm, *args, **kwargs)


def _anticge_sum_torch(backend, local, f_decl, sq):
  """bm_anticge_sum in plain torch for a backend without the kernel: (S, order, [sum S^2 here, |g_(maxpos)|^2])."""
  h = len(local)
  maxpos = h - f_decl
  keys = torch.where(torch.isfinite(sq[:h]), sq[:h], torch.full_like(sq[:h], math.inf))
  order = backend.argsort(keys, h)
  ranked = order[:h].tolist()
  attack = local[ranked[0]].clone()
  for i in ranked[:maxpos]:  # (the smallest row a second time first: anticge.py:70-72)
    attack.add_(local[i])
  return attack, order, torch.stack([attack.double().pow(2).sum(), keys[ranked[maxpos]]])


def _anticge_scale_torch(vec, scal):
  """bm_anticge_scale in plain torch: the norms as fp32 numbers, nextafter and quotient in double (anticge.py:68,74-76)."""
  attnorm, byznorm = scal.sqrt().float().tolist()
  if attnorm > 0:
    vec.mul_(-math.nextafter(byznorm, 0) / attnorm)
  return vec


def _perturb_stats_torch(backend, local, perturbation):
  """bm_perturb_stats in plain torch for a backend without the kernel: the backend's sequential fp32 average, the
  direction in fp32, the scalars as fp64 sums of the fp32 vectors."""
  h = len(local)
  avg = backend.stack_stats(local)[0]
  if perturbation == "unit":
    direction = avg.neg()
  elif perturbation == "std":
    direction = torch.stack(list(local)).var(dim=0).sqrt_().neg_() if avg.numel() else avg.clone()
  else:
    direction = torch.sign(avg).neg_()
  p64, a64 = direction.double(), avg.double()
  scal = torch.zeros(_lib.PERTURB_SLOTS, dtype=torch.float64, device=avg.device)
  for i in range(h):
    scal[i] = torch.dot(p64, a64 - local[i].double())
  scal[_lib.PERTURB_P], scal[_lib.PERTURB_N] = torch.dot(p64, p64), torch.dot(a64, a64)
  return avg, direction, scal


def _minmax_factor_torch(sq, scal, h, mode):
  """bm_minmax_factor in Python floats (fp64, plain index order: the host form's arithmetic): fp64[6]."""
  D = sq.reshape(-1)[:h * h].reshape(h, h).tolist()
  sc = scal.tolist()
  b, P, N = sc[:h], sc[_lib.PERTURB_P], sc[_lib.PERTURB_N]
  rowsum = []
  for i in range(h):
    t = 0.0
    for j in range(h):
      t = t + D[i][j]
    rowsum.append(t)
  total = 0.0
  for t in rowsum:
    total = total + t
  a = [max(rowsum[i] / h - total / (2.0 * h * h), 0.0) if not math.isnan(rowsum[i]) else math.nan for i in range(h)]
  gamma, binding, ok = 0.0, -1.0, P > 0.0 and math.isfinite(P)
  if mode == "minmax":
    pairs = [D[i][j] for i in range(h) for j in range(i + 1, h)]
    bound = math.nan if any(math.isnan(v) for v in pairs) else max(pairs)
    ok = ok and math.isfinite(bound) and all(math.isfinite(v) for v in a + b)
    if ok:
      disc = [b[i] * b[i] + P * (bound - a[i]) for i in range(h)]
      ok = all(v >= 0.0 for v in disc)
    if ok:
      cands = [(-b[i] + math.sqrt(disc[i])) / P for i in range(h)]
      best = min(range(h), key=lambda i: (cands[i], i))
      ok = math.isfinite(cands[best])
      if ok:
        gamma, binding = cands[best], float(best)
  else:
    bound = math.nan if any(math.isnan(v) for v in rowsum) else max(rowsum)
    A = B = 0.0
    for i in range(h):
      A, B = A + a[i], B + b[i]
    disc = B * B + h * P * (bound - A)
    ok = ok and math.isfinite(bound) and math.isfinite(A) and math.isfinite(B) and disc >= 0.0
    if ok:
      g = (-B + math.sqrt(disc)) / (h * P)
      ok = math.isfinite(g)
      gamma = g if ok else 0.0
  return torch.tensor([gamma, bound, binding, P, N, 0.0 if ok else 1.0], dtype=torch.float64, device=sq.device)


def _attack_vector_torch(kind, avg, factor, target, want_direction):
  """bm_attack_vector in plain torch for a backend without the kernel: the same fp32 expression at every coordinate,
  avg + factor * dir with dir in {0, 1} (never a copy of avg), the factor rounded to fp32 first."""
  if kind == "nan":
    return torch.full_like(avg, math.nan)
  if isinstance(factor, torch.Tensor):  # (a device search's float64[1]: rounded as the kernel rounds it)
    factor = factor.reshape(-1)[0].to(avg.device, torch.float32)
  else:
    factor = torch.tensor(float(factor), dtype=torch.float32, device=avg.device)
  if kind == "scale":
    return avg * factor
  direction = torch.ones_like(avg) if kind == "shift_all" else torch.zeros_like(avg)
  if kind == "shift_one" and target is not None and target >= 0:
    direction[target] = 1
  out = avg + factor * direction
  return (out, direction) if want_direction else out


def _center_weights_torch(sq, n, mode, param, iters, tol, has_start):
  """bm_center_weights in plain torch (fp64, where `sq` lives) for a backend without the kernel: the iteration of
  include/bm_gar.h on the weights — (weights fp64[MAX_ROWS], info fp64[3])."""
  N = n + (1 if has_start else 0)
  D = sq[:N, :N].to(torch.float64)
  weights = torch.zeros(_lib.MAX_ROWS, dtype=torch.float64, device=sq.device)
  off = ~torch.eye(N, dtype=torch.bool, device=sq.device)
  bad = (~torch.isfinite(D) & off).sum(dim=1)
  usable = ~((bad > 0) & (2 * bad >= N - 1))
  rows = usable.clone()
  rows[n:] = False
  U = int(rows.sum())
  if U == 0:
    weights[:N] = math.nan
    return weights, torch.tensor([0.0, math.nan, 0.0], dtype=torch.float64, device=sq.device)
  Dz = torch.where(torch.isfinite(D), D, torch.zeros_like(D))  # (a term of weight 0 is skipped, whatever D holds)
  blind = ~torch.isfinite(D)
  c = torch.zeros(N, dtype=torch.float64, device=sq.device)
  if has_start and bool(usable[n]):
    c[n] = 1.0
  else:
    c[rows] = 1.0 / U

  def dot_rows(w):  # sum_j w_j D_ij with the terms of weight 0 skipped; NaN where a term that counts is not finite
    t = Dz @ w
    return torch.where((blind & (w != 0)[None, :]).any(dim=1), torch.full_like(t, math.nan), t)

  done, move2 = 0, 0.0
  for _ in range(iters):
    t = dot_rows(c)
    q = (c * torch.where(c != 0, t, torch.zeros_like(t))).sum()
    r2 = t - 0.5 * q
    r = torch.where(torch.isfinite(r2), r2.clamp_min(0.0).sqrt(), torch.full_like(r2, math.inf))
    if mode == "geomed":
      w = torch.where(rows, 1.0 / r.clamp_min(param), torch.zeros_like(r))
      nxt = w / w.sum()
    else:
      s = torch.where(rows, torch.where(r <= param, torch.ones_like(r), param / r), torch.zeros_like(r))
      nxt = c * (1.0 - s.sum() / U) + s / U
    e = nxt - c
    c = nxt
    u = dot_rows(e)
    move2 = max(0.0, -0.5 * float((e * torch.where(e != 0, u, torch.zeros_like(u))).sum()))
    done += 1
    if tol > 0 and math.sqrt(move2) <= tol:
      break
  weights[:N] = c
  return weights, torch.tensor([float(done), move2, float(U)], dtype=torch.float64, device=sq.device)


def _spectral_weights_torch(sq, n, mode, count, power_iters):
  """bm_spectral_weights in plain torch (fp64, where `sq` lives) for a backend without the kernel: the filter of
  include/bm_gar.h on the squared distances — (weights fp64[MAX_ROWS], info fp64[4])."""
  D = sq.reshape(-1)[:n * n].reshape(n, n).to(torch.float64)
  weights = torch.zeros(_lib.MAX_ROWS, dtype=torch.float64, device=sq.device)
  off = ~torch.eye(n, dtype=torch.bool, device=sq.device)
  bad = (~torch.isfinite(D) & off).sum(dim=1)
  usable = ~((bad > 0) & (2 * bad >= n - 1))
  U = int(usable.sum())

  def info(rounds, lam, kept):
    return torch.tensor([float(rounds), lam, float(U), float(kept)], dtype=torch.float64, device=sq.device)

  if U == 0:
    weights[:n] = math.nan
    return weights, info(0, math.inf, -1)
  Dz = torch.where(usable[:, None] & usable[None, :], D, torch.zeros_like(D))  # (rows without weight take no part)

  def evaluate(c):  # (tau, lambda) of E(c), None when degenerate
    C = c.sum()
    live = c > 0
    r = torch.where(live, (Dz @ c) / C, torch.zeros_like(c))
    s = (c * r).sum() / C
    key = torch.where(live, c * (r - 0.5 * s), torch.zeros_like(c)).clamp_min(0.0)
    top = key.max()
    if not float(top) > 0:
      return None
    first = int((key == top).nonzero()[0])
    sc = c.sqrt()
    z = torch.zeros_like(c)
    z[first] = sc[first]

    def kz(z):
      Z = z.sum()
      return torch.where(live, -0.5 * (Dz @ z - r * Z - (r * z).sum() + s * Z), torch.zeros_like(c))

    for _ in range(power_iters):
      w = sc * kz(z) / C
      norm = float((w * w).sum().sqrt())
      if not (0 < norm < math.inf):
        break
      z = sc * (w / norm)
    q = kz(z)
    zq = float((z * q).sum())
    if not zq > 0:
      return None
    tau = torch.where(live, q * q, torch.zeros_like(q))
    return torch.where(torch.isnan(tau), torch.full_like(tau, math.inf), tau), float((c * q * q).sum() / (C * zq))

  c = usable.to(torch.float64)
  best, lam_best, kept, rounds = c / U, math.inf, -1, 0
  if mode == "caf":
    for rnd in range(n):
      C = float(c.sum())
      if not C > n - 2 * count:
        break
      ev = evaluate(c)
      if ev is None:
        break
      tau, lam = ev
      rounds = rnd + 1
      if lam < lam_best:
        best, lam_best, kept = c / C, lam, rnd
      tmax = float(tau.max())
      if not tmax > 0:
        break
      ratio = torch.where(tau == tmax, torch.ones_like(tau), tau / tmax)
      c = torch.where(c > 0, c * (1.0 - ratio), torch.zeros_like(c))
  else:
    ev = evaluate(c)
    tau = torch.zeros_like(c)
    if ev is not None:
      tau, lam_best, kept, rounds = ev[0], ev[1], 0, 1
    drop = max(0, count - (n - U))
    idx = torch.arange(n, device=sq.device)
    ahead = usable[None, :] & ((tau[None, :] > tau[:, None]) | ((tau[None, :] == tau[:, None]) & (idx[None, :] > idx[:, None])))
    keep = usable & (ahead.sum(dim=1) >= drop)
    best = keep.to(torch.float64) / (U - drop)
  weights[:n] = best
  return weights, info(rounds, lam_best, kept)


def _weighted_sum_torch(points, weights):
  """bm_weighted_sum in plain torch, accumulated in fp64: rows that are one tensor once, with their weights added; rows
  of weight 0 are not read; a NaN weight gives NaN everywhere."""
  w = weights[:len(points)].tolist()
  if any(math.isnan(x) for x in w):
    return torch.full_like(points[0], math.nan)
  groups = {}
  for p, x in zip(points, w):
    groups.setdefault(id(p), [p, 0.0])[1] += x
  acc = torch.zeros(points[0].shape, dtype=torch.float64, device=points[0].device)
  for p, x in groups.values():
    if x != 0.0:
      acc.add_(p.double(), alpha=x)
  return acc.to(points[0].dtype)


def _nnm_masks_torch(sq, n, f):
  """bm_nnm_masks in plain torch (fp64 ranking, where `sq` lives) for a backend without the kernel: row i and the
  n - f - 1 other rows of smallest distance, ties to the lower index, NaN last (a stable sort) — int64[MAX_ROWS]."""
  D = sq[:n, :n].to(torch.float64)
  words = []
  for i in range(n):
    others = [j for j in range(n) if j != i]
    order = torch.sort(D[i, others], stable=True).indices.tolist()  # NaN sorts last, equal keys keep their order
    word = 1 << i
    for t in order[:n - f - 1]:
      word |= 1 << others[t]
    words.append(word - (1 << 64) if word >= (1 << 63) else word)
  return torch.tensor(words + [0] * (_lib.MAX_ROWS - n), dtype=torch.int64, device=sq.device)


def _mix_rows_torch(rows, masks, n_out):
  """bm_mix_rows in plain torch: per output row the sequential fp32 sum, in index order, of the rows in its mask, then
  one division by their count.  A row outside the mask is not touched; an empty mask gives NaN."""
  n = len(rows)
  outs = []
  for word in masks[:n_out].tolist():
    members = [j for j in range(n) if (word >> j) & 1]
    acc = torch.zeros_like(rows[0])
    for j in members:
      acc = acc + rows[j]
    outs.append(acc / torch.tensor(float(len(members)), dtype=rows[0].dtype, device=rows[0].device))
  return outs


def _mask_words(masks, count):
  return [int(w) & ((1 << 64) - 1) for w in masks[:count].tolist()]


def _mixed_sqdist_torch(sq, n_in, masks, n_out):
  """bm_mixed_sqdist for a backend without the kernel: the definition of include/bm_gar.h walked in Python floats (IEEE
  doubles, the sums in the stated order), so the host form's bits — fp64 (n_out, n_out) where `sq` lives.  Reads the
  matrix and the masks on the host."""
  D = sq.reshape(-1)[:n_in * n_in].view(n_in, n_in).tolist()
  words = _mask_words(masks, n_out)
  if any(w >> n_in for w in words):
    raise ValueError(f"mixed_sqdist: a mask has a bit at or above n_in = {n_in}")
  members = [[j for j in range(n_in) if (w >> j) & 1] for w in words]
  Q = [[0.0] * n_out for _ in range(n_in)]
  for i in range(n_in):
    for b in range(n_out):
      s = 0.0
      for j in members[b]:
        if j != i:
          s = s + D[min(i, j)][max(i, j)]
      Q[i][b] = s

  def P(a, b):
    s = 0.0
    for i in members[a]:
      s = s + Q[i][b]
    return s

  diag = [P(a, a) for a in range(n_out)]
  out = [[0.0] * n_out for _ in range(n_out)]
  for a in range(n_out):
    out[a][a] = 0.0 if words[a] else math.nan
    for b in range(a + 1, n_out):
      if not words[a] or not words[b]:
        v = math.nan
      elif words[a] == words[b]:
        v = 0.0
      else:
        x, y = (a, b) if words[a] < words[b] else (b, a)  # the smaller mask word walks the outer sum
        p, cx, cy = P(x, y), float(len(members[x])), float(len(members[y]))
        if not (math.isfinite(p) and math.isfinite(diag[x]) and math.isfinite(diag[y])):
          v = math.nan
        else:
          v = p / (cx * cy) - 0.5 * diag[x] / (cx * cx) - 0.5 * diag[y] / (cy * cy)
          v = 0.0 if v <= 0.0 else v
      out[a][b] = out[b][a] = v
  return torch.tensor(out, dtype=torch.float64, device=sq.device)


def _mix_weights_torch(masks, n_in, n_out, weights=None, selection=None, m=None):
  """bm_mix_weights for a backend without the kernel, in Python floats: the host form's bits — fp64[MAX_ROWS] where the
  weights / the selection live."""
  given = weights if weights is not None else selection
  words = _mask_words(masks, n_out)
  if any(w >> n_in for w in words):
    raise ValueError(f"mix_weights: a mask has a bit at or above n_in = {n_in}")
  ok = True
  if selection is not None:
    sel = [int(t) for t in selection[:m].tolist()]
    ok = all(0 <= t < n_out for t in sel)
    w = [0.0] * n_out
    if ok:
      for t in sel:
        w[t] = w[t] + 1.0 / float(m)
  else:
    w = weights[:n_out].tolist()
  ok = ok and all(w[r] == 0.0 or words[r] for r in range(n_out))
  out = [0.0] * _lib.MAX_ROWS
  for j in range(n_in):
    s = 0.0
    for r in range(n_out):
      if w[r] != 0.0 and (words[r] >> j) & 1:
        s = s + w[r] / float(bin(words[r]).count("1"))
    out[j] = s if ok else math.nan
  return torch.tensor(out, dtype=torch.float64, device=given.device)


class ShardedAggregator:
  """Aggregation rules over gradients whose coordinates are sharded across the ranks of `group`."""

  def __init__(self, backend=None, group=None, force_collectives=False, native_comm="auto", local_only=False):
    """native_comm: "auto" (default) gives the HIP backend its own RCCL communicator when there is
    more than one rank, so that Multi-Krum / Bulyan are single C calls; False keeps every collective
    in torch.distributed; True insists (raises if RCCL cannot be bound).
    local_only: a single-rank aggregator whatever the state of torch.distributed (the whole vectors are here:
    no collective is ever issued) — e.g. the unsharded reference computation inside a multi-rank job."""
    self.backend = backend if backend is not None else HipBackend()
    self.group = group
    initialised = dist.is_available() and dist.is_initialized() and not local_only
    self.world_size = dist.get_world_size(group) if initialised else 1
    self.rank = dist.get_rank(group) if initialised else 0
    # force_collectives: issue the all-reduce / all-gather calls even with one rank (used to
    # exercise the RCCL path on a single-GPU box); never set in production with world_size 1
    self.collective = self.world_size > 1 or (force_collectives and initialised)
    self.native = None
    self.single_call = isinstance(self.backend, HipBackend) and native_comm is not False
    if self.single_call and self.collective:
      self.native, failure = self._create_native(group)
      if self.native is None:
        if native_comm is True:
          raise RuntimeError(f"libbm_gar RCCL communicator unavailable on at least one rank ({failure})")
        warnings.warn(f"libbm_gar RCCL communicator unavailable ({failure}); using torch.distributed collectives")
        self.single_call = False
    self.brute_status = None
    # (index tensor, count): the rows the latest krum / rule_from_sq("krum") / brute / aksel / cge of THIS aggregator
    # averaged are the first `count` entries of the tensor, which stays where the rule left it (device memory with the
    # HIP backend; after a single-call krum a view of the stream's workspace: read it on that stream before the next
    # sharded rule).  step.AggregationStep counts the Byzantine rows among them (attack.py:822)
    self.last_selection = None
    # the weights of the latest geomed / cclip of THIS aggregator (fp64[MAX_ROWS] where the rule left them) and its
    # info (iterations run, move^2, usable rows)
    self.last_weights = None
    self.last_center_info = None
    self.last_spectral_info = None  # the same for the latest caf / dnc: fp64[4], bm_spectral_weights' info
    self.last_masks = None   # the neighbour masks of the latest nnm of THIS aggregator (int64[MAX_ROWS])
    self._total = None       # (length of the whole vectors, this rank's shard length when it was determined)

  def shard_rows(self, rows, d=None):
    """This rank's slice (shard_bounds) of n whole gradients held on every rank, as `Shards` carrying the total."""
    d = int(rows[0].shape[0]) if d is None else int(d)
    lo, hi = shard_bounds(d, self.world_size, self.rank)
    return Shards([r[lo:hi] for r in rows], d_total=d)

  def _total_of(self, local, d_total=None):
    """Total length for a distance pass over `local`: stated, else carried by the shards, else `total_length`."""
    if d_total is None:
      d_total = getattr(local, "d_total", None)
    return self.total_length(local[0].numel(), d_total)

  def total_length(self, d_local, d_total=None):
    """Length of the WHOLE vectors (all shards), the number every rank must hand to the distance pass so that a
    short or empty trailing shard plans it exactly like its peers (bm_gar.h, bm_sharded_krum).

    Stated by the caller (`d_total`, or carried by `Shards`: to_dim_sharded / shard_rows), or, for plain lists,
    determined ONCE per aggregator: the first call sums the shard lengths over
    the ranks (one tiny all-reduce, which every rank enters because every rank makes its first call), later calls
    return that number without any communication.  An aggregator therefore serves ONE vector length; a rank that
    notices another shard length raises instead of guessing — deciding locally whether to repeat the collective could
    leave ranks whose shard length did not change outside of it (a hang).  For another length pass `d_total`, call
    `reset_total_length()` on every rank, or use another aggregator."""
    if d_total is not None:
      return int(d_total)
    if not self.collective:
      return int(d_local)
    if self._total is None:
      self._total = (int(self.backend.sum_over_ranks(self, int(d_local))), int(d_local))
    elif self._total[1] != int(d_local):
      raise ValueError(f"this ShardedAggregator determined the total length {self._total[0]} from shards of "
                       f"{self._total[1]} coordinates and is now given a shard of {d_local}: pass d_total=, or call "
                       f"reset_total_length() on every rank")
    return self._total[0]

  def reset_total_length(self):
    """Forget the total length (collective-free; the next distance pass determines it again, on every rank)."""
    self._total = None

  def _create_native(self, group):
    """The library's own communicator, on EVERY rank or on none: a rank that fell back alone would issue
    torch.distributed collectives while its peers wait inside RCCL calls of the other communicator (a hang,
    not a degradation).  Every step of the bootstrap that can fail locally is followed by a vote (MIN over the
    ranks of a success flag, through the torch group that is known to work); the unique id is only
    broadcast, and bm_comm_init only entered, when every rank can go on."""
    lib = _lib.load()

    def everyone(ok):
      flag = torch.tensor([1.0 if ok else 0.0], dtype=torch.float32,
                          device=torch.device("cuda", torch.cuda.current_device()))
      dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
      return flag.item() >= 1.0

    if not everyone(bool(lib.bm_comm_available())):
      return None, "RCCL could not be bound by libbm_gar.so"
    comm, failure = None, None
    try:
      comm = NativeComm(group, vote=everyone)  # (votes once inside: "rank 0 has an id", before the id is broadcast)
    except Exception as err:  # noqa: BLE001
      failure = err
    if not everyone(comm is not None):
      if comm is not None:
        comm.close()
      return None, failure if failure is not None else "bm_comm_init failed on another rank"
    return comm, None

  # -- collectives (never called when world_size == 1) ----------------------- #
  # Every exchange of this class goes through the three primitives below (a subclass may route them elsewhere:
  # tests/test_gpu_zz_multirank.py stages them through host tensors to run several ranks on ONE GPU over gloo).

  def _all_reduce(self, tensor, op=None):
    if self.collective:
      dist.all_reduce(tensor, op=(op or dist.ReduceOp.SUM), group=self.group)
    return tensor

  def _all_gather_into(self, everyone, mine):
    dist.all_gather_into_tensor(everyone, mine, group=self.group)

  def _all_to_all(self, recv, send):
    dist.all_to_all_single(recv, send, group=self.group)

  def all_reduce_sum(self, tensor):
    """In-place sum over the ranks of a small device tensor (no-op with one rank)."""
    return self._all_reduce(tensor)

  def exchange(self, sums, maxes):
    """ONE collective for every scalar of a step: each rank contributes [sums | maxes] (fp64), an
    all-gather hands every rank all contributions, which it reduces itself in rank order — sums and
    (NaN-propagating) maxima from the same message, bitwise identical on every rank."""
    if not self.collective:
      return sums, maxes
    ns = sums.shape[0]
    mine = torch.cat([sums, maxes]).contiguous()
    everyone = torch.empty(self.world_size * mine.shape[0], dtype=mine.dtype, device=mine.device)
    self._all_gather_into(everyone, mine)
    everyone = everyone.view(self.world_size, -1)
    total = everyone[0, :ns].clone()
    for r in range(1, self.world_size):
      total += everyone[r, :ns]
    return total, everyone[:, ns:].max(dim=0).values

  def all_gather_output(self, local_out, d):
    """Full d-vector on every rank from the per-rank slices (shard_bounds layout)."""
    if not self.collective:
      return local_out
    lo0, hi0 = shard_bounds(d, self.world_size, 0)
    per = hi0 - lo0
    padded = torch.zeros(per, dtype=local_out.dtype, device=local_out.device)
    padded[:local_out.shape[0]] = local_out
    full = torch.empty(per * self.world_size, dtype=local_out.dtype, device=local_out.device)
    self._all_gather_into(full, padded)
    return full[:d]

  def to_dim_sharded(self, my_gradients, n, d, dtype=torch.float32, device=None):
    """Worker-major -> dimension-major in ONE all-to-all (the step before the
    path when the honest gradients are PRODUCED in parallel, experiments/model.py:333-366 run once per
    worker).  `my_gradients`: the full-length gradients of owned_workers(n, P, rank), in that order.
    Returns the n gradients restricted to this rank's coordinate slice (shard_bounds), in worker order, as `Shards`
    (they carry d, so the distance-based rules need neither a d_total argument nor a collective to learn it):
    views into one receive buffer, 256-byte aligned, ready for the rules.  Each rank sends (P-1)/P of
    what it produced — n/P * d * 4 bytes spread over the P-1 peers' links at once — never more."""
    world, rank = self.world_size, self.rank
    mine = owned_workers(n, world, rank)
    if len(my_gradients) != len(mine):
      raise ValueError(f"rank {rank} must pass the gradients of workers {mine}")
    if not self.collective:  # (one rank with forced collectives still goes through the exchange: that is how a
      return Shards(my_gradients, d_total=d)  #  single-GPU box exercises the RCCL all-to-all)
    per = -(-(-(-d // world)) // 64) * 64    # padded shard length: ceil(d / P) rounded up to 64 coordinates (256 B)
    n_max = -(-n // world)
    # a rank that owns no worker (n < P) still takes part in the exchange with an all-zero send buffer:
    # dtype / device come from its gradients when it has some, else from the arguments
    if my_gradients:
      dtype, device = my_gradients[0].dtype, my_gradients[0].device
    elif device is None:
      device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    send = torch.zeros((world, n_max, per), dtype=dtype, device=device)
    for j, g in enumerate(my_gradients):
      full = g.shape[0] // per
      send[:full, j, :] = g[:full * per].view(full, per)
      if full < world and g.shape[0] > full * per:
        send[full, j, :g.shape[0] - full * per] = g[full * per:]
    recv = torch.empty_like(send)
    self._all_to_all(recv.view(-1), send.view(-1))
    lo, hi = shard_bounds(d, world, rank)
    return Shards([recv[i % world, i // world, :hi - lo] for i in range(n)], d_total=d)

  # -- rules ------------------------------------------------------------------ #

  def median(self, local):
    return self.backend.colwise("median", local, 0)

  def trmean(self, local, f):
    return self.backend.colwise("trmean", local, f)

  def phocas(self, local, f):
    return self.backend.colwise("phocas", local, f)

  def meamed(self, local, f):
    return self.backend.colwise("meamed", local, f)

  def global_sqdist(self, local, d_total=None):
    """All-reduced n x n squared-distance matrix (every rank gets the same bits: the sum runs over
    the same P partial matrices in the collective's fixed order)."""
    # the precision plan follows the length of the whole vectors, the same number on every rank (total_length)
    sq = self.backend.pairwise_sqdist(local, d_total=self._total_of(local, d_total))  # fresh, reduced in place
    self._all_reduce(sq)
    return sq

  def krum(self, local, f, m=None, d_total=None):
    n = len(local)
    if m is None:
      m = n - f - 2
    if self.single_call:
      out, order = self.backend.sharded_rule("krum", self.native, local, f, m, self._total_of(local, d_total),
                                             with_order=True)
      self.last_selection = (order, m)
      return out
    order = self.backend.rank(self.global_sqdist(local, d_total), n, f, m, _lib.RANK_KRUM)
    self.last_selection = (order, m)
    return self.backend.selected_mean(local, order, m)

  def bulyan(self, local, f, m=None, d_total=None):
    n = len(local)
    if m is None:
      m = n - f - 2
    if self.single_call:
      return self.backend.sharded_rule("bulyan", self.native, local, f, m, self._total_of(local, d_total))
    order = self.backend.rank(self.global_sqdist(local, d_total), n, f, m, _lib.RANK_BULYAN)
    return self.backend.bulyan_pass2(local, order, f, m)

  def rule_from_sq(self, name, local, local_sq, f, m=None):
    """Multi-Krum / Bulyan when the squared distances of the local shard are already known (the first pass of a step
    produced them, stats.momentum_stats_sqdist): all-reduce, rank, average / pass 2."""
    n = len(local)
    if m is None:
      m = n - f - 2
    sq = self._all_reduce(local_sq)  # in place: a fresh tensor per call
    order = self.backend.rank(sq, n, f, m, _lib.RANK_KRUM if name == "krum" else _lib.RANK_BULYAN)
    if name == "krum":
      self.last_selection = (order, m)
      return self.backend.selected_mean(local, order, m)
    return self.backend.bulyan_pass2(local, order, f, m)

  def aksel(self, local, f, mode="mid"):
    n = len(local)
    count = (n + 1) // 2 if mode == "mid" else n - f
    sq = self.backend.aksel_sqdist(local)
    self._all_reduce(sq)
    order = self.backend.argsort(sq, n)
    self.last_selection = (order, count)
    return self.backend.selected_mean(local, order, count)

  def brute(self, local, f, d_total=None, check=False):
    """Brute rule: all-reduced distances, then the (deterministic) subset search on every rank — on the device with
    the HIP backend (same bits in, same selection out on every rank, no host round trip).  The search's status is
    kept in `self.brute_status` (device int32[1]) — per aggregator, not per process.  Unchecked, a search without a
    usable answer shows in the result (status -1: non-finite where a bad gradient is; -2, the node budget: NaN
    everywhere).  check=True reads the status here (one 4-byte synchronisation; every rank holds the same status, the
    search being a function of the all-reduced matrix): -1 raises like the reference (brute.py:68), -2 repeats the
    search on the host, which has no budget — AggregationStep does this before it hands out the defense vector."""
    n = len(local)
    sq = self.global_sqdist(local, d_total)
    if hasattr(self.backend, "brute_select_device"):
      sel, self.brute_status = self.backend.brute_select_device(sq, n, f)
      if check and not (sq.is_cuda and torch.cuda.is_current_stream_capturing()):
        code = int(self.brute_status.item())
        if code == -2:
          host = self.backend.brute_select(sq.sqrt().cpu().contiguous(), n, f)
          sel = self.backend.index_tensor(host, local[0])
          self.brute_status = None
        elif code != 0:
          from . import gars
          raise RuntimeError(gars.BRUTE_NO_SUBSET)
      self.last_selection = (sel, n - f)  # (after a host re-search: the subset that is averaged, not the device's)
      return self.backend.selected_mean(local, sel, n - f)
    self.brute_status = None
    sel = self.backend.index_tensor(self.backend.brute_select(sq.sqrt().cpu().contiguous(), n, f), local[0])
    self.last_selection = (sel, n - f)
    return self.backend.selected_mean(local, sel, n - f)

  def check_brute(self):
    """Raise when the latest unchecked brute() of THIS aggregator had no usable answer (-1: the reference's assertion,
    brute.py:68; -2: the node budget); syncs."""
    status = getattr(self, "brute_status", None)
    if status is not None:
      from . import gars
      gars.brute_check(status)

  def average(self, local):
    n = len(local)
    return self.backend.selected_mean(local, self.backend.index_tensor(list(range(n)), local[0]), n)

  def cge(self, local, f):
    n = len(local)
    sq = self.backend.row_sqnorms(local)
    self._all_reduce(sq)
    order = self.backend.argsort(sq, n)
    self.last_selection = (order, n - f)
    return self.backend.selected_mean(local, order, n - f)

  def _center(self, mode, local, param, iters, tol, start, d_total):
    """The geometric median / centered clipping of the local slice: (1) the squared distances of rows + [start],
    all-reduced — the one collective, N x N doubles; (2) the weights of the iterate, every rank from the same matrix:
    the same bits; (3) the weighted sum of the local slice.  No host synchronisation and no d-sized collective,
    whatever `iters` is.  A backend that declares the "center_weights" / "weighted_sum" capabilities runs (2) / (3) as
    kernels; any other gets the same steps in plain torch, in fp64."""
    from . import gars
    gars.check_center_args(mode, param, iters, tol)
    rows = list(local)
    points = rows + ([start] if start is not None else [])
    if not rows or len(points) > _lib.MAX_ROWS:
      raise gars.GarInputError(f"{mode}: 1..{_lib.MAX_ROWS} gradients are supported"
                               f"{' (one fewer with a start vector)' if start is not None else ''}, got {len(rows)}")
    caps = getattr(self.backend, "capabilities", ())
    sq = self.global_sqdist(points, self._total_of(local, d_total))
    args = (sq, len(rows), mode, param, iters, tol, start is not None)
    weights, info = self.backend.center_weights(*args) if "center_weights" in caps else _center_weights_torch(*args)
    self.last_weights, self.last_center_info = weights, info
    if "weighted_sum" in caps:
      return self.backend.weighted_sum(points, weights)
    return _weighted_sum_torch(points, weights)

  def geomed(self, local, f=None, nu=1e-6, iters=8, tol=0.0, d_total=None):
    """The geometric median by `iters` smoothed Weiszfeld iterations from the mean of the rows (gars.geomed).
    `self.last_weights` keeps the weights (device fp64[MAX_ROWS]: the n weights, then zeros).  f is ignored."""
    return self._center("geomed", local, nu, iters, tol, None, d_total)

  def cclip(self, local, f=None, tau=None, iters=3, tol=0.0, start=None, d_total=None):
    """Centered clipping from `start` (this rank's slice of it; None: the mean of the rows), gars.cclip.
    `self.last_weights` keeps the weights, the start's being entry n.  tau is required; f is ignored."""
    if tau is None:
      raise ValueError("cclip: tau (the clipping radius) is required")
    return self._center("cclip", local, tau, iters, tol, start, d_total)

  def _spectral(self, mode, local, count, power_iters, d_total):
    """CAF / DnC of the local slice, as `_center`: (1) the squared distances of the rows, all-reduced — the one
    collective; (2) the weights of the filter, every rank from the same matrix: the same bits; (3) the weighted sum of
    the local slice.  A backend that declares the "spectral_weights" / "weighted_sum" capabilities runs (2) / (3) as
    kernels; any other gets the same steps in plain torch, in fp64."""
    from . import gars
    rows = list(local)
    if not rows or len(rows) > _lib.MAX_ROWS:
      raise gars.GarInputError(f"{mode}: 1..{_lib.MAX_ROWS} gradients are supported, got {len(rows)}")
    gars.check_spectral_args(mode, len(rows), count, power_iters)
    caps = getattr(self.backend, "capabilities", ())
    sq = self.global_sqdist(rows, self._total_of(local, d_total))
    args = (sq, len(rows), mode, count, power_iters)
    weights, info = (self.backend.spectral_weights(*args) if "spectral_weights" in caps
                     else _spectral_weights_torch(*args))
    self.last_weights, self.last_spectral_info = weights, info
    if "weighted_sum" in caps:
      return self.backend.weighted_sum(rows, weights)
    return _weighted_sum_torch(rows, weights)

  def caf(self, local, f, power_iters=16, d_total=None):
    """CAF (gars.caf) on this rank's slice.  `self.last_weights` keeps the weights (fp64[MAX_ROWS]: the n weights, then
    zeros), `self.last_spectral_info` the four numbers of bm_spectral_weights."""
    return self._spectral("caf", local, f, power_iters, d_total)

  def dnc(self, local, f, c=1.0, power_iters=16, d_total=None):
    """DnC (gars.dnc) on this rank's slice: the k = min(ceil(c f), n - 1) rows of largest squared projection removed."""
    if isinstance(f, bool) or not isinstance(f, int) or f < 0:
      raise ValueError(f"dnc: f must be an integer >= 0, got {f!r}")
    if isinstance(c, bool) or not isinstance(c, (int, float)) or not (0 <= c < float("inf")):
      raise ValueError(f"dnc: c must be a finite number >= 0, got {c!r}")
    k = min(int(math.ceil(c * f)), max(len(local) - 1, 0))
    return self._spectral("dnc", local, k, power_iters, d_total)

  NNM_RULES = ("median", "trmean", "phocas", "meamed", "krum", "bulyan", "brute", "aksel", "cge", "average", "geomed",
               "cclip", "caf", "dnc")

  SCALAR_RULES = ("krum", "brute", "geomed", "cclip", "average")

  def _nnm_scalars(self, rows, f, rule, total, rule_args):
    """form="scalars" of nnm: (1) the squared distances of the rows (+ a cclip start as point n), all-reduced — the ONE
    collective; (2) on every rank from that matrix, hence with the same bits: the neighbour masks, the distances
    between the mixed rows (mixed_sqdist), the rule's scalar stage, the weights of the original rows (mix_weights);
    (3) the weighted sum of the local slice.  No mixed row is written and no second matrix is reduced.  A backend that
    declares the "mixed_sqdist" / "mix_weights" capabilities runs those as kernels; any other gets them in plain
    Python floats (fp64, the host form's bits)."""
    from . import gars
    caps = getattr(self.backend, "capabilities", ())
    n = len(rows)
    args = dict(rule_args)
    args.pop("d_total", None)
    start, mode = None, rule if rule in ("geomed", "cclip") else None
    if mode == "geomed":
      param, iters = args.pop("nu", 1e-6), args.pop("iters", 8)
    elif mode == "cclip":
      param, iters, start = args.pop("tau", None), args.pop("iters", 3), args.pop("start", None)
      if param is None:
        raise ValueError("cclip: tau (the clipping radius) is required")
    if mode is not None:
      tol = args.pop("tol", 0.0)
      gars.check_center_args(mode, param, iters, tol)
    points = rows + ([start] if start is not None else [])
    N = len(points)
    if N > _lib.MAX_ROWS:
      raise gars.GarInputError(f"cclip: at most {_lib.MAX_ROWS - 1} gradients are supported with a start vector, got {n}")
    sq = self.global_sqdist(points, total)
    sub = sq if start is None else sq[:n, :n].contiguous()
    masks = self.backend.nnm_masks(sub, n, f) if "nnm_masks" in caps else _nnm_masks_torch(sub, n, f)
    self.last_masks = masks
    if start is not None:  # the start is point n and mixed row n, alone in its mask
      own = torch.full((1,), (1 << n) - (1 << 64 if n == 63 else 0), dtype=torch.int64, device=masks.device)
      masks = torch.cat((masks[:n], own))
    mixed_leg = self.backend.mixed_sqdist if "mixed_sqdist" in caps else _mixed_sqdist_torch
    weights_leg = self.backend.mix_weights if "mix_weights" in caps else _mix_weights_torch
    if rule == "average":
      even = torch.full((_lib.MAX_ROWS,), 1.0 / n, dtype=torch.float64, device=sq.device)
      w = weights_leg(masks, N, n, weights=even)
    else:
      mixed = mixed_leg(sq, N, masks, N)
      if rule == "krum":
        m = args.pop("m", None)
        if m is None:
          m = n - f - 2
        order = self.backend.rank(mixed, n, f, m, _lib.RANK_KRUM)
        self.last_selection = (order, m)
        w = weights_leg(masks, N, n, selection=order, m=m)
      elif rule == "brute":
        check = args.pop("check", False)
        if hasattr(self.backend, "brute_select_device"):
          sel, self.brute_status = self.backend.brute_select_device(mixed, n, f)
          if check and not (mixed.is_cuda and torch.cuda.is_current_stream_capturing()):
            code = int(self.brute_status.item())
            if code == -2:
              sel = self.backend.index_tensor(self.backend.brute_select(mixed.sqrt().cpu().contiguous(), n, f), rows[0])
              self.brute_status = None
            elif code != 0:
              raise RuntimeError(gars.BRUTE_NO_SUBSET)
        else:
          self.brute_status = None
          sel = self.backend.index_tensor(self.backend.brute_select(mixed.sqrt().cpu().contiguous(), n, f), rows[0])
        self.last_selection = (sel, n - f)
        w = weights_leg(masks, N, n, selection=sel, m=n - f)
      else:
        cargs = (mixed, n, mode, param, iters, tol, start is not None)
        cw, info = self.backend.center_weights(*cargs) if "center_weights" in caps else _center_weights_torch(*cargs)
        self.last_center_info = info
        w = weights_leg(masks, N, N, weights=cw)
    self.last_weights = w  # of the ORIGINAL rows (and the start): what the weighted sum reads
    if "weighted_sum" in caps:
      return self.backend.weighted_sum(points, w)
    return _weighted_sum_torch(points, w)

  def nnm(self, local, f, rule="trmean", d_total=None, form="rows", **rule_args):
    """Nearest-neighbour mixing, then `rule` on the mixed rows (gars.nnm), on this rank's slice: (1) the squared
    distances, all-reduced — the neighbours are those of the WHOLE vectors, the same masks on every rank; (2) mixing and
    a coordinate-wise rule are column-local: the fused kernel for median / trmean where the backend has it, else the
    mixed slice is written and the aggregator's own rule runs on it (a distance-based rule then all-reduces the
    distances of the mixed rows).  A backend that declares the "nnm_masks" / "mix_rows" / "colwise_mixed" capabilities
    runs the kernels; any other gets the same steps in plain torch (fp64 ranking, sequential fp32 sums).
    `self.last_masks` keeps the masks (int64[MAX_ROWS]).
    form="scalars" (krum, brute, geomed, cclip, average; any other rule raises ValueError): `_nnm_scalars` — ONE
    all-reduce, no mixed row; it also leaves `last_weights` (the weights of the original rows) and, for krum and brute,
    `last_selection`."""
    from . import gars
    if rule not in self.NNM_RULES:
      raise ValueError(f"nnm: unknown rule {rule!r} ({', '.join(sorted(self.NNM_RULES))})")
    if form not in ("rows", "scalars"):
      raise ValueError(f"nnm: unknown form {form!r} (rows, scalars)")
    if form == "scalars" and rule not in self.SCALAR_RULES:
      raise ValueError(f"nnm: form='scalars' serves {', '.join(self.SCALAR_RULES)} only, got rule {rule!r}")
    rows = list(local)
    n = len(rows)
    if not 1 <= n <= _lib.MAX_ROWS or not 0 <= f < n:
      raise gars.GarInputError(f"nnm: 1 <= n <= {_lib.MAX_ROWS} and 0 <= f < n are needed, got n = {n}, f = {f}")
    caps = getattr(self.backend, "capabilities", ())
    total = self._total_of(local, d_total)
    if form == "scalars":
      return self._nnm_scalars(rows, f, rule, total, rule_args)
    sq = self.global_sqdist(rows, total)
    masks = self.backend.nnm_masks(sq, n, f) if "nnm_masks" in caps else _nnm_masks_torch(sq, n, f)
    self.last_masks = masks
    if (rule in ("median", "trmean") and not rule_args and "colwise_mixed" in caps
        and n <= self.backend.colwise_mixed_max_rows()):
      return self.backend.colwise_mixed(rule, rows, masks, f if rule == "trmean" else 0)
    mixed = self.backend.mix_rows(rows, masks, n) if "mix_rows" in caps else _mix_rows_torch(rows, masks, n)
    mixed = Shards(mixed, d_total=total)
    fn = getattr(self, rule)
    if rule in ("median", "average"):
      return fn(mixed, **rule_args)
    if rule in ("krum", "bulyan", "brute", "geomed", "cclip", "caf", "dnc"):
      rule_args.setdefault("d_total", total)
    return fn(mixed, f, **rule_args)

  def anticge(self, local_honests, f_decl, f_real):
    """The reference's `anticge` attack (attacks/anticge.py:49-78) on this rank's slice of the honest gradients:
    `f_real` references to ONE new vector.  Row norms -> all-reduce -> rank and sum the selected rows -> all-reduce of
    the ONE scalar |S|^2 -> scale: two small collectives, never a d-sized one, none with one rank.  A backend that
    declares the "anticge" capability runs the two legs as kernels (HipBackend.anticge); any other gets
    the same steps in plain torch over its `row_sqnorms` and `argsort` legs."""
    local = list(local_honests)
    h = len(local)
    if f_real <= 0:
      return []
    if f_real > f_decl:  # anticge.py:60-63: a Byzantine gradient is selected whatever it is
      return [torch.full_like(local[0], math.nan)] * f_real
    if not 1 <= f_decl <= h:
      raise ValueError(f"anticge needs 1 <= f_decl <= {h} honest gradients, got f_decl = {f_decl}")
    if "anticge" in getattr(self.backend, "capabilities", ()):
      return [self.backend.anticge(local, f_decl, self._all_reduce)] * f_real
    byz, _, scal = _anticge_sum_torch(self.backend, local, f_decl, self._all_reduce(self.backend.row_sqnorms(local)))
    self._all_reduce(scal[:1])
    return [_anticge_scale_torch(byz, scal)] * f_real

  def minmax(self, local_honests, f_real, mode="minmax", perturbation="std", d_total=None):
    """The Min-Max ("minmax") / Min-Sum ("minsum") attack of Shejwalkar & Houmansadr (NDSS 2021) on this rank's slice of
    the honest gradients (stats.minmax_attack): `f_real` references to ONE new vector avg + gamma * p.  The h x h squared
    distances and the scalars of the perturbation are both sums over coordinates: they travel through ONE all-reduce,
    h^2 + PERTURB_SLOTS doubles, concatenated — none with one rank, never a d-sized one — and every rank forms gamma
    from the same numbers: the same bits.  A backend that declares the "perturb_stats" / "minmax_factor" capabilities
    runs those legs as kernels and leaves gamma on the device; any other gets plain-torch fp64 legs.  The vector
    carries `.attack_factor` (fp64[1]) and `.attack_info` (fp64[6], bm_minmax_factor's)."""
    if mode not in _lib.MINMAX_MODES:
      raise ValueError(f"unknown mode {mode!r} (one of {sorted(_lib.MINMAX_MODES)})")
    if perturbation not in _lib.PERTURB_KINDS:
      raise ValueError(f"unknown perturbation {perturbation!r} (one of {sorted(_lib.PERTURB_KINDS)})")
    local = list(local_honests)
    h = len(local)
    if not 2 <= h <= _lib.MAX_ROWS:
      raise ValueError(f"the {mode} attack needs 2 <= h <= {_lib.MAX_ROWS} honest gradients, got h = {h}")
    if f_real <= 0:
      return []
    caps = getattr(self.backend, "capabilities", ())
    if "perturb_stats" in caps:
      avg, direction, scal = self.backend.perturb_stats(local, perturbation)
    else:
      avg, direction, scal = _perturb_stats_torch(self.backend, local, perturbation)
    sq = self.backend.pairwise_sqdist(local, d_total=self._total_of(local_honests, d_total))
    if self.collective:
      both = torch.cat([sq.reshape(-1), scal])
      self._all_reduce(both)
      sq, scal = both[:h * h].view(h, h), both[h * h:]
    if "minmax_factor" in caps:
      info = self.backend.minmax_factor(sq, scal, h, mode)
      factor = info  # (read by the kernel where it is)
    else:
      info = _minmax_factor_torch(sq, scal, h, mode)
      factor = info[0].item()
    byz = torch.empty_like(avg)
    self.backend.multi_fma3([byz], [avg], [direction], 1.0, factor)
    byz.attack_factor, byz.attack_info = info[:1], info
    return [byz] * f_real

  def attack_vector(self, kind, local_avg, factor=None, target_idx=None, d_total=None, want_direction=False):
    """This rank's slice of the Byzantine vector of the `nan` / `bulyan` / `empire-strict` attacks from its slice of
    the honest average (stats.attack_vector, bm_attack_vector): kind "nan", "shift_one" (avg + factor * e_target),
    "shift_all" (avg + factor) or "scale" (avg * factor).  factor: a number, or a device float64 tensor.
    target_idx ("shift_one"): a Python index into the WHOLE vector — negative ones count from its end, IndexError
    outside [-d_total, d_total) as indexing raises in the reference.  The rank whose slice (shard_bounds) holds the
    coordinate shifts it; every other rank is told "not here".  No collective — unless the total length is neither
    stated nor carried by the shards (total_length).  want_direction ("shift_*"): returns (vector, direction).
    A backend that declares the "attack_vector" capability runs the kernel; any other gets the same values in plain
    torch."""
    if kind not in _lib.ATTACK_VECTOR_KINDS:
      raise ValueError(f"unknown attack vector kind {kind!r} (one of {sorted(_lib.ATTACK_VECTOR_KINDS)})")
    if want_direction and kind not in ("shift_one", "shift_all"):
      raise ValueError(f"kind {kind!r} has no direction vector")
    target = None
    if kind == "shift_one":
      if not isinstance(target_idx, int) or isinstance(target_idx, bool):
        raise ValueError(f"kind 'shift_one' needs an integer target_idx, got {target_idx!r}")
      total = self.total_length(local_avg.numel(), d_total)
      if not -total <= target_idx < total:
        raise IndexError(f"index {target_idx} is out of bounds for dimension 0 with size {total}")
      lo, hi = shard_bounds(total, self.world_size, self.rank)
      where = target_idx % total
      target = where - lo if lo <= where < hi else -1
    if "attack_vector" in getattr(self.backend, "capabilities", ()):
      return self.backend.attack_vector(kind, local_avg, factor, target, want_direction)
    return _attack_vector_torch(kind, local_avg, factor, target, want_direction)

  def compute_avg_dev_max(self, local_samples):
    """Sharded tools.compute_avg_dev_max: (local slice of the average, norm, deviation, max)."""
    k = len(local_samples)
    if k == 0:
      return None, math.nan, math.nan, math.nan
    avg, out3 = self.backend.stack_stats(local_samples)
    sums, mx = self.exchange(out3[:2], out3[2:])  # one collective (none with a single rank)
    norm2, dev2 = sums.tolist()
    amax = mx.item()
    dev = math.sqrt(dev2 / (k - 1)) if k >= 2 else math.nan
    return avg, math.sqrt(norm2), dev, amax
