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

from . import _lib, gars, pipelines, stats
from .torch_legs import Legs
# the stand-ins lived here before torch_legs.py: their names stay importable from this module for callers that predate it
from .torch_legs import (_anticge_scale_torch, _anticge_sum_torch, _attack_vector_torch,  # noqa: F401
                         _center_weights_torch, _mask_words, _minmax_factor_torch, _mix_rows_torch, _mix_weights_torch,
                         _mixed_sqdist_torch, _nnm_masks_torch, _perturb_stats_torch, _spectral_weights_torch,
                         _weighted_sum_torch)

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
    "mixed_sqdist", "mix_weights", "spectral_weights", "perturb_stats", "minmax_factor", "colwise_bucketed",
    "bucket_masks"))

  def __init__(self):
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

  def colwise_bucketed_supported(self, rule, n, n_out):
    return self.gars.colwise_bucketed_supported(rule, n, n_out)

  def colwise_bucketed(self, rule, gradients, masks, n_out, f):
    return self.gars.colwise_bucketed(rule, gradients, masks, n_out, f)

  def bucket_masks(self, n, s, seed, counter, like):
    """The bucket masks of (n, s, seed, counter) where `like` lives, int64[MAX_ROWS].  counter: a DEVICE int64[1] tensor —
    drawn on the device and advanced there (bm_bucket_masks_device: no synchronisation, a recorded graph draws the next
    permutation at every replay) — or a Python integer: the host form (bm_bucket_masks), copied over."""
    if isinstance(counter, torch.Tensor):
      return self.gars.bucket_masks_device(n, s, seed, counter)
    return self.gars.bucket_masks_host(n, s, seed, counter).to(like.device)

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


class ShardedAggregator:
  """Aggregation rules over gradients whose coordinates are sharded across the ranks of `group`."""

  def __init__(self, backend=None, group=None, force_collectives=False, native_comm="auto", local_only=False):
    """native_comm: "auto" (default) gives the HIP backend its own RCCL communicator when there is
    more than one rank, so that Multi-Krum / Bulyan are single C calls; False keeps every collective
    in torch.distributed; True insists (raises if RCCL cannot be bound).
    local_only: a single-rank aggregator whatever the state of torch.distributed (the whole vectors are here:
    no collective is ever issued) — e.g. the unsharded reference computation inside a multi-rank job."""
    self.backend = backend if backend is not None else HipBackend()
    self.legs = Legs(self.backend)  # every optional leg, the backend's or its plain-torch stand-in: resolved once
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
    self._identity = {}  # (n, device) -> the index table 0 .. n-1 of average()
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
    sel, self.brute_status = pipelines.brute_search(self.legs, self.global_sqdist(local, d_total), n, f, check, local[0])
    self.last_selection = (sel, n - f)  # (after a host re-search: the subset that is averaged, not the device's)
    return self.backend.selected_mean(local, sel, n - f)

  def check_brute(self):
    """Raise when the latest unchecked brute() of THIS aggregator had no usable answer (-1: the reference's assertion,
    brute.py:68; -2: the node budget); syncs."""
    if self.brute_status is not None:
      gars.brute_check(self.brute_status)

  def average(self, local):
    n = len(local)
    # the table 0 .. n-1 is made once per (n, device): a copy from the host per call could not be recorded into a HIP
    # graph (graphs.GraphedCall), and nobody writes it
    key = (n, local[0].device)
    table = self._identity.get(key)
    if table is None:
      table =self._identity[key] = self.backend.index_tensor(list(range(n)), local[0])
    return self.backend.selected_mean(local, table, n)

  def cge(self, local, f):
    n = len(local)
    sq = self.backend.row_sqnorms(local)
    self._all_reduce(sq)
    order = self.backend.argsort(sq, n)
    self.last_selection = (order, n - f)
    return self.backend.selected_mean(local, order, n - f)

  def _center(self, mode, local, param, iters, tol, start, d_total):
    """The geometric median / centered clipping of the local slice (pipelines.center): (1) the squared distances of
    rows + [start], all-reduced — the one collective, N x N doubles; (2) the weights of the iterate, every rank from the
    same matrix: the same bits; (3) the weighted sum of the local slice.  No host synchronisation and no d-sized
    collective, whatever `iters` is.  A backend that declares the "center_weights" / "weighted_sum" capabilities runs
    (2) / (3) as kernels; any other gets the same steps in plain torch, in fp64 (torch_legs)."""
    out, record = pipelines.center(self.legs, lambda points: self.global_sqdist(points, self._total_of(local, d_total)),
                                   mode, local, param, iters, tol, start)
    self.last_weights, self.last_center_info = record.weights, record.info
    return out

  def geomed(self, local, f=None, nu=1e-6, iters=8, tol=0.0, d_total=None):
    """The geometric median by `iters` smoothed Weiszfeld iterations from the mean of the rows (gars.geomed).
    `self.last_weights` keeps the weights (device fp64[MAX_ROWS]: the n weights, then zeros).  f is ignored."""
    return self._center("geomed", local, nu, iters, tol, None, d_total)

  def cclip(self, local, f=None, tau=None, iters=3, tol=0.0, start=None, d_total=None):
    """Centered clipping from `start` (this rank's slice of it; None: the mean of the rows), gars.cclip.
    `self.last_weights` keeps the weights, the start's being entry n.  tau is required; f is ignored."""
    return self._center("cclip", local, tau, iters, tol, start, d_total)

  def _spectral(self, mode, local, count, power_iters, d_total):
    """CAF / DnC of the local slice, as `_center` (pipelines.spectral): (1) the squared distances of the rows,
    all-reduced — the one collective; (2) the weights of the filter, every rank from the same matrix: the same bits;
    (3) the weighted sum of the local slice.  A backend that declares the "spectral_weights" / "weighted_sum"
    capabilities runs (2) / (3) as kernels; any other gets the same steps in plain torch, in fp64 (torch_legs)."""
    out, record = pipelines.spectral(self.legs, lambda rows: self.global_sqdist(rows, self._total_of(local, d_total)),
                                     mode, local, count, power_iters)
    self.last_weights, self.last_spectral_info = record.weights, record.info
    return out

  def caf(self, local, f, power_iters=16, d_total=None):
    """CAF (gars.caf) on this rank's slice.  `self.last_weights` keeps the weights (fp64[MAX_ROWS]: the n weights, then
    zeros), `self.last_spectral_info` the four numbers of bm_spectral_weights."""
    return self._spectral("caf", local, f, power_iters, d_total)

  def dnc(self, local, f, c=1.0, power_iters=16, d_total=None):
    """DnC (gars.dnc) on this rank's slice: the k = min(ceil(c f), n - 1) rows of largest squared projection removed."""
    return self._spectral("dnc", local, pipelines.dnc_count(len(local), f, c), power_iters, d_total)

  NNM_RULES = tuple(pipelines.NNM_RULES)
  SCALAR_RULES = pipelines.SCALAR_RULES

  def _sq_of(self, total, local_sq=None):
    """points -> their all-reduced squared distances, as the pipelines ask for them.  local_sq: this rank's matrix of
    exactly those points, already formed (the first pass of a step): reduced in place, the stand-alone pass skipped.  A
    matrix of another row count is not that of the points asked for (a cclip start adds one) and is left unread."""
    def sq_of(points):
      if local_sq is not None and local_sq.shape[0] == len(points):
        return self._all_reduce(local_sq)
      return self.global_sqdist(points, total)
    return sq_of

  def _nnm_scalars(self, rows, f, rule, total, rule_args, local_sq=None):
    """form="scalars" of nnm (pipelines.on_scalars with the neighbour masks): (1) the squared distances of the rows (+ a
    cclip start as point n), all-reduced — the ONE collective; (2) on every rank from that matrix, hence with the same
    bits: the neighbour masks, the distances between the mixed rows (mixed_sqdist), the rule's scalar stage, the weights
    of the original rows (mix_weights); (3) the weighted sum of the local slice.  No mixed row is written and no second
    matrix is reduced.  A backend that declares the "mixed_sqdist" / "mix_weights" capabilities runs those as kernels;
    any other gets them in plain Python floats (fp64, the host form's bits: torch_legs)."""
    n = len(rows)
    out, record = pipelines.on_scalars(self.legs, self._sq_of(total, local_sq), rows, rule, f, n,
                                       lambda sq: self.legs.nnm_masks(sq, n, f), True, rule_args)
    self.last_masks, self.last_weights = record.masks_made, record.weights
    self._publish(rule, record)
    return out

  def _publish(self, rule, record):
    """What a scalar-form pipeline decided beside its output, where this aggregator keeps it."""
    if record.selection is not None:
      self.last_selection = record.selection
    if rule == "brute":
      self.brute_status = record.brute_status
    if record.info is not None:
      self.last_center_info = record.info

  def nnm(self, local, f, rule="trmean", d_total=None, form="rows", local_sq=None, **rule_args):
    """Nearest-neighbour mixing, then `rule` on the mixed rows (gars.nnm), on this rank's slice: (1) the squared
    distances, all-reduced — the neighbours are those of the WHOLE vectors, the same masks on every rank; (2) mixing and
    a coordinate-wise rule are column-local: the fused kernel for median / trmean where the backend has it, else the
    mixed slice is written and the aggregator's own rule runs on it (a distance-based rule then all-reduces the
    distances of the mixed rows).  A backend that declares the "nnm_masks" / "mix_rows" / "colwise_mixed" capabilities
    runs the kernels; any other gets the same steps in plain torch (fp64 ranking, sequential fp32 sums).
    `self.last_masks` keeps the masks (int64[MAX_ROWS]).
    form="scalars" (krum, brute, geomed, cclip, average; any other rule raises ValueError): `_nnm_scalars` — ONE
    all-reduce, no mixed row; it also leaves `last_weights` (the weights of the original rows) and, for krum and brute,
    `last_selection`.
    local_sq: this rank's n x n squared distances of `local`, where a caller already holds them (the first pass of a
    step, stats.momentum_stats_sqdist): all-reduced IN PLACE as rule_from_sq does, the stand-alone distance pass skipped,
    in either form (form="scalars" with a cclip start needs the start's distances too and runs its own pass)."""
    pipelines.check_rule_form("nnm", rule, form)
    rows = list(local)
    n = len(rows)
    if not 1 <= n <= _lib.MAX_ROWS or not 0 <= f < n:
      raise gars.GarInputError(f"nnm: 1 <= n <= {_lib.MAX_ROWS} and 0 <= f < n are needed, got n = {n}, f = {f}")
    total = self._total_of(local, d_total)
    if form == "scalars":
      return self._nnm_scalars(rows, f, rule, total, rule_args, local_sq)
    masks = self.last_masks = self.legs.nnm_masks(self._sq_of(total, local_sq)(rows), n, f)
    if (rule in ("median", "trmean") and not rule_args and self.legs.colwise_mixed is not None
        and n <= self.backend.colwise_mixed_max_rows()):
      return self.legs.colwise_mixed(rule, rows, masks, f if rule == "trmean" else 0)
    return self._rule_on_rows(rule, Shards(self.legs.mix_rows(rows, masks, n), d_total=total), f, total, rule_args)

  def _rule_on_rows(self, rule, mixed, f, total, rule_args):
    """The aggregator's own `rule` on mixed rows that were written (a distance-based one all-reduces their distances)."""
    fn = getattr(self, rule)
    if rule in ("median", "average"):
      return fn(mixed, **rule_args)
    if rule in ("krum", "bulyan", "brute", "geomed", "cclip", "caf", "dnc"):
      rule_args.setdefault("d_total", total)
    return fn(mixed, f, **rule_args)

  def bucketing(self, local, s, rule, seed=0, counter=None, masks=None, form="rows", d_total=None, local_sq=None,
                **rule_args):
    """Bucketing, then `rule` on the ceil(n / s) bucket means (gars.bucketing), on this rank's slice.  The buckets are
    those of the counter-based draw (bm_bucket_masks: a function of n, s, seed and counter alone, so every rank draws the
    same permutation without a collective) — `counter`: a Python integer, or a DEVICE int64[1] tensor the draw advances
    (HipBackend.bucket_masks) — or `masks`, int64 words where the slice lives, one per bucket (at least ceil(n / s)).
    Mixing and a coordinate-wise rule are column-local: the fused kernel for median / trmean where the backend has an
    instance (bm_colwise_bucketed) and rule_args hold nothing but trmean's `f`, else the means are written and the
    aggregator's own rule runs on them (a distance-based rule then all-reduces the distances of the means).  The rule's f
    goes in rule_args, as with gars.bucketing.  form="scalars" (SCALAR_RULES) goes through pipelines.on_scalars as
    `_nnm_scalars` does: ONE all-reduce (none for "average"), no mean written; `local_sq` as for nnm (read by this form
    alone: form="rows" starts from no distances of the original rows and ignores it).
    `self.last_masks` keeps the masks (int64[MAX_ROWS], or the tensor given)."""
    pipelines.check_rule_form("bucketing", rule, form)
    rows = list(local)
    n, s = len(rows), int(s)
    if not 1 <= n <= _lib.MAX_ROWS or not 1 <= s <= n:
      raise gars.GarInputError(f"bucketing: 1 <= n <= {_lib.MAX_ROWS} and a bucket size within 1..n are needed, got "
                               f"n = {n}, s = {s}")
    n_out = -(-n // s)
    if masks is None:
      if counter is None:
        raise ValueError("bucketing: counter (the draw's counter) or masks is needed")
      masks = self.legs.bucket_masks(n, s, seed, counter, rows[0])
    elif (not isinstance(masks, torch.Tensor) or masks.dtype != torch.int64 or masks.dim() != 1 or masks.numel() < n_out
          or masks.device != rows[0].device):
      raise gars.GarInputError(f"bucketing: masks must be an int64 tensor of at least {n_out} words where the rows live")
    self.last_masks = masks
    total = self._total_of(local, d_total)
    if form == "scalars":
      if pipelines.NNM_RULES[rule] and "f" not in rule_args:
        raise TypeError(f"bucketing: {rule} needs f (the rule's f on the {n_out} bucket means)")
      rule_args = dict(rule_args)
      out, record = pipelines.on_scalars(self.legs, self._sq_of(total, local_sq), rows, rule, rule_args.pop("f", None),
                                         n_out, lambda sq: masks, False, rule_args)
      self.last_weights = record.weights
      self._publish(rule, record)
      return out
    fused_f = None
    if self.legs.colwise_bucketed is not None and rows[0].numel() > 0:
      if rule == "median" and not rule_args:
        fused_f = 0
      elif rule == "trmean" and set(rule_args) == {"f"} and 0 <= 2 * int(rule_args["f"]) < n_out:
        fused_f = int(rule_args["f"])
      if fused_f is not None and not self.backend.colwise_bucketed_supported(rule, n, n_out):
        fused_f = None
    if fused_f is not None:
      return self.legs.colwise_bucketed(rule, rows, masks, n_out, fused_f)
    rule_args = dict(rule_args)
    f = rule_args.pop("f", None)
    mixed = Shards(self.legs.mix_rows(rows, masks, n_out), d_total=total)
    if pipelines.NNM_RULES[rule] and f is None:
      raise TypeError(f"bucketing: {rule} needs f (the rule's f on the {n_out} bucket means)")
    return self._rule_on_rows(rule, mixed, f, total, rule_args)

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
    return [self.legs.anticge(local, f_decl, self._all_reduce)] * f_real

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
    avg, direction, scal = self.legs.perturb_stats(local, perturbation)
    sq = self.backend.pairwise_sqdist(local, d_total=self._total_of(local_honests, d_total))
    if self.collective:
      both = torch.cat([sq.reshape(-1), scal])
      self._all_reduce(both)
      sq, scal = both[:h * h].view(h, h), both[h * h:]
    info = self.legs.minmax_factor(sq, scal, h, mode)
    factor = info if "minmax_factor" in self.legs.native else info[0].item()  # (a kernel reads it where it is)
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
    return self.legs.attack_vector(kind, local_avg, factor, target, want_direction)

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
