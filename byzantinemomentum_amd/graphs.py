"""HIP graphs of host-mirror calls, for the launch-bound regime.

On one GPU a rule is two or three kernels of 150-400 us each and the launches hide behind them.  A rank of an
8-GPU job runs the same sequence on 1/8 of the coordinates: at C4 (Bulyan, n = 25, d = 11.2 M / 8) six launches
of 5-25 us each plus the n x n all-reduce, 73-78 us of which about 30 are gaps between dependent launches
(profiles/r03_e_per_rank_p8.txt).  When the row buffers of the stack stay where they are from one
aggregation to the next — momentum buffers do (attack.py:676), and a loop that writes its gradients into fixed
buffers has the same property — the whole sequence, collective included, can be recorded once into a HIP graph and
replayed: one submission per aggregation, the kernel arguments (the by-value row table of every kernel, include/
bm_gar.h) frozen at the recorded addresses.

    g = GraphedCall(lambda: aggregator.bulyan(rows, f))   # records: rows are the buffers every replay will read
    out = g()                                             # replays on the current stream; `out` is the SAME tensor
                                                          # each time (consume or copy it before the next replay)

What a replay does NOT do is run the Python of the call again: the shapes, the rule's arguments and the addresses
are those of the recording.  Contents may change freely; a stack at other addresses needs its own GraphedCall.

`fn` must not synchronise with the host while it is recorded.  Calls that do, and therefore cannot be graphed: the
attacks' factor search against Brute and any search with `line_search="host"` / `"generic"` (a read per evaluation; with
`"auto"` the searches against every other rule keep cursor, ranking and factor on the device), `floats()`, sharded
rules over torch.distributed collectives that stage through the host, and `ShardedAggregator.brute` with a backend
that has no device search (the HIP backend has one, bm_brute_select_device: its brute IS capturable; the status of
the search stays on the device until `check_brute()` / `floats()`).  A failed recording raises GraphCaptureError and
leaves nothing behind.

A graphed `AggregationStep.run()` either IS the eager step at every replay or is refused, on the host, before anything
is launched for it (step.AggregationStep.graph_refusal gives the reason, GraphedCall raises it as GraphCaptureError):
  * what the step keeps from one step to the next must live where the recorded kernels read AND write it.  The momentum
    buffers, the update-placement momentum and the bucketing counter do; the server momentum and cclip's start are
    rebound to the newest defense vector by an eager step, so a step warmed up or recorded here keeps both in buffers of
    its own, filled by one d-sized copy at the end of the step (the defense vector handed out is never written again);
  * `floats()`, `last_factor` and `last_search` cache what they fetched; every replay advances `replay_epoch()`, which
    those caches are keyed on, so they read the device again after a replay and not between two;
  * refused: nb_past > 0 (the deque of past averages, the curvature mode 1 / 2 / 3 and the previous step's norm advance
    in Python: a recording would freeze one of them); a factor search whose cursor is on the host (`line_search="host"`
    / `"generic"`, Brute, Bulyan without the device ranking, and the scalar rules under empire-strict or with more than
    62 honest rows: a read per evaluation, or one per search); bucketing on a backend without the device counter of
    bm_bucket_masks_device (the draw's counter is then a Python integer).
"""

import torch

from . import gars

__all__ = ["GraphedCall", "GraphCaptureError"]


class GraphCaptureError(RuntimeError):
  """`fn` could not be recorded into a HIP graph (it synchronised with the host, a launch failed under capture, or a step
  refused: GraphRefusal)."""


class GraphRefusal(RuntimeError):
  """Raised by a call that knows, on the host and before it launches anything, that a replay of it would not be the call
  (step.AggregationStep.run with a configuration of graph_refusal())."""


_replays = 0    # advanced by every replay of every GraphedCall: what host-side caches of device scalars are keyed on
_preparing = 0  # GraphedCalls between their first warm-up call and the end of their recording


def replay_epoch():
  """A number that changes with every replay (notify_replay): a value fetched from device memory under one epoch says
  nothing under the next."""
  return _replays


def notify_replay():
  """What a replay tells the rest of the package: the recorded kernels may have written anything, so no ranking of
  earlier contents (gars.py) and no scalar fetched earlier (step.AggregationStep.floats / last_factor / last_search)
  survives."""
  global _replays
  gars.invalidate_rank_cache()
  _replays += 1


def capturing():
  """Whether the current stream is recording; False in a process that has no GPU (where the runtime's own question
  raises)."""
  try:
    return bool(torch.cuda.is_current_stream_capturing())
  except RuntimeError:
    return False


def preparing():
  """Whether a GraphedCall is warming its call up or recording it: a step that runs now keeps the state it carries from
  step to step at addresses of its own (module docstring)."""
  return _preparing > 0


class GraphedCall:
  """`fn()` (any call of this package whose tensors live on the current GPU) recorded into a HIP graph.

  A replay runs the recorded kernels, which may write user tensors (a recorded momentum update does) without any
  tensor's version changing: every replay therefore forgets the cached rankings of gars.py, like every other routine of
  the package that writes user tensors.  An eager rule after a replay ranks the contents it finds."""

  def __init__(self, fn, warmup=2):
    global _preparing
    if not torch.cuda.is_available():
      raise RuntimeError("GraphedCall records HIP graphs: it needs the GPU the rows live on")
    _preparing += 1
    try:
      self._prepare(fn, warmup)
    finally:
      _preparing -= 1

  def _prepare(self, fn, warmup):
    self._graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
      # everything the call creates lazily (scratch buffers, the LDS size attribute of a kernel, RCCL channels)
      # must exist before the recording; the ranking cache of gars.py must not turn the recorded call into
      # "reuse the last ranking" (the graph would then hold the averaging kernel alone)
      for _ in range(max(int(warmup), 1)):
        gars.invalidate_rank_cache()
        try:
          fn()
        except GraphRefusal as err:  # (decided before anything was launched: nothing to undo)
          self._graph = None
          raise GraphCaptureError(f"the call refuses to be recorded into a HIP graph: {err}") from err
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gars.invalidate_rank_cache()
    # thread_local: RCCL's helper threads may call the runtime while this thread records
    try:
      with torch.cuda.graph(self._graph, stream=side, capture_error_mode="thread_local"):
        self.output = fn()
    except Exception as err:  # noqa: BLE001
      # nothing of the failed recording may survive: the scratch entries the warm-up created for the side stream (a
      # later stream that maps to the same handle would find them), the ranking cache, the half-built graph
      for key in [k for k in gars._Scratch._cache if k[1] == side.cuda_stream]:
        del gars._Scratch._cache[key]
      gars.invalidate_rank_cache()
      self._graph = None
      torch.cuda.synchronize()
      raise GraphCaptureError(
        "the call could not be recorded into a HIP graph: it must not synchronise with the host while recording "
        "(the attacks' factor search, floats(), host-staged collectives and the sharded brute rule do; see the module "
        f"docstring) — {type(err).__name__}: {err}") from err
    gars.invalidate_rank_cache()  # (the entry the recording left points into the graph's private pool)
    # the scratch buffers the recorded kernels use belong to gars._Scratch, keyed by (device, stream): a later call on
    # a stream that maps to the same handle with another size would replace — and free — them under the graph
    self._scratch = [buf for key, buf in gars._Scratch._cache.items() if key[1] == side.cuda_stream]
    self._stream = side

  def __call__(self):
    notify_replay()  # (the recorded kernels may write anything: no ranking, no fetched scalar of earlier contents survives)
    self._graph.replay()
    return self.output
