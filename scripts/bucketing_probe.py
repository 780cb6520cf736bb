"""Timings of bucketing in front of the coordinate-wise rules and of a step with a pre-aggregation on one GPU
(profiles/bucketing_timings.txt).

Part 1, fused against composed: d = 11 173 962, median and trmean, s = 2 and 3, one tensor per row, both forms in ONE
process on the same stack, alternating, device events, >= 20 timed calls each after warm-up:
  (d) bm_mix_rows + bm_colwise on the bucket means     4 d (n + 2 n_out + 1) bytes
  (e) bm_colwise_bucketed                              4 d (n + 1) bytes
and the spread of a repeated identical series: (d) is timed TWICE per round, (d) and (d'); |median(d) - median(d')| /
median(d) is what the box resolves.  An (n, s) keeps its instance where (e) < (d) by more than that.

Part 2, step time: n = 25, f = 5, d = 36.5 M, worker momentum, empire 1.1, pre in {None, nnm, bucketing s = 2}, rule in
{trmean, krum}, with and without the "sqdist" first pass (a backend without the two fused distance legs).

    python scripts/bucketing_probe.py fused [n ...]
    python scripts/bucketing_probe.py step
"""

import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import byzantinemomentum_amd as bm  # noqa: E402
from byzantinemomentum_amd.sharded import HipBackend, ShardedAggregator  # noqa: E402
from byzantinemomentum_amd.step import AggregationStep  # noqa: E402

DEV = torch.device("cuda", 0)
D = 11173962
D_STEP = 36500000


def stack(n, d, seed):
  gen = torch.Generator(device=DEV).manual_seed(seed)
  mu = 0.1 * torch.randn(d, device=DEV, generator=gen)
  return [mu + s * torch.randn(d, device=DEV, generator=gen) for s in torch.linspace(0.5, 1.5, n).tolist()]


def timed(calls, reps, warmup):
  """Every call of `calls` in turn, `reps` rounds after `warmup` rounds: {name: [ms]}."""
  times = {name: [] for name in calls}
  for r in range(warmup + reps):
    for name, fn in calls.items():
      start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      start.record()
      fn()
      stop.record()
      stop.synchronize()
      if r >= warmup:
        times[name].append(start.elapsed_time(stop))
  return times


def line(name, ms):
  q = statistics.quantiles(ms, n=10)
  med = statistics.median(ms)
  print(f"  {name:<40} median {med * 1e3:9.1f} us   p10 {q[0] * 1e3:9.1f}   p90 {q[-1] * 1e3:9.1f}", flush=True)
  return med


def fused_against_composed(n, d=D):
  rows = stack(n, d, seed=n)
  print(f"n = {n}, d = {d}: one tensor per row")
  for s in (2, 3):
    n_out = -(-n // s)
    masks = bm.gars.bucket_masks_host(n, s, 1, 0).to(DEV)
    for rule in ("median", "trmean"):
      f = 0 if rule == "median" else max((n_out - 1) // 4, 1 if n_out >= 3 else 0)
      plain = (lambda means: bm.gars.median(means)) if rule == "median" else (lambda means: bm.gars.trmean(means, f))
      composed = lambda: plain(bm.gars.mix_rows(rows, masks, n_out))  # noqa: E731
      calls = {"(d)": composed, "(d')": composed}
      have = bm.gars.colwise_bucketed_supported(rule, n, n_out)
      if have:
        calls["(e)"] = lambda: bm.gars.colwise_bucketed(rule, rows, masks, n_out, f)
      times = timed(calls, reps=24, warmup=3)
      print(f" s = {s}, n_out = {n_out}, {rule} (f = {f}): row units composed {n + 2 * n_out + 1}, fused {n + 1}")
      med = {name: line(f"{name} {rule}", ms) for name, ms in times.items()}
      spread = abs(med["(d)"] - med["(d')"]) / med["(d)"]
      if have:
        same = torch.equal(calls["(e)"]().view(torch.int32), composed().view(torch.int32))
        ratio = med["(e)"] / min(med["(d)"], med["(d')"])
        print(f"  fused / composed = {ratio:5.3f}   "
              f"spread of the repeated series {spread:6.4f}   same bits: {same}", flush=True)
      else:
        print(f"  no fused instance   spread of the repeated series {spread:6.4f}", flush=True)
  del rows
  torch.cuda.empty_cache()


class PlainBackend(HipBackend):
  capabilities = HipBackend.capabilities - {"momentum_stats_sqdist", "stack_stats_sqdist"}


def step_times(d=D_STEP, n=25, f=5):
  h = n - f
  sampled = stack(h, d, seed=3)
  print(f"step: n = {n}, f = {f}, d = {d}, worker momentum, empire 1.1; a step and its floats(), medians of 20 after 3")
  for rule in ("trmean", "krum"):
    for pre, pre_args in ((None, None), ("nnm", {}), ("bucketing", dict(s=2))):
      for backend in (HipBackend, PlainBackend):
        step = AggregationStep(n, f, f, gar=rule, momentum_at="worker", attack="empire", attack_factor=1.1, nb_past=0,
                               aggregator=ShardedAggregator(backend=backend(), local_only=True), single_call=False,
                               pre=pre, pre_args=pre_args)

        def one():
          step.run(sampled)
          step.floats()
        ms = timed({"step": one}, reps=20, warmup=3)["step"]
        line(f"{rule:<6} pre={pre!s:<9} first pass {step.plan.first_pass}", ms)
        del step
        torch.cuda.empty_cache()


if __name__ == "__main__":
  print(torch.cuda.get_device_name(0))
  what = sys.argv[1] if len(sys.argv) > 1 else "fused"
  if what == "step":
    step_times()
  else:
    for n in [int(a) for a in sys.argv[2:]] or [11, 25, 36, 51]:
      fused_against_composed(n)
