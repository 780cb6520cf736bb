"""Timings of the geometric median and centered clipping on one GPU (profiles/center_timings.txt):
  rules    geomed / cclip against Multi-Krum on the same stack, in the same process, alternating, device events;
           next to the ratio the byte counts predict, (N + distinct active rows + 1) / (n + m + 1)
  weights  the weights kernel alone (bm_center_weights_device) at 3, 8, 32 and 64 iterations, 25 and 64 points

    python scripts/center_probe.py [rules] [weights]
"""

import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import byzantinemomentum_amd as bm  # noqa: E402

DEV = torch.device("cuda", 0)
D = 11173962


def stack(n, f, d, seed):
  gen = torch.Generator(device=DEV).manual_seed(seed)
  h = n - f
  mu = 0.1 * torch.randn(d, device=DEV, generator=gen)
  honest = [mu + s * torch.randn(d, device=DEV, generator=gen) for s in torch.linspace(0.5, 1.5, h).tolist()]
  byz = torch.stack(honest).mean(dim=0).mul_(-0.1)   # empire 1.1: f references to one vector
  return honest + [byz] * f


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


def report(name, ms):
  q = statistics.quantiles(ms, n=10)
  print(f"  {name:<24} median {statistics.median(ms) * 1e3:9.1f} us   p10 {q[0] * 1e3:9.1f}   p90 {q[-1] * 1e3:9.1f}   "
        f"min {min(ms) * 1e3:9.1f}   ({len(ms)} runs)")
  return statistics.median(ms), q[-1] - q[0]


def rules():
  for n, f in ((25, 5), (51, 12)):
    rows = stack(n, f, D, seed=n)
    m = n - f - 2
    tau = 0.5 * math.sqrt(D)
    start = torch.stack(rows[:n - f]).mean(dim=0)
    calls = {
      "krum": lambda: (bm.gars.invalidate_rank_cache(), bm.krum(rows, f))[1],
      "geomed (8 iterations)": lambda: bm.geomed(rows, f),
      "cclip (3 it., no start)": lambda: bm.cclip(rows, f, tau=tau),
      "cclip (3 it., start)": lambda: bm.cclip(rows, f, tau=tau, start=start),
    }
    print(f"n = {n}, f = {f}, d = {D}: {n - f} honest rows + {f} references to one Byzantine vector")
    times = timed(calls, reps=30, warmup=5)
    med = {name: report(name, ms) for name, ms in times.items()}
    krum_ms, krum_spread = med["krum"]
    distinct = n - f + 1
    for name, extra in (("geomed (8 iterations)", 0), ("cclip (3 it., no start)", 0), ("cclip (3 it., start)", 1)):
      expect = (n + extra + distinct + extra + 1) / (n + m + 1)
      print(f"  {name:<24} / krum = {med[name][0] / krum_ms:5.3f}   byte counts: ({n + extra} + {distinct + extra} + 1) / "
            f"({n} + {m} + 1) = {expect:5.3f}   (krum's p90 - p10: {krum_spread / krum_ms:5.3f} of its median)")
    del rows, start
    torch.cuda.empty_cache()


def weights():
  gen = torch.Generator(device=DEV).manual_seed(3)
  for N in (25, 64):
    pts = torch.randn(N, 4099, device=DEV, generator=gen)
    pts[-5:] = pts[-1] + 3.0
    sq = bm.gars.pairwise_sqdist(list(pts))
    print(f"weights kernel, N = {N} points")
    for mode, param in (("geomed", 1e-6), ("cclip", 30.0)):
      calls = {f"{mode} L = {L}": (lambda L=L: bm.gars.center_weights(sq, N, mode, param, L, 0.0)) for L in (3, 8, 32, 64)}
      for name, ms in timed(calls, reps=30, warmup=5).items():
        report(name, ms)


if __name__ == "__main__":
  what = sys.argv[1:] or ["rules", "weights"]
  print(torch.cuda.get_device_name(0))
  if "rules" in what:
    rules()
  if "weights" in what:
    weights()
