"""Timings of the spectral filtering rules CAF and DnC on one GPU (profiles/spectral_timings.txt):
  weights  the weights kernel alone (bm_spectral_weights_device) at 25 and 64 points, 16 and 32 power steps: its
           four-lane form against its one-lane form (BM_SPECTRAL_LANES = 1), alternating in the same process; next to
           each the rounds it ran and the time per row-dot sweep, time / ((T + 2) rounds)
  rules    caf / dnc against Multi-Krum and the geometric median on the same stack, in the same process, alternating,
           device events

    python scripts/spectral_probe.py [weights] [rules]
"""

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


def report(name, ms, extra=""):
  q = statistics.quantiles(ms, n=10)
  print(f"  {name:<28} median {statistics.median(ms) * 1e3:9.1f} us   p10 {q[0] * 1e3:9.1f}   p90 {q[-1] * 1e3:9.1f}   "
        f"min {min(ms) * 1e3:9.1f}   ({len(ms)} runs){extra}")
  return statistics.median(ms)


def weights():
  lib = bm._lib.load()
  gen = torch.Generator(device=DEV).manual_seed(3)

  def with_lanes(lanes, fn):
    def call():
      lib.bm_tuning_set(b"BM_SPECTRAL_LANES", lanes)   # (0: the default, four lanes; read at the launch)
      try:
        return fn()
      finally:
        lib.bm_tuning_set(b"BM_SPECTRAL_LANES", 0)
    return call

  for N, f in ((25, 5), (64, 15)):
    pts = torch.randn(N, 4099, device=DEV, generator=gen)
    pts[-f:] = pts[-1] + 3.0
    sq = bm.gars.pairwise_sqdist(list(pts))
    print(f"weights kernel, N = {N} points, {f} of them copies of one far point")
    for mode, count in (("caf", f), ("dnc", f)):
      for T in (16, 32):
        fn = lambda: bm.gars.spectral_weights(sq, N, mode, count, T)  # noqa: E731
        rounds = int(fn()[1][0].item())
        calls = {f"{mode} T = {T} lanes = 4": with_lanes(0, fn), f"{mode} T = {T} lanes = 1": with_lanes(1, fn)}
        for name, ms in timed(calls, reps=30, warmup=5).items():
          sweeps = (T + 2) * max(rounds, 1)
          report(name, ms, f"   {rounds} rounds, {sweeps} sweeps: {statistics.median(ms) * 1e3 / sweeps:6.2f} us / sweep")


def rules():
  for n, f in ((25, 5), (51, 12)):
    rows = stack(n, f, D, seed=n)
    calls = {
      "krum": lambda: (bm.gars.invalidate_rank_cache(), bm.krum(rows, f))[1],
      "geomed (8 iterations)": lambda: bm.geomed(rows, f),
      "caf (16 power steps)": lambda: bm.caf(rows, f),
      "dnc (16 power steps)": lambda: bm.dnc(rows, f),
    }
    print(f"n = {n}, f = {f}, d = {D}: {n - f} honest rows + {f} references to one Byzantine vector")
    info = bm.caf(rows, f).spectral_info.tolist()
    print(f"  caf: {int(info[0])} rounds, the weights of round {int(info[3])} kept")
    times = timed(calls, reps=30, warmup=5)
    med = {name: report(name, ms) for name, ms in times.items()}
    for name in ("geomed (8 iterations)", "caf (16 power steps)", "dnc (16 power steps)"):
      print(f"  {name:<28} / krum = {med[name] / med['krum']:5.3f}")
    del rows
    torch.cuda.empty_cache()


if __name__ == "__main__":
  what = sys.argv[1:] or ["weights", "rules"]
  print(torch.cuda.get_device_name(0))
  if "weights" in what:
    weights()
  if "rules" in what:
    rules()
