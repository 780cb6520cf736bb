"""Timings of nearest-neighbour mixing on one GPU (profiles/nnm_timings.txt): at n = 25, f = 5 and n = 51, f = 12,
d = 11 173 962, one tensor per row, all in one process on the same stack, alternating, device events, medians:
  (a) plain trmean / median                 the kernels of the plain rules: the yardstick
  (b) pairwise_sqdist + masks               what every form of NNM pays first
  (c) bm_mix_rows alone                     4 d (n + n) bytes
  (d) (c) + (a) on the mixed rows           the composition: 4 d (3 n + 1) bytes
  (e) bm_colwise_mixed                      the fused form: 4 d (n + 1) bytes
each as a time and as a fraction of 8 TB/s on its own algorithmic bytes, then (e) / (a) and (e) / (d): the fused form is
kept where (e) < (d).

    python scripts/nnm_probe.py [n ...]
"""

import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import byzantinemomentum_amd as bm  # noqa: E402

DEV = torch.device("cuda", 0)
D = 11173962
PEAK = 8e12  # bytes / s
SHAPES = {25: 5, 51: 12, 11: 2, 40: 9}


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


def report(name, ms, nbytes):
  q = statistics.quantiles(ms, n=10)
  med = statistics.median(ms)
  rate = f"{nbytes / (med * 1e-3) / PEAK:5.3f} of 8 TB/s on {nbytes / 1e6:8.1f} MB" if nbytes else ""
  print(f"  {name:<34} median {med * 1e3:9.1f} us   p10 {q[0] * 1e3:9.1f}   p90 {q[-1] * 1e3:9.1f}   {rate}")
  return med


def shape(n, f, d):
  rows = stack(n, d, seed=n)
  masks = bm.gars.nnm_masks(bm.gars.pairwise_sqdist(rows), n, f)
  mixed = bm.gars.mix_rows(rows, masks, n)
  fused_ok = n <= bm._lib.load().bm_colwise_mixed_max_rows()
  col, mix, comp = 4 * d * (n + 1), 4 * d * (2 * n), 4 * d * (3 * n + 1)
  calls = {
    "(a) trmean": (lambda: bm.gars.trmean(rows, f), col),
    "(a) median": (lambda: bm.gars.median(rows), col),
    "(b) pairwise_sqdist + masks": (lambda: bm.gars.nnm_masks(bm.gars.pairwise_sqdist(rows), n, f), 4 * d * n),
    "(c) mix_rows": (lambda: bm.gars.mix_rows(rows, masks, n), mix),
    "(a') trmean on the mixed rows": (lambda: bm.gars.trmean(mixed, f), col),
    "(d) mix_rows + trmean": (lambda: bm.gars.trmean(bm.gars.mix_rows(rows, masks, n), f), comp),
    "(d) mix_rows + median": (lambda: bm.gars.median(bm.gars.mix_rows(rows, masks, n)), comp),
  }
  if fused_ok:
    calls["(e) colwise_mixed trmean"] = (lambda: bm.gars.colwise_mixed("trmean", rows, masks, f), col)
    calls["(e) colwise_mixed median"] = (lambda: bm.gars.colwise_mixed("median", rows, masks, 0), col)
  calls["nnm(trmean), whole call"] = (lambda: bm.gars.nnm(rows, f, rule="trmean"), col + 4 * d * n)
  print(f"n = {n}, f = {f}, d = {d}: one tensor per row")
  times = timed({name: fn for name, (fn, _) in calls.items()}, reps=20, warmup=3)
  med = {name: report(name, ms, calls[name][1]) for name, ms in times.items()}
  if fused_ok:
    for rule in ("trmean", "median"):
      e, a, dd = med[f"(e) colwise_mixed {rule}"], med[f"(a) {rule}"], med[f"(d) mix_rows + {rule}"]
      print(f"  {rule}: (e) / (a) = {e / a:5.3f}   (e) / (d) = {e / dd:5.3f}")
      assert torch.equal(bm.gars.colwise_mixed(rule, rows, masks, f), getattr(bm.gars, rule)(mixed, f=f)), rule
  del rows, mixed
  torch.cuda.empty_cache()


if __name__ == "__main__":
  counts = [int(a) for a in sys.argv[1:]] or [25, 51]
  print(torch.cuda.get_device_name(0))
  for n in counts:
    shape(n, SHAPES.get(n, (n - 1) // 4), D)
