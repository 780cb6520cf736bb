"""Errors and timings of the Min-Max / Min-Sum attacks on one GPU:
  errors   the two figures the bars of tests/test_gpu_minmax.py are 4 x of (profiles/minmax_errors.txt), measured by
           that file's own functions on its own cases: the scalars of bm_perturb_stats against float64 sums of the
           device's fp32 vectors, and gamma end to end against the float64 reference on the vectors
  timings  (profiles/minmax_timings.txt) at h = 20 and 39, d = 11 173 962, alternating in one process, medians of 20:
           bm_perturb_stats against bm_stack_stats with a direction on the same rows (the same bytes), and the whole
           attack against the route through the entry points there were before: bm_stack_stats + bm_pairwise_sqdist on
           h + 2 rows (honests, avg, avg + p)

    python scripts/minmax_probe.py [errors] [timings]
"""

import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import byzantinemomentum_amd as bm  # noqa: E402

DEV = torch.device("cuda", 0)
D = 11173962


def errors():
  from tests import test_gpu_minmax as T
  worst = 0.0
  print("scalars of bm_perturb_stats: worst |error| / sum |terms| over d in", T.DS, "offsets", T.OFFSETS, "three perturbations")
  for h in T.HS:
    w = T.measure_scalars(bm, h)
    worst = max(worst, w)
    print(f"  h = {h:2d}                     {w:.3e}")
  for h in (3, 20, 39, 64):
    w = T.measure_scalars_capped(bm, h)
    worst = max(worst, w)
    print(f"  h = {h:2d}, d = 100003, 2 workgroups  {w:.3e}")
  print(f"  worst {worst:.3e}   x 4 = {4 * worst:.3e}")
  worst_gamma = worst_vector = 0.0
  print("end to end against the float64 reference on the vectors: |gamma - ref| / ref, three perturbations, both attacks")
  for h, d, structure in T.END_TO_END:
    g, v = T.measure_end_to_end(bm, h, d, structure)
    worst_gamma, worst_vector = max(worst_gamma, g), max(worst_vector, v)
    print(f"  h = {h:2d}, d = {d}, {structure:<7} gamma {g:.3e}   vector at {v:.3f} of its allowance")
  print(f"  worst gamma {worst_gamma:.3e}   x 4 = {4 * worst_gamma:.3e}   (2e-6: a distance pass good to 1e-6, sensitivity 2)")


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
  print(f"  {name:<44} median {statistics.median(ms) * 1e3:9.1f} us   p10 {q[0] * 1e3:9.1f}   p90 {q[-1] * 1e3:9.1f}   "
        f"min {min(ms) * 1e3:9.1f}   ({len(ms)} runs)")
  return statistics.median(ms)


def timings():
  for h in (20, 39):
    gen = torch.Generator(device=DEV).manual_seed(h)
    rows = [torch.randn(D, device=DEV, generator=gen) for _ in range(h)]

    def old_route():
      avg, _, direction = bm.stats.stack_stats_async(rows, scale=-1.0, attack="little", direction=True)
      moved = avg + direction
      return bm.gars.pairwise_sqdist(rows + [avg, moved])

    calls = {
      "bm_stack_stats, little direction": lambda: bm.stats.stack_stats_async(rows, scale=-1.0, attack="little", direction=True),
      "bm_perturb_stats, std": lambda: bm.stats.perturb_stats(rows, "std"),
      "bm_perturb_stats, unit": lambda: bm.stats.perturb_stats(rows, "unit"),
      "bm_pairwise_sqdist, h rows": lambda: bm.gars.pairwise_sqdist(rows),
      "minmax_attack (std), whole": lambda: bm.stats.minmax_attack(rows, 1, perturbation="std"),
      "old route: stack_stats + sqdist on h + 2 rows": old_route,
    }
    print(f"h = {h}, d = {D}")
    med = {name: report(name, ms) for name, ms in timed(calls, reps=20, warmup=3).items()}
    print(f"  bm_perturb_stats (std) / bm_stack_stats = {med['bm_perturb_stats, std'] / med['bm_stack_stats, little direction']:5.3f}")
    print(f"  whole attack / old route = "
          f"{med['minmax_attack (std), whole'] / med['old route: stack_stats + sqdist on h + 2 rows']:5.3f}"
          f"   (the old route stops at the distances: the search on them and the vector are not in it)")
    del rows
    torch.cuda.empty_cache()


if __name__ == "__main__":
  what = sys.argv[1:] or ["errors", "timings"]
  print(torch.cuda.get_device_name(0))
  if "errors" in what:
    errors()
  if "timings" in what:
    timings()
