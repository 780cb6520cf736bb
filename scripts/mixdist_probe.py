"""Timings of the distance-based rules on mixed rows, form="rows" against form="scalars" (profiles/mixdist_timings.txt):
at n = 25, f = 5 and n = 51, f = 12, d = 11 173 962, one tensor per row, all in one process on the same stack, the two
forms alternating, device events, medians of 20:
  nnm(krum) and nnm(geomed), whole calls    form="rows": distances + masks + bm_mix_rows + the rule on the mixed rows
                                            form="scalars": distances + masks + scalar kernels + one bm_weighted_sum
  the two new kernels alone                 bm_mixed_sqdist_device, bm_mix_weights_device (and bm_nnm_masks_device, the
                                            yardstick for a one-workgroup kernel on the same matrix)
  the stages both forms share or replace    pairwise_sqdist + masks, mix_rows, weighted_sum
then scalars / rows per rule: the scalars form must be the faster one at both shapes.

    python scripts/mixdist_probe.py [n ...]
"""

import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import byzantinemomentum_amd as bm  # noqa: E402

DEV = torch.device("cuda", 0)
D = 11173962
SHAPES = {25: 5, 51: 12, 11: 2}


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


def report(name, ms):
  q = statistics.quantiles(ms, n=10)
  med = statistics.median(ms)
  print(f"  {name:<40} median {med * 1e3:9.1f} us   p10 {q[0] * 1e3:9.1f}   p90 {q[-1] * 1e3:9.1f}")
  return med


def shape(n, f, d):
  g = bm.gars
  rows = stack(n, d, seed=n)
  sq = g.pairwise_sqdist(rows)
  masks = g.nnm_masks(sq, n, f)
  mixed = g.mixed_sqdist(sq, n, masks, n)
  m = n - f - 2
  order, _ = g.rank_from_sqdist(mixed, n, f, m, bm._lib.RANK_KRUM)
  cw, _ = g.center_weights(mixed, n, "geomed", 1e-6, 8)
  w = g.mix_weights(masks, n, n, selection=order, m=m)
  calls = {}
  for rule in ("krum", "geomed"):
    for form in ("rows", "scalars"):
      def whole(rule=rule, form=form):
        g.invalidate_rank_cache()
        return g.nnm(rows, f, rule=rule, form=form)
      calls[f"nnm({rule}, form={form!r}), whole call"] = whole
  calls["pairwise_sqdist + masks"] = lambda: g.nnm_masks(g.pairwise_sqdist(rows), n, f)
  calls["nnm_masks alone"] = lambda: g.nnm_masks(sq, n, f)
  calls["mixed_sqdist alone"] = lambda: g.mixed_sqdist(sq, n, masks, n)
  calls["mix_weights (selection) alone"] = lambda: g.mix_weights(masks, n, n, selection=order, m=m)
  calls["mix_weights (weights) alone"] = lambda: g.mix_weights(masks, n, n, weights=cw)
  calls["rank_from_sqdist alone"] = lambda: g.rank_from_sqdist(mixed, n, f, m, bm._lib.RANK_KRUM)
  calls["center_weights (geomed, 8) alone"] = lambda: g.center_weights(mixed, n, "geomed", 1e-6, 8)
  calls["mix_rows alone"] = lambda: g.mix_rows(rows, masks, n)
  calls["weighted_sum alone"] = lambda: g.weighted_sum(rows, w)
  print(f"n = {n}, f = {f}, d = {d}: one tensor per row")
  times = timed(calls, reps=20, warmup=3)
  med = {name: report(name, ms) for name, ms in times.items()}
  for rule in ("krum", "geomed"):
    r, s = med[f"nnm({rule}, form='rows'), whole call"], med[f"nnm({rule}, form='scalars'), whole call"]
    print(f"  {rule}: scalars / rows = {s / r:5.3f}")
    assert s < r, (rule, s, r)
  print(f"  scratch of form='rows': {4 * d * n / 1e9:.2f} GB of mixed rows; of form='scalars': {8 * n * n} bytes")
  del rows
  torch.cuda.empty_cache()


if __name__ == "__main__":
  counts = [int(a) for a in sys.argv[1:]] or [25, 51]
  print(torch.cuda.get_device_name(0))
  for n in counts:
    shape(n, SHAPES.get(n, (n - 1) // 4), D)
