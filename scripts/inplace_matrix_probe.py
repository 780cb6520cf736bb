"""The in-place matrix (tests/inplace_matrix.py) on one GPU, measured instead of asserted: every writer case compared
over its whole allocation, every reduction case against float64, and per (entry point, group, row count) the number of
cases, of mismatching cases, of coordinates the reference resolved exactly (fp32 midpoints of the float64 sum, results
below the smallest normal) and the worst reduction error in units of the bar tests/test_gpu_inplace_matrix.py holds it
to — written to profiles/inplace_matrix_errors.txt.  A reduction that exceeds its bar is listed with the derivation the
bar would have to come from: chain length x 2^-24 of the sum of |terms|.

    python scripts/inplace_matrix_probe.py [OUTPUT]
"""

import collections
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import inplace_matrix as X  # noqa: E402


def chain_bound(case):
  """The longest fp32 chain of a lane (fused multiply-adds before a fold or the end) x 2^-24, relative to the sum of
  |terms|: what the fp32 part of these sums can lose at worst."""
  longest = 1
  for l in X.reduction_launches(case):
    if case.entry == X.SQNORMS:
      per_lane = min(X.sqnorm_walk(l.count, l.grid).iterations + 1, X.K_FOLD_EVERY)
    else:
      per_lane = min(-(-l.count // (l.grid * 256)), X.K_FOLD_EVERY if case.entry == X.SQDIST2 else 1 << 30)
    longest = max(longest, per_lane * l.width)
  return longest * 2.0 ** -24


def main(path):
  started = time.time()
  writers = collections.OrderedDict()     # (entry, group, k) -> [cases, mismatches, midpoints, subnormal, coordinates]
  misses = []
  for case in X.all_writer_cases():
    got, pre = X.run_writer(case)
    slot = writers.setdefault((case.entry, case.group, case.k), [0, 0, 0, 0, 0])
    pre, m_dev, want64 = X.with_device_multiplier(case, got, pre)
    bad = X.check_writer(case, got, pre)
    if want64 is not None and (m_dev is None or abs(m_dev - want64) > 1e-6 * abs(want64)):
      bad = dict(case=case._asdict(), what="multiplier", got=m_dev, want=want64)
    slot[0] += 1
    slot[1] += bad is not None
    slot[2] += pre.counts.midpoints
    slot[3] += pre.counts.subnormal
    slot[4] += pre.counts.total
    if bad is not None:
      misses.append(f"# MISS {bad}")
  reductions = collections.OrderedDict()  # (entry, group, k) -> [cases, worst error / bar]
  for case in X.all_reduction_cases():
    v = X.reduction_input(case)
    res, bits, flat = X.run_reduction(case, v)
    err, bad = X.check_reduction(case, res, v)
    slot = reductions.setdefault((case.entry, case.group, case.k), [0, 0.0])
    slot[0] += 1
    slot[1] = max(slot[1], err)
    if bad or not np.array_equal(bits, flat.bits):
      misses.append(f"# MISS {case} {bad[:2]} chain bound {chain_bound(case):.3e} of the sum of |terms|")
  lines = [f"# {torch.cuda.get_device_name(0)}: tests/inplace_matrix.py, every case.",
           "# writers: the whole allocation of a case (outputs bit for bit, a NaN matching any NaN; inputs and guard gaps the",
           "# very bits) against the CPU reference; `midpoints` and `small`: coordinates the reference evaluated with fractions.Fraction",
           "# (fp32 midpoints of the float64 sum; results not above 2^-126), none left out of the comparison.",
           "# (bm_anticge_scale with a finite multiplier: fl32(v m) of the device's own multiplier, itself within 1e-6 of float64.)",
           "# entry group k cases mismatching midpoints small coordinates"]
  for (entry, group, k), (n, bad, mid, small, total) in writers.items():
    lines.append(f"{entry} {group} {k} {n} {bad} {mid} {small} {total}")
  lines += ["# reductions: worst |got - float64| in units of the bar (1e-6 of the sum of squares; 1e-6 |a| |b| for a dot)",
            "# entry group k cases worst_error_over_bar"]
  for (entry, group, k), (n, worst) in reductions.items():
    lines.append(f"{entry} {group} {k} {n} {worst:.4f}")
  lines.append(f"# misses: {len(misses)}")
  lines += misses
  lines.append(f"# {time.time() - started:.0f} s")
  os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
  with open(path, "w") as out:
    out.write("\n".join(lines) + "\n")
  print("\n".join(lines[-(len(misses) + 2):]))
  print(f"{len(lines)} lines -> {path}")


if __name__ == "__main__":
  main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "inplace_matrix_errors.txt"))
