"""The step matrix (tests/step_matrix.py) on one GPU, measured instead of asserted: every case of the product, the plan
cases and the long first-pass cases through AggregationStep on the HIP backend against the float64 loop, and the worst
error of every compared quantity per (rule, attack) written to profiles/step_matrix_errors.txt — each next to the bar
tests/test_gpu_step_matrix.py holds it to.  A combination that exceeds a bar while every decision of the device agrees
with the loop's gets 4 x its worst as its bar (step_matrix.MEASURED_BARS); the file lists every miss.

    python scripts/step_matrix_probe.py [OUTPUT]
"""

import collections
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import step_matrix as SM  # noqa: E402

DEV = "cuda:0"


def groups(errs):
  """{quantity: (error, bar)}: the keys of the study row that involve the defense or the attack apart, the others —
  the sampled and honest statistics, the same whatever the rule — as one quantity, `floats.first_pass`."""
  out = {}
  for key, (err, bar) in errs.items():
    name = key
    if key.startswith("floats.") and not any(word in key for word in ("def", "att", "accept", "curv", "cosin_sampled")):
      name = "floats.first_pass"
    if name not in out or err > out[name][0]:
      out[name] = (err, bar)
  return out


def main(path):
  from byzantinemomentum_amd.sharded import ShardedAggregator
  worst = collections.defaultdict(dict)   # (rule, attack) -> {quantity: (error, bar)}
  misses, started = [], time.time()

  for case in SM.cases() + SM.long_cases():
    forms = [None] + ([ShardedAggregator(local_only=True)] if case.rule in SM.CENTER + SM.SPECTRAL else [])
    singles = (True, False) if SM.can_take_the_single_call(case) else (case.single_call,)
    for aggregator in forms:
      for single in singles:
        seen = {}
        try:
          bad = SM.run_case(case._replace(single_call=single), aggregator, DEV, worst=seen)
        except AssertionError as failure:  # a probe reports what the test asserts; a device error ends the run
          bad = {"assertion": str(failure)[:400]}
        if bad:
          misses.append((case.name, "local_only" if aggregator is not None else "plain", single, bad))
        slot = worst[(case.rule, case.attack)]
        for name, pair in groups(seen).items():
          if name not in slot or pair[0] > slot[name][0]:
            slot[name] = pair
  lines = [f"# {torch.cuda.get_device_name(0)}: worst error of every compared quantity per (rule, attack) against the float64",
           "# loop of tests/step_matrix.py, over every case, step and form; `bar`: what tests/test_gpu_step_matrix.py holds it to.",
           "# defense / update / server_momentum / cclip_start in the rule's measure (abs: over max|sampled|; norm: relative",
           "# in norm), byzantine over max|sampled| (minmax / minsum: in units of its allowance), floats: the study row's",
           "# largest error as center_cases.float_errors normalises it.",
           "# rule attack quantity worst bar"]
  for (rule, attack), slot in sorted(worst.items()):
    for name, (err, bar) in sorted(slot.items()):
      lines.append(f"{rule} {attack} {name} {err:.3e} {bar:.3e}")
  lines.append(f"# misses: {len(misses)}")
  for name, form, single, bad in misses:
    lines.append(f"# MISS {name} {form} single_call={single} {bad}")
  lines.append(f"# {time.time() - started:.0f} s")
  os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
  with open(path, "w") as out:
    out.write("\n".join(lines) + "\n")
  print("\n".join(lines[-(len(misses) + 2):]))
  print(f"{len(lines)} lines -> {path}")


if __name__ == "__main__":
  main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "step_matrix_errors.txt"))
