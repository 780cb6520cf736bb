"""Generate tests/golden/attacks/*.npz by running the REAL reference attacks (the unmodified
`attacks.attacks["nan" | "bulyan" | "empire-strict"].unchecked`, attacks/nan.py, attacks/identical.py, attacks/empire.py)
on CPU, with the reference's own aggregation rules as `defense`.  Needs a reference checkout:

    BM_REFERENCE_DIR=/path/to/reference python scripts/make_golden_attacks.py

The cases are listed in tests/attack_vectors_reference.py (CASES): `hetero` stacks O.make_stack("hetero", n, f, d = 203,
seed), f_decl = f_real = f.  Every fixture stores the honest rows themselves, the case (as JSON), the seed, the vector
the reference returned and, for a searched case, the factor it applied (read off the f32 restatement once its vector
is the reference's bit for bit).  A searched case is kept only if the reference's fp32 search and the restatement whose
objective is float64 settle on the SAME factor; where they do not, the next seed is taken — no tolerance is widened.
"""

import json
import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import gar_oracle as O  # noqa: E402
from tests import attack_vectors_reference as R  # noqa: E402
from tests.golden_io import same_bits  # noqa: E402

MAX_SEEDS = 12


def make(name, case, seed):
  """-> the fixture's arrays, or None when the condition on a searched case fails at this seed."""
  n, f = case["n"], case["f"]
  rows, h = O.make_stack("hetero", n, f, R.D, seed)
  honests = rows[:h]
  kept = [g.clone() for g in honests]
  searched = case["arg"] is not None and case["arg"] < 0
  defense = R.reference_rule(case["gar"]) if case["gar"] else None
  res = R.reference_attack(case["attack"])(grad_honests=honests, f_real=f, f_decl=f, defense=defense, model=None,
                                           **R.reference_kwargs(case))
  assert len(res) == f and all(r is res[0] for r in res) and all(res[0] is not g for g in honests)
  assert all(torch.equal(a, b) for a, b in zip(kept, honests))  # the attack leaves its inputs alone
  rule = R.oracle_rule(case["gar"]) if case["gar"] else None
  args = dict(defense=rule, arg=case["arg"], negative=case["negative"], target_idx=case["target_idx"])
  f32 = R.restate(case["attack"], honests, f, f, precision="f32", **args)
  assert same_bits(f32.vector, res[0]), name  # the restatement IS the reference, search included
  data = {"in_honest": torch.stack(honests).numpy(), "case": np.array(json.dumps(case)), "seed": np.int64(seed),
          "vector": res[0].numpy()}
  if searched:
    f64 = R.restate(case["attack"], honests, f, f, precision="f64", **args)
    if f64.factor != f32.factor:
      print(f"  {name}: seed {seed} dropped, the fp32 search found {f32.factor!r}, the float64 objective {f64.factor!r}")
      return None
    data["factor"] = np.float64(f32.factor)
  return data


def main():
  out_dir = pathlib.Path(R.GOLDEN_DIR)
  out_dir.mkdir(parents=True, exist_ok=True)
  for name, case in sorted(R.CASES.items()):
    for seed in range(R.FIRST_SEED, R.FIRST_SEED + MAX_SEEDS):
      data = make(name, case, seed)
      if data is not None:
        break
    else:
      raise AssertionError(f"{name}: no seed within {MAX_SEEDS} meets the condition")
    np.savez_compressed(out_dir / f"{name}.npz", **data)
    print(f"{name}: seed={seed} factor={data.get('factor')} max|v|={float(np.nanmax(np.abs(data['vector']))) if case['attack'] != 'nan' else 'nan'}")


if __name__ == "__main__":
  main()
