"""Generate tests/golden/anticge/*.npz by running the REAL reference attack (the unmodified
`attacks.attacks["anticge"]`, attacks/anticge.py:49-78) on seeded honest stacks.  Needs a reference checkout:

    BM_REFERENCE_DIR=/root/reference python scripts/make_golden_anticge.py

Every fixture stores the honest rows themselves, (f_decl, f_real), the vector the reference returned and the order its
`_compute_normed` put the rows in.  The cases are listed in tests/anticge_reference.py (STACKS: f_decl = f_real = f on
`hetero` and `momentum` stacks, seed 3; EXTRAS: f_decl = h, and f_real > f_decl).  Every stored case must keep a
relative gap of 1e-4 between consecutive sorted norms, so that an fp64 ordering and the reference's fp32 one agree.
"""

import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import gar_oracle as O  # noqa: E402
from tests import anticge_reference as A  # noqa: E402

SEED = 3


def main():
  attack = A.reference_attack()
  out_dir = pathlib.Path(A.GOLDEN_DIR)
  out_dir.mkdir(parents=True, exist_ok=True)
  cases = {name: (kind, n, f, d, f, f) for name, (kind, n, f, d) in A.STACKS.items()}
  cases.update(A.EXTRAS)
  for name, (kind, n, f, d, f_decl, f_real) in sorted(cases.items()):
    rows, h = O.make_stack(kind, n, f, d, SEED)
    honests = rows[:h]
    gap = A.norm_gap(honests)
    assert gap >= A.MIN_NORM_GAP, (name, gap)
    kept = [g.clone() for g in honests]
    res = attack(grad_honests=honests, f_decl=f_decl, f_real=f_real)
    assert len(res) == f_real and all(r is res[0] for r in res) and all(res[0] is not g for g in honests)
    assert all(torch.equal(a, b) for a, b in zip(kept, honests))  # the attack leaves its inputs alone
    data = {"in_honest": torch.stack(honests).numpy(), "meta": np.array([f_decl, f_real], dtype=np.int64),
            "vector": res[0].numpy()}
    if f_real <= f_decl:
      data["order"] = np.array(A.reference_order(honests), dtype=np.int32)
    np.savez_compressed(out_dir / f"{name}.npz", **data)
    print(f"{name}: h={h} d={d} f_decl={f_decl} f_real={f_real} gap={gap:.2e} max|v|={float(res[0].abs().max()):.6g}")


if __name__ == "__main__":
  main()
