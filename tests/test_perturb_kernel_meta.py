"""Code-object metadata of the kernels behind the Min-Max / Min-Sum attacks (no GPU needed, see
tests/test_kernel_meta.py): every instance of the perturbation pass keeps its column and its h + 2 chains in registers
— no scratch memory, no spilled register, scalar ones included (the pointer table of the classes above 16 rows is read
from LDS for that) —, and the factor kernel keeps the distances in LDS."""

import importlib.util
import pathlib
import re

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent

# every (row-count class, vector width) dispatch_perturb can pick: 16 bytes up to 24 rows, 8 up to 40, 4 beyond
INSTANCES = [(k, v) for k in (8, 16, 24) for v in (4, 2, 1)] + [(k, v) for k in (32, 40) for v in (2, 1)] + \
            [(k, 1) for k in (48, 56, 64)]
KERNELS = [rf"perturb_stats_kernel<{k}, {v}>" for k, v in INSTANCES] + [r"perturb_finish_kernel", r"minmax_factor_kernel"]


@pytest.fixture(scope="module")
def kernels():
  spec = importlib.util.spec_from_file_location("kernel_meta", ROOT / "scripts" / "kernel_meta.py")
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  if not mod.LIB.exists() or not (mod.LLVM / "llvm-objdump").exists():
    pytest.skip("libbm_gar.so or the LLVM tools are not here")
  return mod.kernels()


@pytest.mark.parametrize("pattern", KERNELS)
def test_perturb_kernels_have_no_scratch_and_no_spill(kernels, pattern):
  hits = [k for k in kernels if re.search(pattern, k["demangled"])]
  assert hits, f"no kernel matches {pattern}"
  for k in hits:
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (k["demangled"], k)


def test_no_other_instance_of_the_perturbation_pass_exists(kernels):
  found = sorted(re.search(r"perturb_stats_kernel<(\d+), (\d+)>", k["demangled"]).groups()
                 for k in kernels if "perturb_stats_kernel<" in k["demangled"])
  assert found == sorted((str(k), str(v)) for k, v in INSTANCES)
