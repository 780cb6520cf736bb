"""Code-object metadata of the kernels behind the geometric median and centered clipping (no GPU needed, see
tests/test_kernel_meta.py): the weighted sum streams the rows and the weights kernel keeps its state in LDS — neither
may touch scratch memory or spill a vector register."""

import importlib.util
import pathlib
import re

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent

KERNELS = [r"weighted_sum_kernel<4>", r"weighted_sum_kernel<2>", r"weighted_sum_kernel<1>", r"center_weights_kernel"]


@pytest.fixture(scope="module")
def kernels():
  spec = importlib.util.spec_from_file_location("kernel_meta", ROOT / "scripts" / "kernel_meta.py")
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  if not mod.LIB.exists() or not (mod.LLVM / "llvm-objdump").exists():
    pytest.skip("libbm_gar.so or the LLVM tools are not here")
  return mod.kernels()


@pytest.mark.parametrize("pattern", KERNELS)
def test_new_kernels_have_no_scratch_and_no_spill(kernels, pattern):
  hits = [k for k in kernels if re.search(pattern, k["demangled"])]
  assert hits, f"no kernel matches {pattern}"
  for k in hits:
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (k["demangled"], k)
    assert k["vgpr"] <= 128, (k["demangled"], k["vgpr"])
