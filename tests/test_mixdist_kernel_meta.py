"""Code-object metadata of the two scalar kernels behind form="scalars" (no GPU needed, see tests/test_kernel_meta.py):
one workgroup each, D and Q in LDS, a few sums per lane — neither may touch scratch memory or spill a register, and the
distance kernel has to fit 1 024 lanes (at most 128 VGPRs)."""

import importlib.util
import pathlib
import re

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def kernels():
  spec = importlib.util.spec_from_file_location("kernel_meta", ROOT / "scripts" / "kernel_meta.py")
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  if not mod.LIB.exists() or not (mod.LLVM / "llvm-objdump").exists():
    pytest.skip("libbm_gar.so or the LLVM tools are not here")
  return mod.kernels()


@pytest.mark.parametrize("name,vgprs", [("mixed_sqdist_kernel", 128), ("mix_weights_kernel", 128)])
def test_scalar_kernels_stay_in_registers(kernels, name, vgprs):
  hits = [k for k in kernels if re.search(rf"\b{name}\b", k["demangled"])]
  assert len(hits) == 1, (name, len(hits))
  k = hits[0]
  assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
  assert k["vgpr"] <= vgprs, k
  assert k["lds"] <= 2048, k          # static LDS: the masks, the diagonal, the weights; D and Q are dynamic
