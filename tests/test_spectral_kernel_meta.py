"""Code-object metadata of the kernel behind CAF and DnC (no GPU needed, see tests/test_kernel_meta.py): the spectral
weights kernel keeps the distances and its state in LDS — it may not touch scratch memory or spill a register, in its
four-lane form and in the one-lane form of the A/B knob alike."""

import importlib.util
import pathlib
import re

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent

KERNELS = [r"spectral_weights_kernel<4>", r"spectral_weights_kernel<1>"]


@pytest.fixture(scope="module")
def kernels():
  spec = importlib.util.spec_from_file_location("kernel_meta", ROOT / "scripts" / "kernel_meta.py")
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  if not mod.LIB.exists() or not (mod.LLVM / "llvm-objdump").exists():
    pytest.skip("libbm_gar.so or the LLVM tools are not here")
  return mod.kernels()


@pytest.mark.parametrize("pattern", KERNELS)
def test_spectral_kernel_has_no_scratch_and_no_spill(kernels, pattern):
  hits = [k for k in kernels if re.search(pattern, k["demangled"])]
  assert hits, f"no kernel matches {pattern}"
  for k in hits:
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (k["demangled"], k)
    assert k["vgpr"] <= 128, (k["demangled"], k["vgpr"])
    assert k["lds"] <= 64 * 1024, (k["demangled"], k["lds"])
