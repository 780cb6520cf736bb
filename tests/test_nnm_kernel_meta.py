"""Code-object metadata of the mixing kernels (no GPU needed, see tests/test_kernel_meta.py): a lane keeps the N values of
its columns — and, fused, the N mixed values as well — in registers with static indices.  None may touch scratch memory
or spill a vector register at any row count; at n = 11 and 25 no scalar register spills either (the N * n_out pair
weights stay out of the scalar file: mix_kernels.h)."""

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


@pytest.fixture(scope="module")
def limit():
  from byzantinemomentum_amd import _lib
  return _lib.load().bm_colwise_mixed_max_rows()


def _hits(kernels, pattern):
  hits = [k for k in kernels if re.search(pattern, k["demangled"])]
  assert hits, f"no kernel matches {pattern}"
  return hits


@pytest.mark.parametrize("n", [11, 25])
def test_flagship_row_counts_spill_nothing(kernels, n):
  # every vector width of the materialising kernel, both rules and both widths of the fused one
  hits = _hits(kernels, rf"mix_rows_kernel<{n}, \d>") + _hits(kernels, rf"colwise_mixed_kernel<{n}, [01], \d>")
  assert len(hits) == 3 + 2 * 2
  for k in hits:
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (k["demangled"], k)
    assert k["vgpr"] <= 128, (k["demangled"], k["vgpr"])      # four waves per SIMD


def test_every_fused_instance_stays_in_registers(kernels, limit):
  assert limit >= 25
  for n in range(1, limit + 1):
    hits = _hits(kernels, rf"colwise_mixed_kernel<{n}, [01], \d>")
    assert len(hits) == 4, (n, len(hits))
    for k in hits:
      assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (k["demangled"], k)
  assert not [k for k in kernels if re.search(rf"colwise_mixed_kernel<{limit + 1}, ", k["demangled"])]


@pytest.mark.parametrize("n", [51, 64])
def test_wide_materialising_instances_stay_in_registers(kernels, n):
  for k in _hits(kernels, rf"mix_rows_kernel<{n}, \d>"):
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (k["demangled"], k)


def test_masks_kernel(kernels):
  for k in _hits(kernels, r"nnm_masks_kernel"):
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (k["demangled"], k)
