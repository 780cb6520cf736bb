"""The instances of bm_colwise_bucketed without a GPU: a Python mirror of the dispatch rule — which (op, n, n_out) have an
instance, at which vector widths — held to the sources (colwise_bucketed_dispatch.h, colwise_bucketed.hip) and to the
library's own bm_colwise_bucketed_supported, then the code objects: every instance the mirror names is in the library,
no other, none touches scratch or spills a vector register, and 11 and 25 rows keep four waves per SIMD."""

import importlib.util
import pathlib
import re

import pytest

from tests.test_instance_matrix_cpu import c_eval

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "byzantinemomentum_amd" / "csrc"
OPS = {"median": 0, "trmean": 1}
BUCKET_SIZES = (2, 3)
MAX_ROWS = 64


# ---------------------------------------------------------------------------------------------------------------------
# The mirror

BUCKETED_MAX_ROWS = {2: 44, 3: 51}   # per bucket size: where the fused form was measured to win


def n_out_of(n, s):
  return -(-n // s)


def bucket_counts(n):
  """The n_out that have an instance at n rows."""
  return {n_out_of(n, s) for s in BUCKET_SIZES if 2 <= n <= BUCKETED_MAX_ROWS[s]}


def supported(op, n, n_out):
  return op in OPS.values() and n_out in bucket_counts(n)


def max_vec(n, n_out):
  return 4 if (n + n_out) * 4 <= 96 else 2


def instances():
  """{(n, n_out, op, vec)}: every kernel the dispatch can launch."""
  return {(n, n_out, op, vec) for op in OPS.values() for n in range(2, max(BUCKETED_MAX_ROWS.values()) + 1)
          for n_out in bucket_counts(n) for vec in (4, 2, 1) if vec <= max_vec(n, n_out)}


def test_mirror_spelled_out():
  assert (n_out_of(11, 2), n_out_of(25, 2), n_out_of(51, 2)) == (6, 13, 26)   # the reference's worker counts
  assert (n_out_of(11, 3), n_out_of(25, 3), n_out_of(51, 3)) == (4, 9, 17)
  assert supported(0, 2, 1) and supported(1, 3, 2) and supported(0, 5, 2) and supported(0, 5, 3)
  assert not supported(0, 1, 1) and not supported(0, 5, 4) and not supported(2, 11, 6) and not supported(3, 11, 6)
  assert supported(0, 44, 22) and not supported(0, 45, 23) and supported(0, 45, 15)
  assert supported(1, 51, 17) and not supported(1, 51, 26) and not supported(1, 52, 18) and not supported(1, 52, 26)
  assert max_vec(11, 6) == 4 and max_vec(25, 13) == 2 and max_vec(25, 9) == 2 and max_vec(16, 8) == 4 and max_vec(17, 9) == 2
  assert len({(n, o) for n, o, _, _ in instances()}) == (44 - 1) + (51 - 1) - 2    # (n = 2, 4: one bucket count)


# ---------------------------------------------------------------------------------------------------------------------
# ... against the sources

@pytest.fixture(scope="module")
def dispatch():
  return (CSRC / "colwise_bucketed_dispatch.h").read_text()


def test_mirror_matches_the_dispatch_header(dispatch):
  limit_expr = re.search(r"constexpr int bucketed_max_rows\(int s\) \{ return ([^;]+); \}", dispatch).group(1)
  consts = {name: int(value) for name, value in re.findall(r"constexpr int (kBucketedMaxRows\w*)\s*=\s*(\d+);", dispatch)}
  for s in BUCKET_SIZES:
    assert c_eval(limit_expr, dict(consts, s=s)) == BUCKETED_MAX_ROWS[s]
  n_out_expr = re.search(r"constexpr int bucketed_n_out\(int n, int s\) \{ return ([^;]+); \}", dispatch).group(1)
  vec_expr = re.search(r"constexpr int bucketed_max_vec\(\) \{\s*return ([^;]+);", dispatch).group(1)
  for n in range(1, MAX_ROWS + 1):
    for s in (1, 2, 3, 5):
      assert c_eval(n_out_expr, {"n": n, "s": s}) == n_out_of(n, s)
    for s in BUCKET_SIZES:
      assert c_eval(vec_expr, {"N": n, "NOUT": n_out_of(n, s)}) == max_vec(n, n_out_of(n, s)), (n, s)
  # the width the launch site hands to the cutter is that function, and the instances are those of the two bucket sizes
  assert "for_body_and_tail<bucketed_max_vec<N, NOUT>()>(Tail::kRides" in dispatch
  assert "constexpr int NOUT = bucketed_n_out(N, S);" in dispatch


def test_translation_units_cover_the_rules_and_bucket_sizes():
  units = sorted(p.name for p in CSRC.glob("colwise_bucketed_*.hip"))
  assert units == [f"colwise_bucketed_{rule}_s{s}.hip" for rule in sorted(OPS) for s in BUCKET_SIZES]
  for rule in OPS:
    for s in BUCKET_SIZES:
      text = (CSRC / f"colwise_bucketed_{rule}_s{s}.hip").read_text()
      assert f"colwise_bucketed_dispatch<BM_OP_{rule.upper()}, {s}, 2, bucketed_max_rows({s})>" in text
  entry = (CSRC / "colwise_bucketed.hip").read_text()
  assert "for (int s = 2; s <= 3; ++s)" in entry
  assert "if (n <= bucketed_max_rows(s) && n_out == bucketed_n_out(n, s)) return 1;" in entry


def test_mirror_matches_the_library():
  from byzantinemomentum_amd import _lib
  lib = _lib.load()
  assert (_lib.OP_MEDIAN, _lib.OP_TRMEAN) == (OPS["median"], OPS["trmean"])
  for op in range(-1, 5):
    for n in range(0, MAX_ROWS + 2):
      for n_out in range(0, n + 2):
        assert bool(lib.bm_colwise_bucketed_supported(op, n, n_out)) == supported(op, n, n_out), (op, n, n_out)


# ---------------------------------------------------------------------------------------------------------------------
# ... and the code objects (in the manner of tests/test_nnm_kernel_meta.py)

@pytest.fixture(scope="module")
def all_kernels():
  spec = importlib.util.spec_from_file_location("kernel_meta", ROOT / "scripts" / "kernel_meta.py")
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  if not mod.LIB.exists() or not (mod.LLVM / "llvm-objdump").exists():
    pytest.skip("libbm_gar.so or the LLVM tools are not here")
  return mod.kernels()


@pytest.fixture(scope="module")
def kernels(all_kernels):
  found = {}
  for k in all_kernels:
    m = re.search(r"colwise_bucketed_kernel<(\d+), (\d+), (\d+), (\d+)>", k["demangled"])
    if m:
      key = tuple(int(x) for x in m.groups())
      assert key not in found, f"{key} is in two code objects"
      found[key] = k
  return found


def test_the_library_holds_exactly_the_mirrors_instances(kernels):
  assert set(kernels) == instances()


def test_every_instance_stays_in_registers(kernels):
  for key, k in kernels.items():
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (key, k)


@pytest.mark.parametrize("n", [11, 25])
def test_flagship_row_counts_keep_four_waves(kernels, n):
  hits = {key: k for key, k in kernels.items() if key[0] == n}
  assert len(hits) == 2 * 2 * len([v for v in (4, 2, 1) if v <= max_vec(n, n_out_of(n, 2))])
  for key, k in hits.items():
    assert k["sgpr_spill"] == 0, (key, k)                # the N * NOUT pair weights stay out of the scalar file
    assert k["vgpr"] <= 128, (key, k["vgpr"])


def test_the_mask_kernel(all_kernels):
  hits = [k for k in all_kernels if "bucket_masks_kernel" in k["demangled"]]
  assert len(hits) == 1
  for k in hits:
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
