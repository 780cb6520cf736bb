"""Every compiled instance of the step's first pass (csrc/step.hip: 144 of them, tests/first_pass_matrix.py) against
expected values computed from the inputs alone: bit for bit where the arithmetic is determined (buffers, both averages,
the `empire` vector, max|avg|), in float64 at the suite's own bars elsewhere (`little` 4e-6 of the largest, the four
sums 1e-5 on the forms test_momentum_stats_kernel_tiers compares, the rules at the bars of test_gpu_instance_matrix.py,
the distances at those of tests/pair_mode_check.py), plus rows at every byte offset, non-finite coordinates in every
lane position, NULL outputs, and nothing written outside the buffers.

The knobs the library reads once per process (BM_STEP_BURST, BM_STEP_STREAM) run in a child process, one at a time, one
attempt, that holds its outputs to the same bars and prints a SHA-256 per output; this process runs the same cases at
the defaults, so no assertion rests on a knob's output alone.  Needs an MI355X: `pytest -m gpu`.

With BM_FIRST_PASS_ERRORS=FILE in the environment the run also writes the worst error it saw per (kernel family, T, VEC,
quantity) next to its bar — how profiles/first_pass_errors.txt is made.
"""

import json
import os
import subprocess
import sys

import pytest
import torch

from tests import first_pass_matrix as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300


@pytest.fixture(scope="module")
def cus():
  for knob, value in F.DEFAULT_KNOBS.items():  # this process is the one at the defaults
    assert int(os.environ.get(knob, value)) == value, f"{knob} is set: the mirror of this process assumes the defaults"
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module", autouse=True)
def error_table():
  yield
  path = os.environ.get("BM_FIRST_PASS_ERRORS")
  if path:
    with open(path, "w") as out:
      out.write("\n".join(F.ERRORS.lines()) + "\n")


_FAULTED = []  # a GPU fault, a crash or a hang in this file: nothing more is started on the GPU


@pytest.fixture(autouse=True)
def _not_after_a_fault():
  if _FAULTED:
    pytest.fail(f"not started: {_FAULTED[0]}")


def _sweep(todo, cus, digests=None, check=True):
  try:
    return F.sweep(todo, cus, digests=digests, check=check)
  except RuntimeError as err:  # a HIP error surfaces here; whatever it was, the device is not to be used again
    _FAULTED.append(f"an earlier sweep raised {str(err)[:200]!r}")
    raise


def _child(group, part, knobs):
  """The report of `group` (its `part`) from a fresh process with `knobs` set: one attempt; a crash or a timeout fails
  the test."""
  env = dict(os.environ, PYTHONPATH=ROOT, **{k: str(v) for k, v in knobs})
  env.pop("BM_FIRST_PASS_ERRORS", None)
  cmd = [sys.executable, os.path.join(ROOT, "tests", "first_pass_matrix.py"), group] + ([str(part)] if part is not None else [])
  try:
    done = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
  except subprocess.TimeoutExpired as err:
    _FAULTED.append(f"the {group} child hung")
    pytest.fail(f"{group} child timed out after {CHILD_TIMEOUT} s: {(err.stderr or b'')[-2000:]!r}")
  if done.returncode != 0:
    _FAULTED.append(f"the {group} child ended with status {done.returncode}")
  assert done.returncode == 0, (group, done.returncode, done.stderr[-3000:])
  res = json.loads(done.stdout.strip().splitlines()[-1])
  assert all(res["knobs"][k] == str(v) for k, v in knobs), res["knobs"]
  F.ERRORS.merge(res["worst"])
  return res


def _none(fails):
  assert not fails, (len(fails), fails[:6])


def _against_the_defaults(group, part, knobs, cus, check=True):
  """The cases of a knob group in this process at the defaults (bars, digests), then under the knob in a child (the
  same bars there), and the bit-exact outputs of the two compared.  check=False: this process takes the digests only —
  for the groups whose default-knob form is the two-kernel path that other tests of this file hold to the bars."""
  todo = F.cases(group, cus, part)
  assert todo and all(c.knobs == knobs for c in todo)
  mine = {}
  _none(_sweep([c._replace(knobs=()) for c in todo], cus, digests=mine, check=check))
  res = _child(group, part, knobs)
  _none(res["failures"])
  assert set(res["digests"]) == set(mine)
  differ = F.differing(todo, mine, res["digests"])
  assert not differ, (len(differ), differ[:8])
  return todo


# ---------------------------------------------------------------------------------------------------------------------
# 1. Register tiers, plain form

@pytest.mark.parametrize("tier", F.PARTS["register"])
def test_register_tiers(cus, tier):
  """momentum_stats_kernel<T, VEC, EXACT, CLIP, false>: (ks, h) = (1, 1), (3, 3), (8, 8), (8, 5) | (9, 9), (12, 12),
  (12, 7), (11, 9) | (14, 14) | (20, 20); with and without clipping factors, `empire` and `little` (negative scale),
  BM_ATTACK_DIRECTION, rows at byte offset 0 / 4 / 8 / 12 / mixed, d = 0, 1, 3, 4, 5, 255, 1027, 3074; one NaN, +inf,
  -inf in turn in a sampled row and in a buffer, first and last lane of a vector and the scalar tail."""
  todo = F.cases("register", cus, tier)
  assert all(i[0] == "stats" and i[1] == tier and not i[5] for c in todo for i in F.instances(c, cus))
  _none(_sweep(todo, cus))


# ---------------------------------------------------------------------------------------------------------------------
# 2. Streaming tiers

@pytest.mark.parametrize("tier", F.PARTS["stream"])
def test_streaming_tiers(cus, tier):
  """momentum_stats_stream_kernel<T, VEC, CLIP>: batches of four rows that straddle h, straddle ks, or hold sampled rows
  only — (13, 13), (14, 13), (20, 19), (20, 17), (19, 1) | (21, 21), (22, 21), (40, 40), (40, 37), (39, 4) | (41, 41),
  (64, 64), (64, 50), (64, 1) — on the axes of the register tiers."""
  todo = F.cases("stream", cus, tier)
  assert all(i[0] == "stream" and i[1] == tier for c in todo for i in F.instances(c, cus))
  _none(_sweep(todo, cus))


@pytest.mark.parametrize("tier", F.PARTS["knob_stream"])
def test_register_shapes_in_the_streaming_form(cus, tier):
  """BM_STEP_STREAM=1 (a child process): the register shapes run momentum_stats_stream_kernel<20>; the float64 bars
  hold there, and buffers, both averages, the `empire` vector and the maxima have the digests of the register form."""
  todo = _against_the_defaults("knob_stream", tier, F.STREAM_ONLY, cus)
  assert all(i[0] == "stream" for c in todo for i in F.instances(c, cus))


# ---------------------------------------------------------------------------------------------------------------------
# 3. Burst forms

@pytest.mark.parametrize("shape", F.PARTS["knob_burst"], ids=lambda p: "ks%d-h%d" % F.BURST_SHAPES[p])
def test_burst_forms(cus, shape):
  """BM_STEP_BURST=1 (a child process): every register shape with h >= 3 at every width, at exactly one iteration of the
  burst form per CU and at one iteration and a ragged second with a scalar tail.  The float64 bars hold; every output
  but the four sums has the digest of the plain form at the same length (this process, which holds the plain form —
  more than one grid-stride trip of 2047 workgroups at 16 bytes — to the expected values as well)."""
  todo = _against_the_defaults("knob_burst", shape, F.BURST_ONLY, cus)
  for c in todo:
    body = max(F.instances(c, cus), key=lambda i: i[2])
    assert body[5] and not any(i[5] for i in F.instances(c._replace(knobs=()), cus)), c


# ---------------------------------------------------------------------------------------------------------------------
# 4. The rule riding along

def test_rule_riding_along(cus):
  """bm_momentum_stats_colwise and bm_stack_stats_colwise at (20, 20, 5) and (14, 14, 11) x median / trmean / phocas /
  meamed x every legal rule_f x {no clip, clip, no buffers}, d = 3072 and 3075: every output against the expected
  values, the aggregated vector against the float64 references of instance_matrix.py.  The neighbours (20, 20, 4),
  (20, 20, 6), (14, 14, 10), (21, 20, 5), 8-byte rows, and no buffers with d % 4 != 0 take the two kernels: same bars."""
  _none(_sweep(F.cases("rule", cus), cus))


@pytest.mark.parametrize("shape", F.PARTS["knob_burst_rule"], ids=lambda p: "h%d-nb%d" % F.RULE_SHAPES[p][1:])
def test_rule_riding_along_burst_form(cus, shape):
  """The same instances in their burst form (BM_STEP_BURST=1, a child process) at the two burst lengths: the bars, and
  the digests of the plain form, the aggregated vector included."""
  _against_the_defaults("knob_burst_rule", shape, F.BURST_ONLY, cus, check=False)


# ---------------------------------------------------------------------------------------------------------------------
# 5. The distances riding along

@pytest.mark.parametrize("part", F.PARTS["knob_burst_sqdist"], ids=lambda p: "h%d-nb%d" % F.SQDIST_CASES[p] if p < len(F.SQDIST_CASES) else "neighbours")
def test_distances_riding_along(cus, part):
  """momentum_gram_kernel<TT, CLIP, NOMOM> (BM_STEP_BURST=1, a child process: at the defaults it needs 4.2 M columns):
  h = 20 with 1, 5, 6 Byzantine copies and h = 14 with 11, `momentum` inputs, at one full iteration per CU, at a ragged
  second one, and with 1, 2, 3 trailing columns (tail_gram_kernel); d_total = 2^24; a NaN / +inf / -inf coordinate; the
  neighbours that take the two passes (7 copies, 8-byte rows, one vector short of an iteration).  Distances within 1e-5
  of the float64 direct differences of the EXPECTED rows, a bitwise symmetric matrix with a zero diagonal, exact zeros
  and equal rows for the copies, Krum and Bulyan rankings those of the float64 matrix; every other output against its
  expected value, with the digests of the two passes this process runs at the defaults."""
  _against_the_defaults("knob_burst_sqdist", part, F.BURST_ONLY, cus, check=False)


# ---------------------------------------------------------------------------------------------------------------------
# 6. NULL outputs

def test_null_outputs(cus):
  """bm_momentum_stats through the C ABI with sampled_avg, honest_avg, byz_out NULL in turn at (8, 8), (20, 20) and
  (21, 21): the remaining outputs keep their bits."""
  todo = F.cases("null", cus)
  digests = {}
  _none(_sweep(todo, cus, digests=digests))
  for c in todo:
    if c.null is not None:
      full = digests[F.case_key(c._replace(null=None))]
      mine = digests[F.case_key(c)]
      assert set(full) - set(mine) == {{"sampled_avg": "sampled_avg", "honest_avg": "honest_avg", "byz": "byz"}[c.null]}
      assert all(mine[name] == full[name] for name in mine), (F.case_key(c), mine, full)
