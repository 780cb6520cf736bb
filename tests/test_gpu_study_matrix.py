"""Every compiled instance of the study block (csrc/study.hip: 48 plain and 24 burst instances) and of the plain stack
statistics (csrc/reduce.hip: 12, tests/study_matrix.py) against expected values computed from the inputs alone: bit for
bit where the arithmetic is determined (the attack average, C, M, the stack average, the `empire` vector, every
maximum, every zero slot, the guard gaps and the inputs), in float64 at the suite's own bars elsewhere (Gram, dots and
l2 1e-6 of |a||b|, the deviation sums 1e-5, `little` 4e-6 of the largest).  The long cases carry power-of-two spikes at
their edge coordinates, so a coordinate or a column group that is dropped or counted twice moves a sum by ten bars or
more (tests/test_study_matrix_cpu.py holds that).

BM_STUDY_BURST is read once per process, so the burst form runs in a child process, one attempt, that holds its
outputs to the same bars and prints a SHA-256 per output; this process runs the same cases at the default knob, so no
assertion rests on a knob's output alone.  Needs an MI355X: `pytest -m gpu`.

With BM_STUDY_ERRORS=FILE in the environment the run also writes the worst error it saw per (kernel, instance, VEC,
quantity) next to its bar — how profiles/study_errors.txt is made.
"""

import json
import os
import subprocess
import sys

import pytest
import torch

from tests import study_matrix as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300


@pytest.fixture(scope="module")
def cus():
  for knob, value in S.DEFAULT_KNOBS.items():  # this process is the one at the defaults
    assert int(os.environ.get(knob, value)) == value, f"{knob} is set: the mirror of this process assumes the defaults"
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module", autouse=True)
def error_table():
  yield
  path = os.environ.get("BM_STUDY_ERRORS")
  if path:
    with open(path, "w") as out:
      out.write("\n".join(S.ERRORS.lines()) + "\n")


_FAULTED = []  # a GPU fault, a crash or a hang in this file: nothing more is started on the GPU


@pytest.fixture(autouse=True)
def _not_after_a_fault():
  if _FAULTED:
    pytest.fail(f"not started: {_FAULTED[0]}")


def _sweep(todo, cus, digests=None, knobs=None):
  try:
    return S.sweep(todo, cus, digests=digests, knobs=knobs)
  except RuntimeError as err:  # a HIP error surfaces here; whatever it was, the device is not to be used again
    _FAULTED.append(f"an earlier sweep raised {str(err)[:200]!r}")
    raise


def _child(group, part, knobs):
  """The report of `group` (its `part`) from a fresh process with `knobs` set: one attempt; a crash or a timeout fails
  the test."""
  env = dict(os.environ, PYTHONPATH=ROOT, **{k: str(v) for k, v in knobs})
  env.pop("BM_STUDY_ERRORS", None)
  cmd = [sys.executable, os.path.join(ROOT, "tests", "study_matrix.py"), group] + ([str(part)] if part is not None else [])
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
  S.ERRORS.merge(res["worst"])
  return res


def _none(fails):
  assert not fails, (len(fails), fails[:6])


# ---------------------------------------------------------------------------------------------------------------------
# 1. The plain form

@pytest.mark.parametrize("part", S.PARTS["plain"], ids=("vec4", "vec2", "vec1", "edges"))
def test_plain_form(cus, part):
  """study_stats_kernel<ATT, CM, L2, VEC>: every instance with the momentum stream on and off and, with an attack, the
  attack average on and off, at d = 1175 (two workgroups, the second ragged, a 3-coordinate tail), f_real rotating over
  1, 2, 3, 5, 64 | every pointer live at d = 0, 1, 3, 4, 5, 1023, 1024, 1027 at each width, all vectors at byte offset
  12, each of the eleven pointers alone moved on by 4 and by 8 bytes, f_real = 1, 2, 3, 5, 64."""
  todo = S.cases("plain", cus, part)
  assert all(i[0] == "study" for c in todo for i in S.instances(c, cus)[0])
  if part < 3:
    assert all(l.vec in ((4, 2, 1)[part], 1) for c in todo for l in S.instances(c, cus)[1])
  _none(_sweep(todo, cus))


@pytest.mark.parametrize("part", S.PARTS["plain_long"], ids=("fold", "grid-cap", "nparts"))
def test_plain_form_long(cus, part):
  """The smallest d at which a lane has 17 iterations (4-byte columns: the fp32 chains are folded into fp64 once and
  one iteration follows) | the grid cap and one workgroup of work more with a 3-coordinate tail: 2049 partial sets |
  2048, 64 and 65 partial sets.  Power-of-two spikes at the edge coordinates."""
  todo = S.cases("plain_long", cus, part)
  assert all(l.form == "plain" for c in todo for l in S.instances(c, cus)[1])
  _none(_sweep(todo, cus))


# ---------------------------------------------------------------------------------------------------------------------
# 2. The burst form

@pytest.mark.parametrize("part", S.PARTS["knob_burst"],
                         ids=("instances-no-attack", "instances-attack", "one-and-three-iterations", "past-a-burst-2x8",
                              "past-a-burst-1x8", "past-a-burst-1x4", "output-and-non-finite"))
def test_burst_form(cus, part):
  """study_stats_burst_kernel<ATT, CM, L2, MOM> (BM_STUDY_BURST=1, a child process): all 24 instances at two iterations,
  the second partly live, and a 3-coordinate tail launch behind the compute units' partial sets | per (U, staged
  iterations) class one iteration and three (with U = 2 the second group of the last step is not live) | one iteration
  past a burst (9, 9, 5), partly live | an attack-average output (stays plain), NaN / inf / the maximum in lane 1023 and
  in the last live group.  The bars hold in the child; C, M and the maxima have the digests of this process, which
  runs the same cases at the default knob and holds them to the expected values as well."""
  todo = S.cases("knob_burst", cus, part)
  assert todo and all(c.knobs == S.BURST_ONLY for c in todo)
  mine = {}
  _none(_sweep(todo, cus, digests=mine, knobs=()))  # (the same inputs, spikes at the burst form's edge coordinates)
  res = _child("knob_burst", part, S.BURST_ONLY)
  _none(res["failures"])
  assert set(res["digests"]) == set(mine)
  differ = S.differing(todo, mine, res["digests"])
  assert not differ, (len(differ), differ[:8])


# ---------------------------------------------------------------------------------------------------------------------
# 3. Arguments and non-finite values

def test_argument_behaviours(cus):
  """An attack-average output or a Byzantine vector with f_real = 0, C with curv_mode = 0 (none of them read or
  written: slots 18-20, 16-17 zero), a NaN-filled C in mode 1 (C = s, no NaN in a slot), past_newest is past_oldest,
  s is h, the spare slots zeroed over a NaN-filled `out`, d = 0."""
  todo = S.cases("args", cus)
  assert [c.arg for c in todo] == list(S.ARGS)
  _none(_sweep(todo, cus))


def test_non_finite_values_and_maxima(cus):
  """One NaN, +inf, -inf or the maximum in the defense vector or the Byzantine vector: at coordinate 0, in lane 63 and
  lane 255 of the last live iteration, in the last vector of the body and in the tail, at each width.  A maximum is NaN
  where torch's abs().max() is NaN."""
  _none(_sweep(S.cases("bad", cus), cus))


# ---------------------------------------------------------------------------------------------------------------------
# 4. The stack statistics

@pytest.mark.parametrize("part", S.PARTS["stack"], ids=("k1-8", "k9-16", "k17-24", "k25-32", "k33-64", "cap-and-non-finite"))
def test_stack_statistics(cus, part):
  """stack_stats_kernel<KMAX, VEC>: k at both edges of every tier x every combination of the two outputs x `empire`
  (1.1) and `little` (-1.5) with and without BM_ATTACK_DIRECTION at d = 1027; rows at byte offset 0 / 4 / 8 / mixed x
  d = 0, 3, 1027, 3074 (25..32 rows: 8-byte columns over twice the count; more: 4-byte columns over four times, each with
  a tail launch) | the 2047-workgroup cap, one vector more and a tail; one NaN, +inf, -inf."""
  _none(_sweep(S.cases("stack", cus, part), cus))


def test_attack_statistics_are_the_stack_statistics_of_aliased_rows(cus):
  """study.hip: "stack_stats_kernel on f aliased rows".  f_real = 1, 3, 5, 64: the attack average of the study block and
  bm_stack_stats' average of [byz] * f_real bit for bit, slot 20 and out3[2] bit for bit, slots 18 and 19 against
  out3[0:2] at the bars; both calls against the expected values."""
  _none(_sweep(S.cases("aliased", cus), cus))
