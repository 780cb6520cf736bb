"""The Min-Max / Min-Sum attacks on the GPU (bm_perturb_stats -> distance pass -> bm_minmax_factor_device ->
bm_multi_fma3_bdev).  Needs an MI355X: `pytest -m gpu`.  Rows are separately allocated tensors.
  (7)  avg_out has the bits of bm_stack_stats' average; dir_out the bits of its LITTLE | DIRECTION output at scale -1
       ("std"), -avg exactly ("unit"), -sign(avg) exactly ("sign") — at every row-count class (8 rows each) and at
       both ends of every class (CLASS_EDGES, which (8) and (9) run as well), every vector width (rows offset by 0, 1
       and 2 floats), lengths with and without a tail;
  (8)  the scalars against float64 sums of the device's OWN fp32 avg / dir and the rows — only the summation is
       measured —, as |error| / sum |terms|; one case with the grid capped (BM_PERTURB_GRID) at d = 100 003, where a lane
       runs 49-196 iterations (the fp32 -> fp64 fold is reached) and several workgroups contribute;
  (9)  two calls give the same bits; the device factor equals the host factor bit for bit on the device's own matrix
       and scalars;
  (10) gamma and the vector end to end against the float64 reference on the vectors, and tightness of gamma;
  (11) one step of AggregationStep(attack="minmax" | "minsum") against Krum, the median and DnC.
The bars of (8) and (10) are 4 x the worst value measured on an MI355X over these very cases
(profiles/minmax_errors.txt, written by scripts/minmax_probe.py from the functions below):
  (8)  worst 9.936e-08 -> BAR_SCALARS = 3.98e-07;
  (10) worst 3.010e-08 of gamma (next to the 2e-6 that a distance pass good to 1e-6 and a sensitivity of 2 allow)
       -> BAR_GAMMA = 1.21e-07; the vector is held to BAR_GAMMA * gamma |p| plus the fp32 roundings of the average, the
       direction and the sum (worst: 0.33 of that allowance)."""

import functools

import numpy as np
import pytest
import torch

from tests import minmax_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HS = (2, 3, 11, 20, 27, 39, 45, 50, 64)   # every row-count class of the dispatch: 8, 8, 16, 24, 32, 40, 48, 56, 64
# the last row count of a class and the first of the next (has(i) deciding the last 8 rows; from 25 rows on the pointer
# table travels in the kernel-argument segment): run through (7), (8) and (9); the bars were measured over HS
CLASS_EDGES = (8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 48, 49, 56, 57)
DS = (1, 3, 63, 1027, 4100)
OFFSETS = (0, 1, 2)                       # floats: vector widths 4, 1, 2
BAR_SCALARS = 3.98e-07
BAR_GAMMA = 1.21e-07


@pytest.fixture(scope="module")
def bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


@functools.lru_cache(maxsize=None)
def host_rows(h, d, structure="common", seed=2):
  return R.stack(h, d, structure, seed).astype(np.float32)


def device_rows(rows32, offset=0):
  """One allocation per row, the row `offset` floats into it."""
  out = []
  for r in rows32:
    buf = torch.empty(len(r) + offset + 4, dtype=torch.float32, device=DEV)
    view = buf[offset:offset + len(r)]
    view.copy_(torch.from_numpy(np.ascontiguousarray(r)))
    assert view.data_ptr() % 16 == (4 * offset) % 16
    out.append(view)
  return out


def bits(t):
  return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def scalar_errors(rows, avg, direction, scal):
  """max over the h + 2 scalars of |scal - float64 sum| / sum |terms|, the sums over the device's own fp32 vectors."""
  h = len(rows)
  a64, p64 = avg.double(), direction.double()
  worst = 0.0
  terms = [p64 * (a64 - r.double()) for r in rows] + [p64 * p64, a64 * a64]
  for slot, t in zip(list(range(h)) + [64, 65], terms):
    scale = t.abs().sum().item()
    err = abs(scal[slot].item() - t.sum().item())
    if scale > 0.0:
      worst = max(worst, err / scale)
    else:
      assert err == 0.0
  assert bool((scal[h:64] == 0).all())
  return worst


# ---------------------------------------------------------------------------- #
# (7)

@pytest.mark.parametrize("h", HS + CLASS_EDGES)
def test_average_and_direction_bits(bm, h):
  for d in DS:
    for offset in OFFSETS:
      rows = device_rows(host_rows(h, d), offset)
      want_avg, _, want_std = bm.stats.stack_stats_async(rows, scale=-1.0, attack="little", direction=True)
      for perturbation in R.PERTURBATIONS:
        avg, direction, scal = bm.stats.perturb_stats(rows, perturbation)
        tag = (h, d, offset, perturbation)
        assert torch.equal(bits(avg), bits(want_avg)), tag
        if perturbation == "std":
          assert torch.equal(bits(direction), bits(want_std)), tag
        elif perturbation == "unit":
          assert torch.equal(bits(direction), bits(-avg)), tag
        else:
          assert torch.equal(direction, -torch.sign(avg)), tag
        assert scal.shape == (66,) and bool(torch.isfinite(scal).all()), tag


# ---------------------------------------------------------------------------- #
# (8)

def measure_scalars(bm, h):
  worst = 0.0
  for d in DS:
    for offset in OFFSETS:
      rows = device_rows(host_rows(h, d), offset)
      for perturbation in R.PERTURBATIONS:
        avg, direction, scal = bm.stats.perturb_stats(rows, perturbation)
        worst = max(worst, scalar_errors(rows, avg, direction, scal))
  return worst


def measure_scalars_capped(bm, h, grid=2, d=100003):
  lib = bm._lib.load()
  rows = device_rows(host_rows(h, d), 0)
  worst = 0.0
  assert lib.bm_tuning_set(b"BM_PERTURB_GRID", grid) == 0
  try:
    for perturbation in R.PERTURBATIONS:
      avg, direction, scal = bm.stats.perturb_stats(rows, perturbation)
      worst = max(worst, scalar_errors(rows, avg, direction, scal))
      want_avg, _, want_std = bm.stats.stack_stats_async(rows, scale=-1.0, attack="little", direction=True)
      assert torch.equal(bits(avg), bits(want_avg))
      if perturbation == "std":
        assert torch.equal(bits(direction), bits(want_std))
  finally:
    assert lib.bm_tuning_set(b"BM_PERTURB_GRID", 0) == 0
  return worst


@pytest.mark.parametrize("h", HS + CLASS_EDGES)
def test_scalars_against_float64_sums_of_the_device_vectors(bm, h):
  worst = measure_scalars(bm, h)
  print(f"h = {h}: scalars, worst |error| / sum |terms| = {worst:.3e} (bar {BAR_SCALARS:.1e})")
  assert worst <= BAR_SCALARS


@pytest.mark.parametrize("h", [3, 20, 39, 64])
def test_scalars_with_the_grid_capped(bm, h):
  """d = 100 003 on two workgroups (+ the tail's): 49 iterations per lane at 16 bytes, 98 at 8, 196 at 4."""
  worst = measure_scalars_capped(bm, h)
  print(f"h = {h}, capped grid: scalars, worst |error| / sum |terms| = {worst:.3e} (bar {BAR_SCALARS:.1e})")
  assert worst <= BAR_SCALARS


def test_empty_vectors_give_zero_scalars(bm):
  rows = [torch.empty(0, dtype=torch.float32, device=DEV) for _ in range(5)]
  avg, direction, scal = bm.stats.perturb_stats(rows, "std")
  assert avg.numel() == 0 and direction.numel() == 0 and bool((scal == 0).all())


# ---------------------------------------------------------------------------- #
# (9)

@pytest.mark.parametrize("h", HS + CLASS_EDGES)
def test_same_bits_twice_and_device_factor_equals_host_factor(bm, h):
  for d, offset in ((63, 1), (4100, 0), (1027, 2)):
    rows = device_rows(host_rows(h, d), offset)
    sq = bm.gars.pairwise_sqdist(rows)
    for perturbation in R.PERTURBATIONS:
      first = bm.stats.perturb_stats(rows, perturbation)
      second = bm.stats.perturb_stats(rows, perturbation)
      for a, b in zip(first, second):
        assert torch.equal(bits(a), bits(b)), (h, d, perturbation)
      scal = first[2]
      for mode in R.MODES:
        dev = bm.stats.minmax_factor(sq, scal, h, mode)
        again = bm.stats.minmax_factor(sq, scal, h, mode)
        host = bm.stats.minmax_factor(sq.cpu().contiguous(), scal.cpu(), h, mode)
        assert dev.is_cuda and not host.is_cuda
        assert torch.equal(bits(dev.cpu()), bits(host)) and torch.equal(bits(dev), bits(again)), (h, d, perturbation, mode, dev, host)
        assert host[5] == 0.0 and host[0] > 0.0


# ---------------------------------------------------------------------------- #
# (10)

def measure_end_to_end(bm, h, d, structure):
  """(worst relative error of gamma, worst excess of the vector over its allowance in units of the allowance)"""
  rows32 = host_rows(h, d, structure, 4)
  rows = device_rows(rows32, 0)
  rows64 = rows32.astype(np.float64)
  worst_gamma = worst_vector = 0.0
  for perturbation in R.PERTURBATIONS:
    for fn, mode in ((bm.stats.minmax_attack, "minmax"), (bm.stats.minsum_attack, "minsum")):
      res = fn(rows, 2, perturbation=perturbation, unknown_keyword=1)
      assert len(res) == 2 and res[0] is res[1] and all(res[0].data_ptr() != r.data_ptr() for r in rows)
      byz = res[0]
      info = byz.attack_info.cpu().numpy()
      ref = R.attack(rows64, perturbation, mode)
      assert byz.attack_factor.is_cuda and info[5] == 0.0 and not ref["degenerate"]
      gamma = info[0]
      worst_gamma = max(worst_gamma, abs(gamma - ref["gamma"]) / ref["gamma"])
      if mode == "minmax":
        two = np.sort(ref["gammas"])[:2]
        if two[1] - two[0] > 1e-3 * two[1]:
          assert info[2] == ref["binding"], (h, d, structure, perturbation)
      else:
        assert info[2] == -1.0
      # tightness of the returned factor on the float64 vectors, with the slack of the bar (the constraint is
      # quadratic in gamma: twice the relative slack)
      value, limit = R.objective(rows64, ref["avg"] + gamma * ref["p"], mode)
      assert value <= limit * (1 + 2 * BAR_GAMMA + 1e-9), (h, d, structure, perturbation, mode, value, limit)
      beyond, _ = R.objective(rows64, ref["avg"] + gamma * (1 + 2 * BAR_GAMMA + 1e-6) * ref["p"], mode)
      assert beyond > limit, (h, d, structure, perturbation, mode, beyond, limit)
      # the vector: gamma's bar along p, plus the fp32 roundings of avg (h additions and a division), p and the sum
      allowed = BAR_GAMMA * gamma * np.abs(ref["p"]) + (h + 4) * 2.0 ** -24 * (np.abs(rows64).max(axis=0) + gamma * np.abs(ref["p"]))
      excess = np.abs(byz.cpu().numpy().astype(np.float64) - ref["vector"]) / np.maximum(allowed, 1e-300)
      worst_vector = max(worst_vector, float(excess.max()))
  return worst_gamma, worst_vector


END_TO_END = [(h, d, s) for h in (2, 11, 20, 39, 64) for d, s in ((1027, "iid"), (4100, "common"), (4100, "scaled"))]


@pytest.mark.parametrize("h,d,structure", END_TO_END)
def test_end_to_end_against_the_float64_reference(bm, h, d, structure):
  worst_gamma, worst_vector = measure_end_to_end(bm, h, d, structure)
  print(f"h = {h}, d = {d}, {structure}: gamma off by {worst_gamma:.3e} (bar {BAR_GAMMA:.1e}; 2e-6 allowed by the "
        f"distance pass), vector at {worst_vector:.3f} of its allowance")
  assert worst_gamma <= BAR_GAMMA and worst_vector <= 1.0


def test_degenerate_stacks_return_the_average(bm):
  x = torch.from_numpy(host_rows(1, 259)[0]).to(DEV)
  equal = [x.clone() for _ in range(4)]          # (four equal rows: their sequential fp32 mean is the row, exactly)
  opposite = [x.clone(), -x]                     # avg = 0
  poisoned = [t.clone() for t in device_rows(host_rows(5, 259))]
  poisoned[3][17] = float("nan")
  for rows, perturbation, flag in ((equal, "unit", 0.0), (equal, "std", 1.0), (equal, "sign", 0.0),
                                   (opposite, "unit", 1.0), (opposite, "sign", 1.0), (poisoned, "std", 1.0)):
    for fn in (bm.stats.minmax_attack, bm.stats.minsum_attack):
      byz = fn(rows, 1, perturbation=perturbation)[0]
      info = byz.attack_info.cpu()
      avg = bm.stats.stack_stats_async(rows)[0]
      assert info[5] == flag and info[0] == 0.0 and not np.signbit(info[0].item()), (perturbation, info)
      if rows is poisoned:
        assert bool(torch.isnan(byz[17])) and torch.equal(byz[:17], avg[:17]) and torch.equal(byz[18:], avg[18:])
      else:
        assert torch.equal(byz, avg), perturbation
  pair = device_rows(host_rows(2, 63))           # h = 2: the vector may sit as far from either row as they are apart
  info = bm.stats.minmax_attack(pair, 1, perturbation="unit")[0].attack_info.cpu()
  assert info[5] == 0.0 and info[0] > 0.0 and info[2] in (0.0, 1.0)


# ---------------------------------------------------------------------------- #
# (11)

@pytest.mark.parametrize("attack", R.MODES)
@pytest.mark.parametrize("gar", ["krum", "median", "dnc"])
def test_one_step_with_the_attack(bm, gar, attack):
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from byzantinemomentum_amd.step import AggregationStep
  n, f, d = 11, 2, 4100
  sampled = device_rows(host_rows(n - f, d, "common", 6))
  step = AggregationStep(n, f, f, gar=gar, momentum_at="update", attack=attack, nb_past=0,
                         attack_args={"perturbation": "sign"})
  assert not step.single_call and step.plan.first_pass == "plain"
  defense = step.run([g.clone() for g in sampled])
  fn = bm.stats.minmax_attack if attack == "minmax" else bm.stats.minsum_attack
  want = fn(sampled, f, perturbation="sign")[0]
  byz = step.last_byzantine
  assert torch.equal(bits(byz), bits(want)) and torch.equal(bits(byz.attack_info), bits(want.attack_info))
  assert step.last_factor is byz.attack_factor and step.last_factor.is_cuda and float(step.last_factor) > 0.0
  stack = sampled + [byz] * f
  rule = ShardedAggregator()
  want_def = rule.median(stack) if gar == "median" else getattr(rule, gar)(stack, f)
  assert torch.equal(bits(defense), bits(want_def))
  floats = step.floats()
  assert floats["attack_norm_avg"] > 0.0
