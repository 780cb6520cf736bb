"""The in-place streaming kernels of the step bit for bit, the scalar reductions beside them at the project's bars, and
the ranking cache behind every routine that writes user tensors (tests/inplace_matrix.py; its reach proofs and mutation
checks are in tests/test_inplace_matrix_cpu.py).

Every vector of a case lies in one flat allocation between guard gaps of a sentinel.  After each call the WHOLE
allocation is compared: the outputs bit for bit against the CPU reference (where both sides are NaN that is the
comparison: payloads are not specified), every guard gap and every input that is not an output unchanged.  No
coordinate is left out.  Needs an MI355X: `pytest -m gpu`."""

import math

import numpy as np
import pytest
import torch

from tests import inplace_matrix as X

pytestmark = pytest.mark.gpu
F32 = np.float32
DEV = X.DEV


@pytest.fixture(scope="module")
def bm():
  return X._bm()


def _run_writers(todo):
  assert todo
  for case in todo:
    got, pre = X.run_writer(case)
    assert X.check_writer(case, got, pre) is None, X.check_writer(case, got, pre)
  return len(todo)


# ---------------------------------------------------------------------------------------------------------------------
# The four writers

@pytest.mark.parametrize("k", X.K_SHORT)
@pytest.mark.parametrize("entry", (X.AXPBY, X.FMA3, X.SCALE))
def test_writer_at_the_short_lengths(bm, entry, k):
  """Every width with the tail alone, a body without a tail, a tail of 1, 2 and 3 columns behind a body, one workgroup
  and several, at rows 0 / 4 / 8 bytes behind a 16-byte boundary and a mix; k = 64 of axpby and fma3 through the C entry
  points (the wrappers validate at most 64 tensors in one list)."""
  todo = X.writer_cases("short", entry, k)
  assert {i for c in todo for i in X.instances(entry, X.writer_pointers(c), c.d)} == {(X.SITES[entry].kernel, w) for w in (1, 2, 4)}
  assert _run_writers(todo) == len(X.D_SHORT) * len(X.OFFSETS)


def test_anticge_scale_at_the_short_lengths(bm):
  """bm_anticge_scale with an ordinary multiplier: the device's own multiplier (anticge_reference.multiplier_of on the
  ordinary elements) is within 1e-6 of the float64 one, and the whole vector — special elements included — is
  fl32(v m) of that multiplier bit for bit."""
  _run_anticge(X.writer_cases("short", X.ANTICGE))


def _run_anticge(todo):
  for case in todo:
    got, pre = X.run_writer(case)
    pre, m_dev, want64 = X.with_device_multiplier(case, got, pre)
    if want64 is not None:
      print(case.d, case.out_off, "multiplier", m_dev, "float64", want64, "restated", float(pre.args["multiplier"]))
      assert m_dev is not None and abs(m_dev - want64) <= 1e-6 * abs(want64), (case, m_dev, want64)
    assert X.check_writer(case, got, pre) is None, X.check_writer(case, got, pre)


@pytest.mark.parametrize("entry", (X.AXPBY, X.FMA3))
def test_widths_forced_by_one_side(bm, entry):
  """Only the outputs 4 or 8 bytes off with aligned inputs, and the inverse: the width follows the narrower side."""
  assert _run_writers(X.writer_cases("forced", entry)) == 8


@pytest.mark.parametrize("width", (1, 2, 4))
@pytest.mark.parametrize("entry", X.WRITERS)
def test_second_trip_of_the_grid_stride_loop(bm, entry, width):
  """The capped grid of 2048 workgroups with one whole workgroup on a second trip and the widest tail behind it; every
  element of every row and of the gaps is compared."""
  todo = [c for c in X.writer_cases("second_trip", entry) if X.writer_launches(c)[0].width == width]
  assert len(todo) == 1 and X.writer_launches(todo[0])[0].trips == 2
  if entry == X.ANTICGE:
    _run_anticge(todo)
  else:
    _run_writers(todo)


@pytest.mark.parametrize("pscale", (False, True))
@pytest.mark.parametrize("form", ("inplace", "fresh", "shared_q", "nesterov"))
def test_fma3_forms_and_both_entry_points(bm, form, pscale):
  """out = p, out fresh, one q shared by every row, the Nesterov look-ahead (k = 1, a = 1); b as a number and as a
  device float64; with and without clipping factors (some exactly 1).  Both entry points give the same bits."""
  todo = [c for c in X.writer_cases("fma3_forms", X.FMA3) if c.form == form and c.pscale == pscale]
  assert {c.bdev for c in todo} == {False, True}
  images = {}
  for case in todo:
    got, pre = X.run_writer(case)
    assert X.check_writer(case, got, pre) is None, X.check_writer(case, got, pre)
    images[case] = got
    # through the C entry point as well
    got_c, _ = X.run_writer(case, pre, entry_point="c")
    assert np.array_equal(got_c, got), case
  for case, got in images.items():
    if not case.bdev:
      assert np.array_equal(got, images[case._replace(bdev=True)]), case


def test_scale_factors_and_the_untouched_rows(bm):
  """Powers of two and arbitrary factors; a factor of exactly 1 on a row of signalling-NaN bit patterns and -0 (a
  multiply by 1 would quiet the NaNs: the row must come back with its bits); a factor 0."""
  todo = X.writer_cases("scale_special", X.SCALE)
  for case in todo:
    if case.special == "one_on_snan":
      pre = X.prepare(case)
      assert pre.outputs[0][1] and set(pre.outputs[0][0].view(np.uint32).tolist()) <= set(X.SNAN_BITS)
  _run_writers(todo)


def test_anticge_scale_multipliers(bm):
  """An ordinary multiplier; |S|^2 = 0 and NaN: the vector untouched bit for bit; an infinite Byzantine norm."""
  todo = X.writer_cases("anticge_special", X.ANTICGE)
  for case in todo:
    pre = X.prepare(case)
    assert pre.outputs[0][1] == (case.special in ("zero_norm", "nan_norm"))
  _run_anticge(todo)


# ---------------------------------------------------------------------------------------------------------------------
# The clip chain

@pytest.mark.parametrize("k", (1, 64))
def test_clip_factors_bit_exact(bm, k):
  clip = 2.5
  c2 = float(np.float64(F32(clip)) ** 2)
  crafted = [c2 * 0.99, c2, float(np.nextafter(c2, np.inf)), 0.0, math.inf, math.nan, 4 * c2, c2 * (1 + 1e-9), 1e-300, 1e300]
  rng = np.random.default_rng(k)
  for start in range(len(crafted) if k == 1 else 1):
    sq = np.array((crafted[start:] + crafted[:start] + list(rng.uniform(0.0, 3 * c2, size=64)))[:k], dtype=np.float64)
    got = bm.stats.clip_factors_from_sq(torch.from_numpy(sq).to(DEV), k, clip)[:k].cpu().numpy()
    want = X.clip_factors_reference(sq, clip)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (k, sq.tolist(), got.tolist(), want.tolist())


@pytest.mark.parametrize("off", X.OFFSETS)
def test_clip_gradients_end_to_end(bm, off):
  """Rows of norm <= clip come back with their bits; the others are fl32(y c) of the device's own factor, which is
  within 1e-6 of clip / |y| in float64; gaps intact."""
  k, d = 20, 1027
  v = X.finite_values(k, d).copy()
  norms = np.sqrt((v.astype(np.float64) ** 2).sum(axis=1))
  clip = float(F32(0.5 * (norms[9] + norms[10])))          # rows of scale 1 .. 10 below, 11 .. 20 above
  flat = X.Flat(list(v), X.row_offsets(off, k))
  dev, views = X.upload(flat)
  factors = bm.stats.clip_gradients(views, clip)[:k].cpu().numpy()
  torch.cuda.synchronize()
  below = norms <= clip
  assert 5 <= below.sum() <= 15
  assert (factors[below] == 1.0).all()
  want64 = clip / norms[~below]
  assert (np.abs(factors[~below] - want64) <= 1e-6 * want64).all(), (factors[~below], want64)
  want = v * factors[:, None]
  want[below] = v[below]
  image, loose = flat.expected({i: (want[i], bool(below[i])) for i in range(k)})
  at = X.first_mismatch(X.download(dev), image, loose)
  assert at is None, (off, flat.where(at))


# ---------------------------------------------------------------------------------------------------------------------
# The reductions, at the project's bars

def _run_reductions(todo):
  worst = 0.0
  for case in todo:
    v = X.reduction_input(case)
    res, bits, flat = X.run_reduction(case, v)
    assert np.array_equal(bits, flat.bits), (case, "an input or a guard gap was written")
    err, misses = X.check_reduction(case, res, v)
    assert not misses, (case, misses[:3], [tuple(l) for l in X.reduction_launches(case)])
    worst = max(worst, err)
  print(f"{len(todo)} cases, worst error {worst:.3f} of the bar")
  return worst


@pytest.mark.parametrize("k", X.K_SHORT)
def test_row_sqnorms_at_the_short_lengths(bm, k):
  _run_reductions([c for c in X.reduction_cases(X.SQNORMS, "short") if c.k == k])


@pytest.mark.parametrize("index", (0, 1))
def test_row_sqnorms_fold_and_remainder(bm, index):
  """Every lane passes the fp32 -> fp64 fold and most then take the single-load remainder: 4-byte rows, and the 16-byte
  form with a 3-column tail."""
  case = X.reduction_cases(X.SQNORMS, "fold")[index]
  w = X.sqnorm_walk(X.reduction_launches(case)[0].count, 128)
  assert w.folds == 128 * 256 and w.remainder_after_fold > 0
  _run_reductions([case])


def test_row_sqnorms_partial_areas_and_non_finite_rows(bm):
  """k = 64 with the body and the tail area both in use, and each alone with several workgroups; a NaN row and an
  infinite row next to finite ones."""
  _run_reductions(X.reduction_cases(X.SQNORMS, "areas") + X.reduction_cases(X.SQNORMS, "nonfinite"))
  case = X.reduction_cases(X.SQNORMS, "nonfinite")[0]
  res, _, _ = X.run_reduction(case)
  assert math.isnan(res[1]) and res[3] == math.inf and np.isfinite(res[[0, 2, 4]]).all()


def test_sqdist2_short_equal_and_empty(bm):
  todo = [c for c in X.reduction_cases(X.SQDIST2) if c.group != "fold"]
  _run_reductions(todo)
  for case in todo:
    if case.group in ("equal", "empty"):
      res, _, _ = X.run_reduction(case)
      assert res[0] == 0.0 and not np.signbit(res[0]), case


def test_sqdist2_fold(bm):
  """The shortest length at which a lane folds; that lane's columns carry the weight of the sum."""
  (case,) = X.reduction_cases(X.SQDIST2, "fold")
  v = X.reduction_input(case)
  stride = X.SITES[X.SQDIST2].cap_tail * 256
  hot = float(((v[0, ::stride].astype(np.float64) - v[1, ::stride]) ** 2).sum())
  total = X.reduction_reference(case, v)
  assert hot > 0.5 * total
  res, bits, flat = X.run_reduction(case, v)
  err, misses = X.check_reduction(case, res, v)
  print(f"sqdist2 fold: {err:.3f} of the bar")
  assert not misses, misses
  assert np.array_equal(bits, flat.bits)


@pytest.mark.parametrize("nc", (1, 2, 3, 4))
def test_multi_dot_every_slot(bm, nc):
  """Every Gram entry, its transpose and every extra at ne = 0, 1, 31, 32; the doubles of `out` beyond nc^2 + ne keep
  what the caller put there."""
  _run_reductions([c for c in X.reduction_cases(X.DOT) if c.nc == nc])


# ---------------------------------------------------------------------------------------------------------------------
# The ranking cache: every routine that writes user tensors is followed by a fresh ranking

N, F, D = 11, 2, 1027
TAGS = ("krum", "bulyan", "brute", "aksel")


def _select(bm, tag, rows):
  g = bm.gars
  return {"krum": g.krum_selection, "bulyan": g.bulyan_ranking, "brute": g.brute_selection, "aksel": g.aksel_selection}[tag](rows, F)


def _cluster(seed, outlier_first=False):
  """11 rows around a common centre, row 0 the centre itself (or, outlier_first, 1000 times it); a source vector far
  from all of them; the centre's norm."""
  rng = np.random.default_rng(seed)
  centre = rng.standard_normal(D).astype(F32)
  rows = [centre + F32(0.05 * (1 + 0.2 * i)) * rng.standard_normal(D).astype(F32) for i in range(N)]
  rows[0] = centre * F32(1000.0) if outlier_first else centre.copy()
  far = (30.0 * rng.standard_normal(D)).astype(F32)
  return [torch.from_numpy(r).to(DEV) for r in rows], torch.from_numpy(far).to(DEV), float(np.linalg.norm(centre.astype(np.float64)))


def _sampled_for(far):
  """Sampled gradients that move buffer 0 alone under mu = 1: the far vector, then zeros."""
  return [far] + [torch.zeros_like(far) for _ in range(N - 1)]


def _writer(bm, name, rows, far, norm):
  s = bm.stats
  if name == "multi_axpby":
    s.multi_axpby([rows[0]], [far], 1.0, 100.0)
  elif name == "multi_fma3":
    s.multi_fma3([rows[0]], [rows[0]], [far], 1.0, 100.0)
  elif name == "multi_fma3_bdev":
    s.multi_fma3([rows[0]], [rows[0]], [far], 1.0, torch.tensor([100.0], dtype=torch.float64, device=DEV))
  elif name == "multi_scale":
    factors = torch.ones(64, device=DEV)
    factors[0] = 1000.0
    s.multi_scale(rows, factors)
  elif name == "clip_gradients":
    s.clip_gradients(rows, norm)
  elif name == "anticge_scale":
    s.anticge_scale(rows[0], torch.tensor([1.0, 1e6], dtype=torch.float64, device=DEV))
  elif name == "momentum_stats":
    s.momentum_stats(_sampled_for(far), rows, 1.0, 100.0)
  elif name == "momentum_stats_colwise":
    s.momentum_stats_colwise(_sampled_for(far), rows, 1.0, 100.0, None, 1.1, "empire", "median", F, F)
  elif name == "momentum_stats_sqdist":
    s.momentum_stats_sqdist(_sampled_for(far), rows, 1.0, 100.0, None, 1.1, "empire", F)
  elif name == "study_stats":
    s.study_stats(rows[1], rows[2], far, rows[3], F, update_momentum=rows[0], update_mu=1.0, update_omd=100.0)
  else:
    raise ValueError(name)


WRITERS = ("multi_axpby", "multi_fma3", "multi_fma3_bdev", "multi_scale", "clip_gradients", "anticge_scale", "momentum_stats",
           "momentum_stats_colwise", "momentum_stats_sqdist", "study_stats")


def _follows(bm, tag, rows, first, what):
  second = _select(bm, tag, rows)
  fresh = _select(bm, tag, [r.clone() for r in rows])
  assert second == fresh, (what, tag, "a ranking of earlier contents was reused", first, second, fresh)
  assert second != first, (what, tag, "the writer did not move the ranking: the case proves nothing")
  return second


@pytest.mark.parametrize("name", WRITERS)
def test_ranking_is_fresh_after_every_writer(bm, name):
  """krum_selection fills the cache; the writer makes one row a far outlier (clip_gradients: brings the outlier in) on
  the device alone, no torch op touches the rows; the next selection is that of fresh clones of the contents and differs
  from the first.  The same for the bulyan, brute and aksel entries of the cache."""
  for i, tag in enumerate(TAGS):
    rows, far, norm = _cluster(100 + i, outlier_first=name == "clip_gradients")
    versions = [r._version for r in rows]
    first = _select(bm, tag, rows)
    assert _select(bm, tag, rows) == first
    _writer(bm, name, rows, far, norm)
    assert [r._version for r in rows] == versions                   # the cache cannot have seen the write that way
    _follows(bm, tag, rows, first, name)


@pytest.mark.parametrize("single_call", (True, False))
def test_ranking_is_fresh_after_a_step(bm, single_call):
  """AggregationStep.run at the worker placement writes its momentum buffers: rankings of the buffers follow."""
  from byzantinemomentum_amd.step import AggregationStep
  for i, tag in enumerate(TAGS):
    rows, far, _ = _cluster(200 + i)
    step = AggregationStep(N + F, F, F, gar="median", momentum=0.5, dampening=0.5, attack_factor=1.1, nb_past=2,
                           single_call=single_call)
    step.run(rows)
    buffers = list(step.buffers)
    assert len(buffers) == N
    first = _select(bm, tag, buffers)
    step.run([far * 100.0] + rows[1:])
    _follows(bm, tag, buffers, first, f"step single_call={single_call}")


def test_ranking_is_fresh_after_a_graph_replay(bm):
  """A recorded multi_fma3(row 0 <- src) replayed between eager rankings: each replay may have written anything, so the
  ranking after it must be computed from the contents (GraphedCall forgets the cached rankings)."""
  from byzantinemomentum_amd.graphs import GraphedCall
  for i, tag in enumerate(TAGS):
    rows, far, _ = _cluster(300 + i)
    src, zeros, centre = rows[0].clone(), torch.zeros_like(rows[0]), rows[0].clone()
    graph = GraphedCall(lambda: bm.stats.multi_fma3([rows[0]], [src], [zeros], 1.0, 0.0))   # idempotent: row 0 <- src
    assert torch.equal(rows[0], centre)
    first = _select(bm, tag, rows)
    src.copy_(far * 100.0)
    graph()
    torch.cuda.synchronize()
    assert torch.equal(rows[0], src)
    second = _follows(bm, tag, rows, first, "graph replay")
    src.copy_(centre)
    graph()
    third = _select(bm, tag, rows)
    assert third == first and third != second, (tag, first, second, third)
