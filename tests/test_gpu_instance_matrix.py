"""Every compiled instance of the column kernels at each vector width and launch form (tests/instance_matrix.py).

Rows are cut out of one flat allocation so that they start at byte offsets 0, 4, 8 or a mix of them (VEC = 4 / 2 / 1),
the same values at every offset.  Each output is held to the suite's bar against a high-precision reference, and the
outputs of one input are bit-identical whichever instance computed them.  Knobs that choose an instance are read once
per process: those cases run in a child process that prints a SHA-256 per output, compared with the defaults here.
Needs an MI355X: `pytest -m gpu`.
"""

import json
import math
import os
import subprocess
import sys

import pytest
import torch

from oracle import gar_oracle as O
from tests import instance_matrix as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


@pytest.fixture(scope="module")
def cus():
  return torch.cuda.get_device_properties(0).multi_processor_count


def _stack_cols(rows, cols):
  st = torch.stack(rows) if cols is None else torch.stack([r[cols.to(r.device)] for r in rows])
  return st.cpu()


def _check_colwise(case, got, rows):
  """The suite's bar for a colwise output (every column, or the sampled ones of a long case)."""
  cols = M.sample_columns(case.d)
  st = _stack_cols(rows, cols)
  g = got if cols is None else got[cols.to(got.device)]
  bad = M.check_colwise(case.rule, case.f, g, st)
  assert int(bad.sum()) == 0, (case, int(bad.sum()), torch.nonzero(bad).flatten()[:8].tolist())


def _child(group, knobs, timeout):
  """The digests of `group` in a fresh process with `knobs` set (one attempt; a crash or a timeout fails the test)."""
  env = dict(os.environ, PYTHONPATH=ROOT, **{k: str(v) for k, v in knobs})
  try:
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "instance_matrix.py"), group], cwd=ROOT,
                          env=env, capture_output=True, text=True, timeout=timeout)
  except subprocess.TimeoutExpired as err:
    pytest.fail(f"{group} child timed out after {timeout} s: {(err.stderr or b'')[-2000:]!r}")
  assert done.returncode == 0, (group, done.returncode, done.stderr[-3000:])
  res = json.loads(done.stdout.strip().splitlines()[-1])
  assert all(res["knobs"][k] == str(v) for k, v in knobs), res["knobs"]
  return res["digests"]


def _compare_digests(group, cus, timeout, check=None):
  knobs = M.cases(group, cus)[0].knobs
  theirs = _child(group, knobs, timeout)
  ours = M.digests(group, cus, check=check)
  assert set(ours) == set(theirs) and len(ours) == len(M.cases(group, cus))
  differ = [k for k in ours if ours[k] != theirs[k]]
  assert not differ, (group, knobs, len(differ), differ[:8])


# ---------------------------------------------------------------------------------------------------------------------
# A. Coordinate-wise rules

@pytest.mark.parametrize("group", ["colwise_short", "colwise_long"])
def test_colwise_every_n_rule_and_width(bm, cus, group):
  """Every n = 1..64 x rule x rows at 0 / 4 / 8 bytes and mixed: the suite's bars against the references, and the same
  bits at every offset.  At 17 M coordinates every lane makes more than one grid-stride trip at each VEC, and the
  VEC-4 instances up to 22 / 25 rows run their burst form across staging groups (checked on sampled windows)."""
  todo = M.cases(group, cus)
  for n in range(1, M.BM_MAX_ROWS + 1):
    mine = [c for c in todo if c.n == n]
    vals, rowmap = M.colwise_values(n, mine[0].d, mine[0].f, M.colwise_seed(mine[0]))
    for rule in M.RULES:
      outs = {}
      for case in (c for c in mine if c.rule == rule):
        out, rows = M.run_colwise(case, vals, rowmap)
        if case.offset == 0:
          _check_colwise(case, out, rows)
        outs[case.offset] = out
      for off in M.OFFSETS[1:]:
        assert M.same_bits_strict(outs[off], outs[0]), (group, rule, n, off,
                                                       int((outs[off].view(torch.int32) != outs[0].view(torch.int32)).sum()))
    del vals


def test_colwise_every_f(bm, cus):
  """Every f = 1 .. (n-1)/2 at every n for the trimmed mean, phocas and meamed: each case of both f switches
  (trimmed_sum, closest_sum), n = 2f + 1 and (64, 31) included."""
  for case in M.cases("colwise_f", cus):
    out, rows = M.run_colwise(case)
    _check_colwise(case, out, rows)


def test_colwise_default_burst_thresholds_closest_rules(bm, cus):
  """phocas / meamed at n = 11 and 20 over a ResNet-18-sized gradient take the burst form under the default threshold
  (10.7 iterations per CU: across the 10-slot staging group): against the float64 window on the GPU, the way
  test_gpu_parity_r2.py::test_closest_rules_full_size checks n = 25."""
  for case in M.cases("colwise_resnet", cus):
    assert M.instances(case, cus) == {("colwise", case.rule, case.n, 4, "burst")}
    gen = torch.Generator(device=DEV).manual_seed(case.n)
    rows = [0.1 * i + torch.randn(case.d, device=DEV, generator=gen) for i in range(case.n)]
    rows[3][::1001] = rows[3][::1001].round()
    got = getattr(bm, case.rule)(rows, case.f)
    n, f, keep = case.n, case.f, case.n - case.f
    srt = torch.stack(rows).sort(dim=0).values
    centre = srt[(n - 1) // 2] if case.rule == M.MEAMED else srt[f:n - f].mean(dim=0)
    scale = float(srt.abs().max())
    want, tie = M.sorted_window(srt, keep, centre, 1e-6 * scale)
    bad = ((got.double() - want).abs() > 2e-6 * scale) & ~tie
    assert int(bad.sum()) == 0, (case, int(bad.sum()))
    assert int(tie.sum()) <= case.d // 1000, (case, "tie columns", int(tie.sum()))
    del srt, want, tie


@pytest.mark.parametrize("group,timeout", [("knob_burst", 600), ("knob_wide", 300)])
def test_colwise_knob_forms_give_the_same_bits(bm, cus, group, timeout):
  """BM_COL_BURST=1: every n <= 25 (median, trmean) / 22 (phocas, meamed) in the burst form at 1 and 1.5 iterations
  per CU plus a tail; BM_COL_WIDE=0: median / trmean at 29-52 rows with 8-byte columns, Aksel's pass 1 with 4-byte
  ones.  Each output's SHA-256 equals the default form's here, whose outputs are checked against the references."""
  _compare_digests(group, cus, timeout, check=_check_colwise)


# ---------------------------------------------------------------------------------------------------------------------
# B. Bulyan pass 2

def test_bulyan_pass2_every_fast_pair_and_width(bm, cus):
  """The 14 register-resident (n, f) instances at every width they can take (MMAX <= 20: 4, <= 44: 2; rows at 0 / 8 /
  4 bytes): the ranking of the (unaligned) Gram kernel equals the float64 oracle's, the output is within 2e-6 scale
  of the oracle's Bulyan, and bit-identical across widths."""
  for n, f in M.BULYAN_CASES:
    for d in M.D_BULYAN:
      stack = M.bulyan_stack(n, f, d)
      rows, h = stack[0], stack[1]
      want_order = O.bulyan_order(rows, f, None, "f64")[0]
      want = O.bulyan(rows, f)
      scale = float(torch.stack(rows[:h]).abs().max())
      outs = {}
      for case in (c for c in M.cases("bulyan", cus) if (c.n, c.f, c.d) == (n, f, d)):
        out, ranking, _ = M.run_bulyan(case, stack)
        assert ranking == want_order, (case, ranking, want_order)
        ok = M.check_close(out.cpu(), want, 2e-6, scale)
        assert bool(ok.all()), (case, int((~ok).sum()))
        outs[case.offset] = out
      assert M.same_bits_strict(outs[8], outs[0]) and M.same_bits_strict(outs[4], outs[0]), (n, f, d)


def test_bulyan_pass2_generic_neighbours(bm, cus):
  """(n, f) outside the table and m < m_max take the generic LDS kernel, at 0 and 4 bytes."""
  for case in M.cases("bulyan_generic", cus):
    stack = M.bulyan_stack(case.n, case.f, case.d)
    rows, h = stack[0], stack[1]
    out, ranking, _ = M.run_bulyan(case, stack)
    assert ranking == O.bulyan_order(rows, case.f, case.m, "f64")[0], case
    scale = float(torch.stack(rows[:h]).abs().max())
    assert bool(M.check_close(out.cpu(), O.bulyan(rows, case.f, case.m), 2e-6, scale).all()), case


def test_bulyan_short_window_knob_gives_the_same_bits(bm, cus):
  """BM_BULYAN_SHORT=0 (every window position searched) against the default short search: the same bits at every fast
  pair, width and length, as bm_common.h promises."""
  _compare_digests("knob_bulyan_short", cus, 600)


# ---------------------------------------------------------------------------------------------------------------------
# C. Aksel pass 1

def test_aksel_pass1_every_n_and_width(bm, cus):
  """Every n at 0 / 8 / 4 bytes (VEC 2 / 1, and the scalar tail launch): the selection equals the float64 oracle's, the
  rule's output the oracle's bit for bit, the median output bit-exact and identical across widths."""
  for n in range(1, M.BM_MAX_ROWS + 1):
    stack = M.aksel_stack(n, M.D_SHORT)
    rows = stack[0]
    f = n // 5
    want_sel = O.aksel_order(rows, "f64")[0][:(n + 1) // 2]
    want = O.aksel(rows, f)
    meds = {}
    for case in (c for c in M.cases("aksel", cus) if c.n == n):
      med, sq, sel, out, _ = M.run_aksel(case, stack)
      assert sel == want_sel, (case, sel, want_sel)
      assert torch.equal(out.cpu(), want), case
      assert bool(M.median_ok(med.cpu(), torch.stack(rows)).all()), case
      meds[case.offset] = med
    assert M.same_bits_strict(meds[8], meds[0]) and M.same_bits_strict(meds[4], meds[0]), n


# ---------------------------------------------------------------------------------------------------------------------
# D. Evaluate-only kernels and the other streaming entry points

def _flat_rows(tensors, off):
  """The tensors (equal lengths, on the GPU) copied into one allocation at byte offset `off`."""
  return M.place(torch.stack(tensors), off)


def test_colwise_eval_every_instance(bm, cus):
  """bm_colwise_eval at every instance and width against the per-evaluation form: the candidate written, the rule on
  the materialised stack, the objective |rule - avg|^2 in float64 (1e-5, the bar of the entry point in
  test_evaluate_only_search_form_against_the_per_evaluation_form)."""
  for case in M.cases("colwise_eval", cus):
    n, f, d = case.n, case.f, case.d
    gen = torch.Generator(device=DEV).manual_seed(17 * n + f)
    if case.rule == M.MEDIAN:
      base = [torch.randn(d, device=DEV, generator=gen) for _ in range(2)]
      honests = [torch.minimum(base[0], base[1]), torch.maximum(base[0], base[1])]
      copies = 1
    else:
      copies = f
      honests = [0.1 * i + torch.randn(d, device=DEV, generator=gen) for i in range(n - copies)]
      honests[0][::9] = honests[0][::9].round()
    avg = torch.stack(honests).mean(dim=0)
    direction = torch.randn(d, device=DEV, generator=gen)
    views = _flat_rows(honests + [avg, direction], case.offset)
    hv, av, dv = views[:-2], views[-2], views[-1]
    for t in (0.0, 0.7, -2.5):
      cand = torch.empty_like(avg)
      bm.stats.multi_fma3([cand], [avg], [direction], 1.0, t)
      rule = getattr(bm, case.rule)
      agg = rule(honests + [cand] * copies) if case.rule == M.MEDIAN else rule(honests + [cand] * copies, f)
      want = (agg.double() - avg.double()).pow(2).sum().item()
      got = bm.stats.colwise_eval(case.rule, hv, copies, f, av, dv, t).item()
      assert abs(got - want) <= 1e-5 * want, (case, t, got, want)


def test_bulyan_pass2_eval_every_instance(bm, cus):
  """bm_bulyan_pass2_eval at its three shapes and every width against the per-evaluation form in float64."""
  from byzantinemomentum_amd import _lib, gars
  for case in M.cases("bulyan_pass2_eval", cus):
    n, f, m, d = case.n, case.f, case.m, case.d
    gen = torch.Generator(device=DEV).manual_seed(97 + n)
    honests = [0.2 * torch.randn(d, device=DEV, generator=gen) + (0.5 + 0.05 * i) * torch.randn(d, device=DEV,
                                                                                              generator=gen)
               for i in range(n - f)]
    avg = torch.stack(honests).mean(dim=0)
    direction = -avg
    views = _flat_rows(honests + [avg, direction], case.offset)
    hv, av, dv = views[:-2], views[-2], views[-1]
    for t in (0.6, 7.5, -3.0):
      cand = torch.empty_like(avg)
      bm.stats.multi_fma3([cand], [avg], [direction], 1.0, t)
      rows = honests + [cand] * f
      gars.invalidate_rank_cache()
      order, _ = gars._rank(rows, f, m, _lib.RANK_BULYAN)
      want = (gars.bulyan_pass2(rows, order, f, m).double() - avg.double()).pow(2).sum().item()
      got = bm.stats.bulyan_pass2_eval(hv, f, order, f, m, av, dv, t).item()
      assert abs(got - want) <= 1e-5 * want, (case, t, got, want)


def test_order_pair_every_instance(bm, cus):
  """bm_order_pair at its three row buckets (h up to 51) and every width against a float64 sort: ranks in range, off
  either end (-inf / +inf), NaN columns; ties and infinities among the values."""
  for case in M.cases("order_pair", cus):
    h, d = case.n, case.d
    gen = torch.Generator(device=DEV).manual_seed(1000 + h)
    vals = torch.randn(h, d, device=DEV, generator=gen)
    vals[:, ::5] = vals[:, ::5].round()
    vals[0, 7::97] = math.inf
    vals[h - 1, 9::89] = -math.inf
    vals[h // 2, 11::101] = math.nan
    rows = M.place(vals, case.offset)
    st = vals.double().cpu()
    nan = torch.isnan(st).any(dim=0)
    srt = st.sort(dim=0).values
    for il, ih in ((-1, h), (0, h - 1), ((h - 1) // 2, h // 2), (h // 3 - 1, h - 2)):
      lo, hi = bm.stats.order_pair(rows, il, ih)
      for got, r in ((lo, il), (hi, ih)):
        want = torch.full((d,), -math.inf if r < 0 else math.inf, dtype=torch.float64) if r < 0 or r >= h else srt[r]
        want = torch.where(nan, torch.full_like(want, math.nan), want)
        got = got.cpu().double()
        assert torch.equal(torch.isnan(got), torch.isnan(want)), (case, r)
        assert torch.equal(got[~nan], want[~nan]), (case, r)


def test_sums_of_squares_and_axpby_at_every_width(bm, cus):
  """bm_sqdist2 and bm_row_sqnorms against float64 (1e-6), bm_multi_axpby against a float64 axpby rounded to fp32
  (1e-6), at rows of 0 / 4 / 8 bytes and a mix; so bm_multi_dot (1e-6 of |a| |b|), bm_multi_fma3 with its factor as a
  number and in device memory (1e-6) and bm_multi_scale (a power of two: exact; a factor 1: untouched)."""
  d = 300007
  gen = torch.Generator(device=DEV).manual_seed(3)
  vals = (1.0 + torch.arange(6, device=DEV)[:, None]) * torch.randn(6, d, device=DEV, generator=gen)
  v64 = vals.double()
  for off in M.OFFSETS:
    rows = M.place(vals, off)
    want = (v64[0] - v64[1]).pow(2).sum().item()
    assert abs(bm.stats.sqdist2(rows[0], rows[1]).item() - want) <= 1e-6 * want, off
    got = bm.stats.row_sqnorms(rows).tolist()
    for g, w in zip(got, v64.pow(2).sum(dim=1).tolist()):
      assert abs(g - w) <= 1e-6 * w, (off, g, w)
    gram, extra = bm.stats.study_dots(rows[:2], rows[2:4])
    norm = v64.pow(2).sum(dim=1).sqrt().tolist()
    for i in range(2):
      for j in range(2):
        assert abs(gram[i, j].item() - torch.dot(v64[i], v64[j]).item()) <= 1e-6 * norm[i] * norm[j], (off, i, j)
      assert abs(extra[i].item() - torch.dot(v64[0], v64[2 + i]).item()) <= 1e-6 * norm[0] * norm[2 + i], (off, i)
    for b in (0.1, torch.tensor([0.1], dtype=torch.float64, device=DEV)):
      outs = M.place(torch.zeros(2, d, device=DEV), off)
      bm.stats.multi_fma3(outs, rows[:2], rows[2:4], 0.99, b)
      for i, o in enumerate(outs):
        want = (0.99 * v64[i] + 0.1 * v64[2 + i]).float()
        assert bool(M.check_close(o.cpu(), want.cpu(), 1e-6, float(want.abs().max())).all()), (off, i)
    ys, xs = rows[:3], rows[3:]
    bm.stats.multi_axpby(ys, xs, 0.99, 0.1)
    for y, i in zip(ys, range(3)):
      want = (0.99 * v64[i] + 0.1 * v64[3 + i]).float()
      ok = M.check_close(y.cpu(), want.cpu(), 1e-6, float(want.abs().max()))
      assert bool(ok.all()), (off, i)
    factors = torch.ones(64, device=DEV)
    factors[0] = 0.5
    bm.stats.multi_scale(rows[4:], factors)
    assert torch.equal(rows[4], 0.5 * vals[4]) and torch.equal(rows[5], vals[5]), off


@pytest.mark.parametrize("n", [3, 11, 25, 51, 64])
def test_means_and_statistics_at_every_width(bm, cus, n):
  """average, Krum and CGE (the selected-mean kernel) and the statistics pass at rows of 0 / 4 / 8 bytes and mixed, at
  the bars of test_unaligned_rows_and_tails; the first pass of a step (bm_momentum_stats, the rows as sampled gradients
  and as many buffers, 63 at most) at the bars of test_momentum_stats_kernel_tiers, and the study block (bm_study_stats_update) at
  those of test_study_stats_against_fp64."""
  f = {3: 0, 11: 2, 25: 5, 51: 12, 64: 15}[n]
  d = 4099
  rows, h = O.make_stack("hetero", n, f, d, seed=41 * n)
  distinct, rowmap = M.distinct_rows(rows)
  krum_order = O.krum_order(rows, f, "f64")[0][:n - f - 2]
  want_krum, want_avg, want_cge = O.krum(rows, f), O.average(rows), O.cge(rows, f)
  wavg, wnorm, wdev, wmx = O.compute_avg_dev_max(rows, "f64")
  want_stats_avg = O.compute_avg_dev_max(rows)[0]
  gen = torch.Generator().manual_seed(5 * n)
  hb = min(n, 63)  # (the wrapper validates the buffers and one gradient as one list of at most 64)
  bufs = torch.randn(hb, d, generator=gen)
  want_bufs = [b.clone().mul_(0.9).add_(g, alpha=0.1) for b, g in zip(bufs, rows)]
  wh_avg, wh_norm, wh_dev, wh_max = O.compute_avg_dev_max(want_bufs, "f64")
  want_h_avg = O.compute_avg_dev_max(want_bufs)[0]
  study = torch.randn(10, d, generator=gen).to(DEV)   # s, h, defense, byz, past, oldest, params, origin, C, M
  s64 = study.double()
  for off in M.OFFSETS:
    dev = M.rows_of(M.place(distinct, off), rowmap)
    bm.gars.invalidate_rank_cache()
    assert bm.gars.krum_selection(dev, f) == krum_order, (n, off)
    assert torch.equal(bm.krum(dev, f).cpu(), want_krum), (n, off)
    assert torch.equal(bm.average(dev).cpu(), want_avg), (n, off)
    assert torch.equal(bm.cge(dev, f).cpu(), want_cge), (n, off)
    avg, norm, devi, mx = bm.compute_avg_dev_max(dev)
    assert torch.equal(avg.cpu(), want_stats_avg), (n, off)
    assert abs(norm - wnorm) <= 1e-6 * wnorm and abs(devi - wdev) <= 1e-6 * wdev and abs(mx - wmx) <= 1e-6 * wmx
    dbufs = M.place(bufs.to(DEV), off)
    s_avg, h_avg, _, out6 = bm.stats.momentum_stats(dev, dbufs, 0.9, 0.1)
    for a, b in zip(dbufs, want_bufs):
      assert float((a.cpu() - b).abs().max()) <= 1e-6 * float(b.abs().max()), (n, off)
    assert torch.equal(s_avg.cpu(), want_stats_avg), (n, off)
    assert float((h_avg.cpu() - want_h_avg).abs().max()) <= 2e-7 * wh_max, (n, off)
    o = out6.tolist()
    for got, want in ((math.sqrt(o[0]), wnorm), (math.sqrt(o[1] / (n - 1)), wdev), (o[2], wmx),
                      (math.sqrt(o[3]), wh_norm), (math.sqrt(o[4] / (hb - 1)), wh_dev), (o[5], wh_max)):
      assert abs(got - want) <= 1e-5 * want, (n, off, got, want)
    s, h, df, byz, past, old, par, org, curv, mom = M.place(study, off)
    mu, w = 0.9, -(0.9 ** 4)
    out = bm.stats.study_stats(s, h, df, byz, 2, past_newest=past, curv=curv, past_oldest=old, curv_mode=3, mu=mu,
                               oldest_weight=w, params=par, origin=org, update_momentum=mom, update_mu=0.9,
                               update_omd=0.1).tolist()
    c64 = [s64[0], s64[1], s64[2], ((study[3] + study[3]) / torch.full_like(study[3], 2.0)).double()]
    for i in range(4):
      for j in range(4):
        scale = math.sqrt(float(c64[i].pow(2).sum()) * float(c64[j].pow(2).sum()))
        assert abs(out[4 * i + j] - float(torch.dot(c64[i], c64[j]))) <= 1e-6 * scale, (n, off, i, j)
    for slot, other in ((16, s64[4]), (17, s64[8])):
      scale = math.sqrt(float(c64[0].pow(2).sum()) * float(other.pow(2).sum()))
      assert abs(out[slot] - float(torch.dot(c64[0], other))) <= 1e-6 * scale, (n, off, slot)
    want_l2 = float((s64[6] - s64[7]).pow(2).sum())
    assert abs(out[22] - want_l2) <= 1e-6 * want_l2 and out[21] == float(study[2].abs().max()), (n, off)
    want_c = study[0] + mu * torch.addcmul(study[8], torch.full_like(study[5], w), study[5])  # fma(w, oldest, C)
    assert float((curv - want_c).abs().max()) <= 2e-7 * float(want_c.abs().max()), (n, off)
    want_m = (0.1 * s64[2] + 0.9 * s64[9]).float()
    assert bool(M.check_close(mom.cpu(), want_m.cpu(), 1e-6, float(want_m.abs().max())).all()), (n, off)
