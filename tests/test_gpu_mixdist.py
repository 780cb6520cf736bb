"""Distance-based rules on mixed rows from scalars, on the GPU.  Every stage is tested GIVEN the device's own output of
the stage before it, so that a near-tie in one stage cannot fail the next:
  1. the device forms of bm_mixed_sqdist / bm_mix_weights bit for bit against the host forms, on the matrix and the
     masks the device computed;
  2. the mixed distances against the float64 distances of float64 mixed rows built from the device's masks;
  3. the ranking of the mixed distances against the float64 Krum order, up to ties within the bars of 2;
  4. the output of nnm(form="scalars") against the definition of bm_weighted_sum on the device's composed weights, bit
     for bit, and against the float64 weighted sum;
  5. end to end on crafted inputs on which form="rows", form="scalars" and float64 must select the same rows;
  6. NaN attack copies;  7. a graph replay.
Lines starting with "mixdist_error" are what profiles/mixdist_errors.txt records.  Needs an MI355X: `pytest -m gpu`."""

import functools
import math

import numpy as np
import pytest
import torch

from tests import center_cases as cc
from tests import mixdist_cases as mc
from tests import nnm_cases as nc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = ((7, 1), (11, 2), (25, 5), (51, 12), (64, 15))
LENGTHS = (1027, 3074)
BAR = cc.BAR_B["geomed"]     # relative L2 error of an fp32 weighted sum against float64 (tests/test_gpu_center_rules.py)


@pytest.fixture(scope="module")
def bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


def _upload(host):
  """Rows cut from ONE allocation, each at byte offset 0 of a 256-byte boundary; entries that are one object on the host
  are one tensor on the device."""
  n, d = len(host), host[0].shape[0]
  per = -(-d // 64) * 64
  pool = torch.zeros(n * per, dtype=torch.float32, device=DEV)
  seen, dev = {}, []
  for i, h in enumerate(host):
    if id(h) not in seen:
      view = pool[i * per:i * per + d]
      view.copy_(torch.from_numpy(h))
      seen[id(h)] = view
    dev.append(seen[id(h)])
  return dev


def _words(masks, count):
  return nc.from_int64(masks[:count].tolist())


def _masks(words):
  return torch.tensor(nc.to_int64(words), dtype=torch.int64, device=DEV)


@functools.lru_cache(maxsize=None)
def _host_rows(kind, n, f, d):
  if kind == "random":
    return tuple(nc.random_rows(n, d, seed=1000 * n + d))
  if kind == "ladder":
    return tuple(nc.ladder_rows(n, d, 1.15, seed=n + d))
  honest = nc.random_rows(n - f + 1, d, seed=77 * n + d)      # "aliased-far": f references to ONE far row
  far = (honest[-1] * np.float32(30.0)).astype(np.float32)
  return tuple(honest[:n - f]) + (far,) * f


KINDS = ("random", "ladder", "aliased-far")


def _pair_bars(sq64, n_in, words, terms, ref, d):
  """The bar of every pair (a, b): 1e-5 * 1/2 sum |w_i| |w_j| D_ij (the distance pass's own relative bar, through the
  quadratic form) + 2^-40 of the three terms (the fp64 sums) + d 2^-53 of the reference (its own summation)."""
  W = np.stack([mc.weights_of(w, n_in) if w else np.zeros(n_in) for w in words])
  n_out = len(words)
  bars = np.zeros((n_out, n_out))
  for a in range(n_out):
    diff = np.abs(W[a][None, :] - W)
    bars[a] = mc.PASS_BAR * 0.5 * np.einsum("bi,ij,bj->b", diff, sq64, diff)
    for b in range(n_out):
      if terms[a][b] is not None:
        bars[a, b] += mc.SUM_BAR * sum(terms[a][b]) + d * mc.EPS64 * ref[a, b]
  return bars


@functools.lru_cache(maxsize=None)
def _stage(kind, n, f, d):
  """Everything one (kind, n, f, d) needs, computed once: the device's matrix, masks and mixed distances, and the float64
  references built from the DEVICE's masks."""
  import byzantinemomentum_amd as bm
  host = list(_host_rows(kind, n, f, d))
  dev = _upload(host)
  sq = bm.gars.pairwise_sqdist(dev)
  masks = bm.gars.nnm_masks(sq, n, f)
  mixed = bm.gars.mixed_sqdist(sq, n, masks, n)
  words = _words(masks, n)
  sq64 = nc.sqdist64(host)
  y64 = mc.mixed_rows64(host, words)
  ref = nc.sqdist64(y64)
  _, terms = mc.mixed_reference(sq64, n, words)
  bars = _pair_bars(sq64, n, words, terms, ref, d)
  return dict(host=host, dev=dev, sq=sq, masks=masks, mixed=mixed, words=words, sq64=sq64, y64=y64, ref=ref, bars=bars)


# ---------------------------------------------------------------------------- #
# 1. device = host, bit for bit

@pytest.mark.parametrize("n,f", SHAPES)
def test_device_forms_equal_host_forms(bm, n, f):
  g = bm.gars
  for d in LENGTHS:
    st = _stage("random", n, f, d)
    sq, sq_host = st["sq"], st["sq"].cpu()
    sets = [("nnm", st["masks"][:n].clone())]
    sets.append(("random", _masks(mc.visible(nc.random_masks(n, min(64, n + 3), seed=n + d), n))))
    sets.append(("buckets", _masks(mc.bucket_words(n, 3, seed=n))))
    sets.append(("empty-and-equal", _masks([st["words"][0], 0, st["words"][0]] + st["words"][1:4])))
    for name, masks in sets:
      n_out = masks.numel()
      got = g.mixed_sqdist(sq, n, masks, n_out)
      want = g.mixed_sqdist(sq_host, n, masks.cpu(), n_out)
      assert got.is_cuda and got.shape == (n_out, n_out) and got.dtype == torch.float64
      assert mc.same_bits64(got.cpu().numpy(), want.numpy()), (n, d, name)
      # the weights the device's own next stages leave: a ranking, and the weights of the geometric median
      if name == "empty-and-equal":
        continue
      if n_out - f - 2 >= 1:
        m = n_out - f - 2
        order, _ = g.rank_from_sqdist(got, n_out, f, m, bm._lib.RANK_KRUM)
        w_dev = g.mix_weights(masks, n, n_out, selection=order, m=m)
        w_host = g.mix_weights(masks.cpu(), n, n_out, selection=order.cpu(), m=m)
        assert w_dev.is_cuda and mc.same_bits64(w_dev.cpu().numpy(), w_host.numpy()), (n, d, name, "selection")
        assert mc.same_bits64(w_host.numpy(), mc.weights_reference(_words(masks, n_out), n, sel=order.tolist(), m=m))
      cw, _ = g.center_weights(got, n_out, "geomed", 1e-6, 4)
      w_dev = g.mix_weights(masks, n, n_out, weights=cw)
      w_host = g.mix_weights(masks.cpu(), n, n_out, weights=cw.cpu())
      assert mc.same_bits64(w_dev.cpu().numpy(), w_host.numpy()), (n, d, name, "weights")
      assert abs(float(w_dev.sum()) - 1.0) <= 64 * 2.0 ** -52


def test_device_forms_poison_what_the_host_forms_refuse_or_poison(bm):
  g = bm.gars
  n = 11
  st = _stage("random", n, 2, 1027)
  masks = st["masks"][:n].clone()
  bad = masks.clone()
  bad[4] |= 1 << n                                      # a bit at n_in: the host refuses, the device writes NaN everywhere
  assert torch.isnan(g.mixed_sqdist(st["sq"], n, bad, n)).all()
  with pytest.raises(RuntimeError):
    g.mixed_sqdist(st["sq"].cpu(), n, bad.cpu(), n)
  even = torch.full((64,), 1.0 / n, dtype=torch.float64, device=DEV)
  w = g.mix_weights(bad, n, n, weights=even)
  assert torch.isnan(w[:n]).all() and not w[n:].any()
  # a negative index, a selection of the empty mask, a weight on the empty mask; a zero weight there is skipped
  sel = torch.tensor([0, 1, -1, 3], dtype=torch.int32, device=DEV)
  for m, poisoned in ((2, False), (3, True), (4, True)):
    w = g.mix_weights(masks, n, n, selection=sel, m=m)
    assert bool(torch.isnan(w[:n]).all()) == poisoned and not w[n:].any()
    assert mc.same_bits64(w.cpu().numpy(), g.mix_weights(masks.cpu(), n, n, selection=sel.cpu(), m=m).numpy())
  holed = masks.clone()
  holed[1] = 0
  for value, poisoned in ((0.0, False), (0.25, True)):
    wm = even.clone()
    wm[1] = value
    w = g.mix_weights(holed, n, n, weights=wm)
    assert bool(torch.isnan(w[:n]).all()) == poisoned
    assert mc.same_bits64(w.cpu().numpy(), g.mix_weights(holed.cpu(), n, n, weights=wm.cpu()).numpy())
  # NaN and inf entries of D: the same NaN pattern and bits as the host form
  sq = st["sq"].clone()
  sq[0, 3] = math.nan
  sq[2, 7] = math.inf
  got = g.mixed_sqdist(sq, n, masks, n)
  want = g.mixed_sqdist(sq.cpu(), n, masks.cpu(), n)
  assert mc.same_bits64(got.cpu().numpy(), want.numpy()) and torch.isnan(want).any() and torch.isfinite(want).any()


# ---------------------------------------------------------------------------- #
# 2. the mixed distances against float64 on the vectors;  3. the ranking

@pytest.mark.parametrize("n,f", SHAPES)
def test_mixed_distances_and_ranking_against_float64(bm, n, f):
  from tests.pair_mode_check import same_up_to_ties
  for kind in KINDS:
    for d in LENGTHS:
      st = _stage(kind, n, f, d)
      words, ref, bars = st["words"], st["ref"], st["bars"]
      got = st["mixed"].cpu().numpy()
      worst = 0.0
      for a in range(n):
        for b in range(n):
          if words[a] == words[b]:
            assert got[a, b] == 0.0 and not np.signbit(got[a, b]), (kind, n, d, a, b)     # exactly +0
          else:
            worst = max(worst, abs(got[a, b] - ref[a, b]) / bars[a, b])
      print(f"mixdist_error distances {kind} n={n} f={f} d={d} distinct_masks={len(set(words))} "
            f"worst error / bar {worst:.3e}")
      assert worst <= 1.0, (kind, n, f, d, worst)
      # 3. the ranking of the device's mixed distances against the float64 Krum order of the float64 mixed rows
      m = n - f - 2
      order, _ = bm.gars.rank_from_sqdist(st["mixed"], n, f, m, bm._lib.RANK_KRUM)
      scores64, order64 = mc.krum_scores64(ref, n, f)
      with np.errstate(divide="ignore", invalid="ignore"):
        delta = np.minimum(np.sqrt(bars), np.where(ref > 0, bars / np.sqrt(ref), np.inf))   # |sqrt(x + e) - sqrt(x)|
      np.fill_diagonal(delta, 0.0)
      tol = max(2.0 * delta[i].sum() / scores64[i] for i in range(n) if scores64[i] > 0)
      assert same_up_to_ties(order[:n].tolist(), order64, scores64, tol), (kind, n, f, d, tol)


# ---------------------------------------------------------------------------- #
# 4. the output, given the device's composed weights

def _exact_weighted_sum(points, weights):
  """cc.weighted_sum_exact with the mask of the coordinates whose emulated fma met a midpoint (those are left out)."""
  import collections
  from tests.first_pass_matrix import fma_emulated
  groups = collections.OrderedDict()
  for p, c in zip(points, weights):
    groups.setdefault(id(p), [p, 0.0])
    groups[id(p)][1] += float(c)
  acc = torch.zeros(points[0].shape[0], dtype=torch.float32)
  met = torch.zeros(points[0].shape[0], dtype=torch.bool)
  for p, c in groups.values():
    w = np.float32(c)
    if w == 0:
      continue
    acc, mid = fma_emulated(float(w), torch.from_numpy(p), 1.0, acc)
    met |= mid
  return acc.numpy(), met.numpy()


def _check_output(out, points_host, tag):
  """Item 4 for one result of form="scalars": bit for bit against the definition of bm_weighted_sum on the weights the
  device composed (where the emulation met no midpoint), and the float64 weighted sum at the bar of the centre tests."""
  w = out.mix_weights.cpu().numpy()
  got = out.cpu().numpy()
  want, met = _exact_weighted_sum(points_host, list(w[:len(points_host)]))
  # (composed weights are often short binary fractions — 3 of 24 is 1/8 — and then w x + acc IS an fp32 midpoint for a
  #  good share of the coordinates: those the emulation cannot vouch for, the others it decides)
  assert 2 * int(met.sum()) <= met.size, (tag, int(met.sum()))
  assert nc.same_bits(got[~met], want[~met]), tag
  clean = [p if np.isfinite(p).all() else np.zeros_like(p) for p in points_host]
  assert all(w[i] == 0 for i, p in enumerate(points_host) if not np.isfinite(p).all()), tag
  ref = cc.combine(w, clean)
  err = cc.relative_error(got.astype(np.float64), ref)
  print(f"mixdist_error output {tag} relative error {err:.3e} (bar {BAR:.3e})")
  assert err <= BAR, (tag, err)
  return err


@pytest.mark.parametrize("n,f", SHAPES)
def test_output_given_the_composed_weights(bm, n, f):
  d = 3074 if n <= 25 else 1027
  st = _stage("random", n, f, d)
  host, dev = st["host"], st["dev"]
  tau = 0.5 * math.sqrt(d)
  rules = [("krum", {}), ("geomed", {"iters": 8}), ("average", {}), ("cclip", {"tau": tau})]
  if n <= 25:
    rules.append(("brute", {}))
  for rule, args in rules:
    out = bm.gars.nnm(dev, f, rule=rule, form="scalars", **args)
    assert out.shape == (d,) and out.dtype == torch.float32
    assert _words(out.mix_masks, n) == st["words"]
    _check_output(out, host, f"{rule} n={n} f={f} d={d}")
    if rule in ("krum", "brute"):
      count = out.mix_selection[1]
      assert count == (n - f - 2 if rule == "krum" else n - f)
      sel = out.mix_selection[0][:count].tolist()
      want = mc.weights_reference(st["words"], n, sel=sel, m=count)
      assert mc.same_bits64(out.mix_weights.cpu().numpy(), want), rule
    if rule == "brute":
      assert int(out.brute_status.item()) == 0


# ---------------------------------------------------------------------------- #
# 5. end to end on crafted inputs: both forms and float64 select the same rows

def _mix_bound_norm(host, words):
  _, bounds = nc.mix_reference64(host, words)
  return float(np.linalg.norm(np.max(np.stack(bounds), axis=0)))


def _agree(bm, dev, host, words, rule, ref, tag, call):
  """The two forms against each other, within the sum of their bars: BAR |ref| for the weighted sum of the scalars
  form; BAR |ref| for the rule's kernel on the mixed rows plus the float32 mixing's own bound (nc.mix_reference64: an
  affine combination of the mixed rows moves by at most the largest of their bounds) for the rows form."""
  bm.gars.invalidate_rank_cache()
  rows_out = call("rows").cpu().numpy().astype(np.float64)
  scal_out = call("scalars").cpu().numpy().astype(np.float64)
  norm = float(np.linalg.norm(ref))
  err = cc.relative_error(scal_out, ref)
  gap = float(np.linalg.norm(scal_out - rows_out))
  bar = 2 * BAR * norm + _mix_bound_norm(host, words)
  print(f"mixdist_error forms {tag} {rule}: scalars vs float64 {err:.3e} (bar {BAR:.3e}), "
        f"|scalars - rows| / bar {gap / bar:.3e}")
  assert err <= BAR, (tag, rule, err)
  assert gap <= bar, (tag, rule, gap, bar)


@pytest.mark.parametrize("n,f", [(11, 2), (25, 5), (51, 12)])
def test_crafted_inputs_select_the_same_rows(bm, n, f):
  g = bm.gars
  d, m = 1027, n - f - 2
  host, words, order64, seed, gap, margin = mc.crafted_case(n, f, d)
  assert gap >= 1e-2 and margin >= 1e-2                 # conditions on the inputs, from float64 alone
  host = list(host)
  dev = _upload(host)
  tag = f"line n={n} f={f} seed={seed} gap={gap:.3g} margin={margin:.3g} distinct_masks={len(set(words))}"
  y64 = np.stack(mc.mixed_rows64(host, words))
  out = g.nnm(dev, f, rule="krum", form="scalars")
  assert _words(out.mix_masks, n) == words, tag
  sel_scalars = out.mix_selection[0][:m].tolist()
  g.invalidate_rank_cache()
  sel_rows = g.krum_selection(g.nnm_rows(dev, f), f)
  assert _same_selection(sel_scalars, order64[:m], words) and _same_selection(sel_rows, order64[:m], words), tag
  assert sorted(words[i] for i in sel_scalars) == sorted(words[i] for i in sel_rows)
  _check_output(out, host, tag)
  _agree(bm, dev, host, words, "krum", y64[order64[:m]].mean(axis=0), tag,
         lambda form: g.nnm(dev, f, rule="krum", form=form))
  nu, iters = 1e-6 * math.sqrt(d), 8
  ref, _ = cc.vector_iteration(y64, "geomed", nu, iters)
  _agree(bm, dev, host, words, "geomed", ref, tag, lambda form: g.nnm(dev, f, rule="geomed", form=form, nu=nu, iters=iters))
  tau = 0.25 * math.sqrt(d)
  ref, _ = cc.vector_iteration(y64, "cclip", tau, 3)
  _agree(bm, dev, host, words, "cclip", ref, tag, lambda form: g.nnm(dev, f, rule="cclip", form=form, tau=tau))
  _agree(bm, dev, host, words, "average", y64.mean(axis=0), tag, lambda form: g.nnm(dev, f, rule="average", form=form))


def _same_selection(got, want, words):
  """The same rows up to exchanging rows whose masks are equal (their mixed rows are one vector: exact ties in both
  forms, and either choice averages the same vectors)."""
  return sorted(words[i] for i in got) == sorted(words[i] for i in want)


@pytest.mark.parametrize("n,f,ratio", [(7, 1, 1.3), (11, 2, 1.3), (25, 5, 1.15)])
def test_separated_ladders(bm, n, f, ratio):
  """The ladders of tests/test_gpu_nnm.py: the neighbour sets are the float64 ones, and wherever the float64 order is
  decided at all (by a margin of 1e-2 or by equal masks) both forms select the float64 rows."""
  g = bm.gars
  d, m = 1027, n - f - 2
  host, sq64, seed, gap = nc.separated_case(n, f, d, ratio)
  _, margin, words, order64 = mc.selection_margin(host, n, f, m)
  dev = _upload(host)
  out = g.nnm(dev, f, rule="krum", form="scalars")
  assert _words(out.mix_masks, n) == words
  tag = f"ladder n={n} f={f} seed={seed} gap={gap:.3g} margin={margin:.3g} distinct_masks={len(set(words))}"
  _check_output(out, host, tag)
  if margin >= 1e-2:
    g.invalidate_rank_cache()
    assert _same_selection(out.mix_selection[0][:m].tolist(), order64[:m], words), tag
    assert _same_selection(g.krum_selection(g.nnm_rows(dev, f), f), order64[:m], words), tag
  y64 = np.stack(mc.mixed_rows64(host, words))
  _agree(bm, dev, host, words, "average", y64.mean(axis=0), tag, lambda form: g.nnm(dev, f, rule="average", form=form))


def test_cclip_with_a_start_at_63_rows(bm):
  g = bm.gars
  n, f, d = 63, 15, 1027
  host = nc.random_rows(n, d, seed=63)
  start = (np.mean(np.stack(host[:5]), axis=0) + np.float32(0.1)).astype(np.float32)
  dev, start_dev = _upload(host), torch.from_numpy(start).to(DEV)
  tau = 0.5 * math.sqrt(d)
  out = g.nnm(dev, f, rule="cclip", form="scalars", tau=tau, start=start_dev)
  words = _words(out.mix_masks, n + 1)
  assert words[n] == 1 << 63 and all(w >> n == 0 for w in words[:n])       # the start: alone in its mask, in no other
  # the masks are those of the rows alone (their sub-matrix of the pass over rows + start)
  sq = g.pairwise_sqdist(dev + [start_dev])
  assert words[:n] == _words(g.nnm_masks(sq[:n, :n].contiguous(), n, f), n)
  _check_output(out, host + [start], "cclip+start n=63")
  y64 = np.stack(mc.mixed_rows64(host, words[:n]))
  ref, _ = cc.vector_iteration(y64, "cclip", tau, 3, start=start)
  _agree(bm, dev, host, words[:n], "cclip+start", ref, "n=63 f=15",
         lambda form: g.nnm(dev, f, rule="cclip", form=form, tau=tau, start=start_dev))
  with pytest.raises(g.GarInputError):
    g.nnm(_upload(nc.random_rows(64, 64, seed=1)), 15, rule="cclip", form="scalars", tau=1.0, start=start_dev[:64].clone())


@pytest.mark.parametrize("n", [11, 25])
def test_bucketing_on_scalars(bm, n):
  g = bm.gars
  d, s = 1027, 2
  host = nc.random_rows(n, d, seed=5 * n)
  dev = _upload(host)
  perm = np.random.default_rng(n).permutation(n).tolist()
  words = g.bucket_masks(n, s, perm)
  assert len(words) == (n + 1) // 2 and bin(words[-1]).count("1") == 1           # odd n: an uneven last bucket
  y64 = np.stack(mc.mixed_rows64(host, words))
  tag = f"buckets n={n} s={s}"
  out = g.bucketing(dev, s, "average", perm=perm, form="scalars")
  _check_output(out, host, tag + " average")
  _agree(bm, dev, host, words, "average", y64.mean(axis=0), tag,
         lambda form: g.bucketing(dev, s, "average", perm=perm, form=form))
  nu = 1e-6 * math.sqrt(d)
  ref, _ = cc.vector_iteration(y64, "geomed", nu, 8)
  out = g.bucketing(dev, s, "geomed", perm=perm, form="scalars", nu=nu, iters=8)
  _check_output(out, host, tag + " geomed")
  _agree(bm, dev, host, words, "geomed", ref, tag,
         lambda form: g.bucketing(dev, s, "geomed", perm=perm, form=form, nu=nu, iters=8))
  # the rule's f travels in rule_args, and a rule that needs one says so
  k = len(words)
  out = g.bucketing(dev, s, "krum", perm=perm, form="scalars", f=1)
  assert out.mix_selection[1] == k - 3
  _check_output(out, host, tag + " krum")
  with pytest.raises(TypeError):
    g.bucketing(dev, s, "krum", perm=perm, form="scalars")
  with pytest.raises(ValueError):
    g.bucketing(dev, s, "trmean", perm=perm, form="scalars", f=1)


# ---------------------------------------------------------------------------- #
# 6. NaN attack copies

@pytest.mark.parametrize("n,f,f_real", [(11, 2, 1), (11, 2, 2), (25, 5, 3)])
def test_nan_copies_rank_last(bm, n, f, f_real):
  g = bm.gars
  d, m = 1027, n - f - 2
  honest = nc.random_rows(n - f_real, d, seed=n + f_real)
  byz = np.full(d, np.nan, dtype=np.float32)
  host = honest + [byz] * f_real
  dev = _upload(host)
  out = g.nnm(dev, f, rule="krum", form="scalars")
  words = _words(out.mix_masks, n)
  h = n - f_real
  assert all(w >> h == 0 for w in words[:h])                                 # the honest masks exclude the copies
  assert all((words[i] >> i) & 1 for i in range(h, n))
  order, scores = g.rank_from_sqdist(g.mixed_sqdist(g.pairwise_sqdist(dev), n, out.mix_masks, n), n, f, m, bm._lib.RANK_KRUM)
  assert sorted(order[h:n].tolist()) == list(range(h, n))                    # their own mixed rows rank last
  assert all(i < h for i in out.mix_selection[0][:m].tolist())
  assert torch.isfinite(out).all()
  _check_output(out, host, f"nan copies n={n} f={f} f_real={f_real}")


# ---------------------------------------------------------------------------- #
# 7. no synchronisation: capture and replay

def test_scalars_form_replays_in_a_graph(bm):
  n, f, d = 11, 2, 3074
  dev = _upload(nc.ladder_rows(n, d, 1.3, seed=1))
  graphed = bm.graphs.GraphedCall(lambda: bm.gars.nnm(dev, f, rule="krum", form="scalars"))
  for seed in (2, 3):
    fresh = nc.ladder_rows(n, d, 1.3, seed=seed)
    for t, h in zip(dev, fresh):
      t.copy_(torch.from_numpy(h))
    out = graphed().clone()
    eager = bm.gars.nnm(dev, f, rule="krum", form="scalars")
    assert torch.equal(out, eager), seed                                     # the replay followed the inputs
    assert _words(eager.mix_masks, n) == nc.masks_reference(nc.sqdist64(fresh), n, f)
