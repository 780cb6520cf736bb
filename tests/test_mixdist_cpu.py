"""Distance-based rules on mixed rows from scalars, without a GPU: the host forms of bm_mixed_sqdist and bm_mix_weights
bit for bit against loops over Python floats, the properties the exact-tie handling relies on, the float64 distances of
float64 mixed rows, every refused argument, the arguments of gars.nnm / gars.bucketing, and
ShardedAggregator.nnm(form="scalars") on one rank and on the gloo world of two (one all-reduce)."""

import ctypes
import math
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import mixdist_cases as mc
from tests import nnm_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("bm_mixed_sqdist", "bm_mixed_sqdist_device", "bm_mix_weights", "bm_mix_weights_device")


@pytest.fixture(scope="module")
def bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


@pytest.fixture(scope="module")
def lib(bm):
  return bm._lib.load()


def _matrix(n, seed, scale=1.0):
  """A symmetric float64 matrix of positive entries with an arbitrary diagonal (never read)."""
  rng = np.random.default_rng(seed)
  a = rng.uniform(0.5, 2.0, size=(n, n)) * scale
  a = (a + a.T) / 2
  np.fill_diagonal(a, rng.uniform(-3.0, 3.0, size=n))
  return a


# ---------------------------------------------------------------------------- #
# 1. bm_mixed_sqdist against the float loop

@pytest.mark.parametrize("n", mc.ROW_COUNTS)
def test_host_form_is_the_float_loop(lib, n):
  sq = _matrix(n, seed=n, scale=1e3 if n == 25 else 1.0)
  for name, words in mc.mask_sets(n):
    code, got = mc.host_mixed(lib, sq, n, list(words))
    assert code == 0, (n, name)
    want, _ = mc.mixed_reference(sq, n, list(words))
    assert mc.same_bits64(got, want), (n, name)
    assert not np.signbit(got[~np.isnan(got)]).any()


def test_upper_triangle_only(lib):
  """D_ij is read at (min, max): the lower triangle and the diagonal may hold anything."""
  n = 11
  sq = _matrix(n, seed=4)
  words = list(mc.mask_sets(n)[1][1])
  _, want = mc.host_mixed(lib, sq, n, words)
  junk = sq.copy()
  junk[np.tril_indices(n)] = np.nan
  _, got = mc.host_mixed(lib, junk, n, words)
  assert mc.same_bits64(got, want)


# ---------------------------------------------------------------------------- #
# 2. Properties

@pytest.mark.parametrize("n", [7, 25, 64])
def test_properties(lib, n):
  sq = _matrix(n, seed=100 + n)
  words = list(nc.masks_reference(sq, n, max(1, n // 5)))
  words[3] = words[1]                                  # equal masks
  words.append(words[0])
  n_out = len(words)
  if n_out > mc.MAX_ROWS:
    words = words[:mc.MAX_ROWS - 1] + [words[0]]
    n_out = mc.MAX_ROWS
  code, out = mc.host_mixed(lib, sq, n, words)
  assert code == 0
  bits = out.view(np.uint64)
  assert np.array_equal(bits, bits.T)                                           # bitwise symmetry
  assert not bits.diagonal().any()                                              # +0 on the diagonal
  assert bits[1, 3] == 0 and bits[0, n_out - 1] == 0                            # +0 for equal masks
  assert np.array_equal(bits[1], bits[3]) and np.array_equal(bits[0], bits[n_out - 1])   # equal masks: equal rows
  assert (out >= 0).all() and not np.signbit(out).any()                         # nothing negative, no -0
  # the diagonal of D and every entry outside all masks set to NaN: the same bits
  inside = np.array([[(w >> j) & 1 for j in range(n)] for w in words], dtype=bool)
  used = np.zeros((n, n), dtype=bool)
  for a in range(n_out):
    for b in range(n_out):
      if words[a] != words[b]:
        used |= np.outer(inside[a], inside[b]) | np.outer(inside[a], inside[a])
  used = np.triu(used | used.T, 1)
  holed = np.where(used, sq, np.nan)
  _, got = mc.host_mixed(lib, holed, n, words)
  assert mc.same_bits64(got, out) and not np.isnan(got).any()


def test_empty_mask_gives_nan(lib):
  n = 7
  sq = _matrix(n, seed=7)
  words = [0b0000111, 0, 0b1110000, 0b0000111]
  _, out = mc.host_mixed(lib, sq, n, words)
  assert np.isnan(out[1]).all() and np.isnan(out[:, 1]).all()
  rest = np.delete(np.delete(out, 1, axis=0), 1, axis=1)
  assert np.isfinite(rest).all() and rest[0, 2] == 0.0
  want, _ = mc.mixed_reference(sq, n, words)
  assert mc.same_bits64(out, want)


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
def test_non_finite_entry_reaches_exactly_the_pairs_that_read_it(lib, bad):
  n = 9
  sq = _matrix(n, seed=9)
  sq[2, 5] = bad                                       # the entry the masks read ((5, 2) is never read)
  words = [0b000000111, 0b000100101, 0b000100100, 0b111000000, 0b000100101, 0b110000010, 0b000011011]
  _, out = mc.host_mixed(lib, sq, n, words)
  want, _ = mc.mixed_reference(sq, n, words)
  assert mc.same_bits64(out, want)
  for a in range(len(words)):
    for b in range(len(words)):
      reads = False
      if a != b and words[a] != words[b]:
        for wa, wb in ((words[a], words[b]), (words[b], words[a]), (words[a], words[a]), (words[b], words[b])):
          reads = reads or ((wa >> 2) & 1 and (wb >> 5) & 1)
      assert bool(np.isnan(out[a, b])) == bool(reads), (a, b)
  assert out[1, 4] == 0.0                              # equal masks read nothing, even with the bad entry inside


def test_aliased_rows_keep_their_ties(lib):
  """f aliased Byzantine rows: bitwise-equal rows of D, exact zeros between the copies, ties everywhere.  The masks come
  out in a few classes; rows of one class get bitwise-equal rows of the output, whatever their indices."""
  n, f = 11, 3
  rows = nc.random_rows(n - f + 1, 64, seed=5)
  stack = rows[:n - f] + [rows[n - f]] * f
  sq = nc.sqdist64(stack)
  words = nc.masks_reference(sq, n, f)
  _, out = mc.host_mixed(lib, sq, n, words)
  want, _ = mc.mixed_reference(sq, n, words)
  assert mc.same_bits64(out, want)
  for a in range(n):
    for b in range(n):
      if words[a] == words[b]:
        assert np.array_equal(out[a].view(np.uint64), out[b].view(np.uint64))


# ---------------------------------------------------------------------------- #
# 3. Against the vectors

@pytest.mark.parametrize("n,f", [(7, 1), (11, 2), (25, 5), (51, 12), (64, 15)])
def test_against_float64_mixed_rows(lib, n, f):
  d = 1027
  for kind in ("random", "ladder", "buckets"):
    rows = nc.ladder_rows(n, d, 1.15, seed=n) if kind == "ladder" else nc.random_rows(n, d, seed=n)
    sq = nc.sqdist64(rows)
    words = mc.bucket_words(n, 3, seed=n) if kind == "buckets" else nc.masks_reference(sq, n, f)
    code, out = mc.host_mixed(lib, sq, n, words)
    assert code == 0
    _, terms = mc.mixed_reference(sq, n, words)
    ref = nc.sqdist64([y.astype(np.float64) for y in mc.mixed_rows64(rows, words)])
    worst = 0.0
    for a in range(len(words)):
      for b in range(len(words)):
        if terms[a][b] is None:
          assert out[a, b] == 0.0
          continue
        bar = mc.SUM_BAR * sum(terms[a][b]) + d * mc.EPS64 * ref[a, b]
        worst = max(worst, abs(out[a, b] - ref[a, b]) / bar)
    print(f"mixdist host n={n} f={f} {kind}: worst error / bar {worst:.3g}")
    assert worst <= 1.0, (n, f, kind, worst)


# ---------------------------------------------------------------------------- #
# 4. bm_mix_weights

@pytest.mark.parametrize("n", mc.ROW_COUNTS)
def test_weights_are_the_float_loop(lib, n):
  rng = np.random.default_rng(n)
  for name, words in mc.mask_sets(n):
    words = list(words)
    n_out = len(words)
    w = [float(v) for v in rng.normal(size=n_out)]
    if n_out > 2:
      w[1] = 0.0
    code, got = mc.host_weights(lib, words, n, w=w)
    assert code == 0
    want = mc.weights_reference(words, n, w=w)
    assert mc.same_bits64(got, want), (n, name)
    assert not got[n:].any()
    m = min(mc.MAX_ROWS, n_out + 2)
    sel = [int(t) for t in rng.integers(0, n_out, size=m)]     # duplicates
    code, got = mc.host_weights(lib, words, n, sel=sel, m=m)
    assert code == 0
    assert mc.same_bits64(got, mc.weights_reference(words, n, sel=sel, m=m)), (n, name)
    # the weights of the original rows add up to the weights of the mixed rows
    for given in (dict(w=[abs(v) for v in w]), dict(sel=sel, m=m)):
      _, got = mc.host_weights(lib, words, n, **given)
      total = math.fsum(given["w"]) if "w" in given else 1.0
      assert abs(float(got.sum()) - total) <= 64 * 2.0 ** -52 * total, (n, name)


def test_weights_poison_and_skip(lib):
  n = 7
  words = [0b0000111, 0, 0b1110000]
  # a zero weight on the empty mask is skipped; a weight that counts there poisons (the mixed row is NaN)
  _, got = mc.host_weights(lib, words, n, w=[0.5, 0.0, 0.5])
  assert mc.same_bits64(got, mc.weights_reference(words, n, w=[0.5, 0.0, 0.5])) and np.isfinite(got).all()
  assert got[:3].tolist() == [0.5 / 3] * 3 and got[3] == 0 and got[4:7].tolist() == [0.5 / 3] * 3
  _, got = mc.host_weights(lib, words, n, w=[0.5, 0.25, 0.25])
  assert np.isnan(got[:n]).all() and not got[n:].any()
  # a NaN weight reaches the members of its mask (bm_weighted_sum then answers NaN everywhere)
  _, got = mc.host_weights(lib, words, n, w=[math.nan, 0.0, 1.0])
  assert np.isnan(got[:3]).all() and np.isfinite(got[3:]).all()
  # a negative index (a Brute search that gave up) or one beyond n_out: NaN for every original row, zeros beyond
  for sel in ([0, -1], [0, 3], [2, 2, -7]):
    code, got = mc.host_weights(lib, words, n, sel=sel, m=len(sel))
    assert code == 0 and np.isnan(got[:n]).all() and not got[n:].any()
    assert mc.same_bits64(got, mc.weights_reference(words, n, sel=sel, m=len(sel)))
  # a selection that names the empty mask
  _, got = mc.host_weights(lib, words, n, sel=[0, 1], m=2)
  assert np.isnan(got[:n]).all()
  # only the first m entries count
  _, got = mc.host_weights(lib, words, n, sel=[0, 2, -1], m=2)
  assert np.isfinite(got).all() and abs(got.sum() - 1.0) < 1e-15


# ---------------------------------------------------------------------------- #
# 5. Refusals

def test_refused_arguments(bm, lib):
  E = bm._lib.EINVAL
  sq = (ctypes.c_double * (64 * 64))()
  masks = (ctypes.c_uint64 * 64)(*([1] * 64))
  out = (ctypes.c_double * (64 * 64))()
  w = (ctypes.c_double * 64)()
  sel = (ctypes.c_int32 * 64)()
  for n_in, n_out in ((0, 1), (65, 1), (-1, 1), (1, 0), (1, 65), (11, -2)):
    assert lib.bm_mixed_sqdist(sq, n_in, masks, n_out, out) == E, (n_in, n_out)
    assert lib.bm_mixed_sqdist_device(sq, n_in, masks, n_out, out, None) == E, (n_in, n_out)   # before any HIP call
    assert lib.bm_mix_weights(masks, n_in, n_out, w, None, 0, out) == E, (n_in, n_out)
    assert lib.bm_mix_weights_device(masks, n_in, n_out, w, None, 0, out, None) == E, (n_in, n_out)
  for args in ((None, 11, masks, 11, out), (sq, 11, None, 11, out), (sq, 11, masks, 11, None)):
    assert lib.bm_mixed_sqdist(*args) == E
    assert lib.bm_mixed_sqdist_device(*args, None) == E
  for args in ((None, 11, 11, w, None, 0, out), (masks, 11, 11, w, None, 0, None),
               (masks, 11, 11, None, None, 0, out),      # neither weights nor selection
               (masks, 11, 11, w, sel, 3, out),          # both
               (masks, 11, 11, None, sel, 0, out), (masks, 11, 11, None, sel, 65, out), (masks, 11, 11, None, sel, -1, out)):
    assert lib.bm_mix_weights(*args) == E
    assert lib.bm_mix_weights_device(*args, None) == E
  # a mask bit at or above n_in: the host forms refuse
  masks[4] = 1 << 11
  assert lib.bm_mixed_sqdist(sq, 11, masks, 11, out) == E
  assert lib.bm_mix_weights(masks, 11, 11, w, None, 0, out) == E
  assert lib.bm_mixed_sqdist(sq, 11, masks, 4, out) == 0           # beyond n_out: not read
  assert lib.bm_mixed_sqdist(sq, 12, masks, 11, out) == 0
  masks[4] = 1 << 63
  assert lib.bm_mixed_sqdist(sq, 63, masks, 11, out) == E
  assert lib.bm_mixed_sqdist(sq, 64, masks, 11, out) == 0
  assert lib.bm_mix_weights(masks, 64, 11, w, None, 0, out) == 0
  assert lib.bm_mix_weights(masks, 64, 11, None, sel, 64, out) == 0


def test_python_wrappers_refuse(bm):
  g = bm.gars
  sq = torch.zeros(11, 11, dtype=torch.float64)
  masks = torch.ones(64, dtype=torch.int64)
  for n_in, n_out in ((0, 1), (65, 1), (1, 0), (1, 65)):
    with pytest.raises(g.GarInputError):
      g.mixed_sqdist(sq, n_in, masks, n_out)
    with pytest.raises(g.GarInputError):
      g.mix_weights(masks, n_in, n_out, weights=torch.zeros(64, dtype=torch.float64))
  with pytest.raises(g.GarInputError):
    g.mixed_sqdist(sq.float(), 11, masks, 11)
  with pytest.raises(g.GarInputError):
    g.mixed_sqdist(sq, 12, masks, 11)                              # the matrix is too small
  with pytest.raises(g.GarInputError):
    g.mixed_sqdist(sq, 11, masks.int(), 11)
  with pytest.raises(g.GarInputError):
    g.mixed_sqdist(sq, 11, masks[:5], 11)
  with pytest.raises(RuntimeError):
    g.mixed_sqdist(sq, 11, [1 << 11], 1)                           # BM_EINVAL of the host form
  with pytest.raises(ValueError):
    g.mix_weights(masks, 11, 11)
  with pytest.raises(ValueError):
    g.mix_weights(masks, 11, 11, weights=torch.zeros(64, dtype=torch.float64), selection=torch.zeros(64, dtype=torch.int32), m=3)
  with pytest.raises(ValueError):
    g.mix_weights(masks, 11, 11, selection=torch.zeros(64, dtype=torch.int32))      # no m
  with pytest.raises(g.GarInputError):
    g.mix_weights(masks, 11, 11, selection=torch.zeros(64, dtype=torch.int64), m=3)
  with pytest.raises(g.GarInputError):
    g.mix_weights(masks, 11, 11, weights=torch.zeros(5, dtype=torch.float64))
  with pytest.raises(g.GarInputError):
    g.mix_weights(masks, 11, 11, selection=torch.zeros(64, dtype=torch.int32), m=65)
  # and what they return on the host
  out = g.mixed_sqdist(sq, 11, [0b11, 0b110, 0b11], 3)
  assert out.shape == (3, 3) and out.dtype == torch.float64 and not out.any()
  w = g.mix_weights([0b11, 0b110], 11, 2, selection=torch.tensor([1, 0], dtype=torch.int32), m=2)
  assert w.shape == (64,) and w[:3].tolist() == [0.25, 0.5, 0.25] and not w[3:].any()


def test_header_declares_and_library_exports_the_four(bm, lib):
  text = open(os.path.join(ROOT, "include", "bm_gar.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  declared = set(re.findall(r"\b(bm_[a-z0-9_]+)\s*\(", text))
  for name in NEW_NAMES:
    assert name in declared and name in bm._lib.SIGNATURES and hasattr(lib, name), name
  assert bm._lib.ABI_VERSION == 23 and lib.bm_abi_version() == 23


# ---------------------------------------------------------------------------- #
# 6. gars.nnm / gars.bucketing: the arguments

def test_scalars_form_serves_five_rules(bm):
  g = bm.gars
  cpu = [torch.zeros(4) for _ in range(5)]
  assert g.SCALAR_RULES == ("krum", "brute", "geomed", "cclip", "average")
  for rule in g.NNM_RULES:
    if rule in g.SCALAR_RULES:
      continue
    for call in (lambda: g.nnm(cpu, 1, rule=rule, form="scalars"), lambda: g.bucketing(cpu, 2, rule, form="scalars")):
      with pytest.raises(ValueError) as err:
        call()
      assert not isinstance(err.value, g.GarInputError) and all(name in str(err.value) for name in g.SCALAR_RULES)
  with pytest.raises(ValueError):
    g.nnm(cpu, 1, rule="krum", form="columns")
  for rule in g.SCALAR_RULES:                           # accepted: the next complaint is about the CPU tensors
    with pytest.raises(g.GarInputError):
      g.nnm(cpu, 1, rule=rule, form="scalars")


class _Spy:
  """Stand-ins for the module functions of gars that record (name, what identifies the call)."""

  def __init__(self, monkeypatch, gars, n, d):
    self.calls = []
    rows = [torch.zeros(d) for _ in range(n)]

    def record(name, result):
      def fn(*args, **kwargs):
        self.calls.append((name, tuple(a if isinstance(a, (int, str, float)) else type(a).__name__ for a in args),
                           tuple(sorted(kwargs))))
        return result(*args, **kwargs) if callable(result) else result
      return fn

    monkeypatch.setattr(gars, "_validate", record("_validate", lambda g: (len(g), d, torch.device("cpu"))))
    monkeypatch.setattr(gars, "pairwise_sqdist", record("pairwise_sqdist", torch.zeros(n, n, dtype=torch.float64)))
    monkeypatch.setattr(gars, "nnm_masks", record("nnm_masks", torch.ones(64, dtype=torch.int64)))
    monkeypatch.setattr(gars, "mix_rows", record("mix_rows", lambda g, m, n_out: rows[:n_out]))
    monkeypatch.setattr(gars, "colwise_mixed", record("colwise_mixed", torch.zeros(d)))
    for rule in gars.NNM_RULES:
      monkeypatch.setattr(gars, rule, record(rule, torch.zeros(d)))
    for name in ("mixed_sqdist", "mix_weights", "rank_from_sqdist", "center_weights", "weighted_sum",
                 "brute_select_device"):
      monkeypatch.setattr(gars, name, record(name, lambda *a, _name=name, **k: pytest.fail(f"{_name} on the rows path")))


@pytest.mark.parametrize("rule", ["krum", "geomed", "average", "brute", "cclip", "bulyan", "phocas"])
def test_rows_form_makes_the_calls_it_made(bm, monkeypatch, rule):
  g = bm.gars
  n, f, d = 11, 2, 8
  grads = [torch.zeros(d) for _ in range(n)]
  extra = {"tau": 1.0} if rule == "cclip" else {}
  spy = _Spy(monkeypatch, g, n, d)
  g.nnm(grads, f, rule=rule, **extra)
  default = list(spy.calls)
  del spy.calls[:]
  g.nnm(grads, f, rule=rule, form="rows", **extra)
  assert spy.calls == default
  names = [c[0] for c in default]
  assert names == ["_validate", "pairwise_sqdist", "nnm_masks", "mix_rows", rule]     # today's path, nothing else
  del spy.calls[:]
  kwargs = dict(extra, f=f) if g.NNM_RULES[rule] else extra
  g.bucketing(grads, 2, rule, perm=list(range(n)), **kwargs)
  default = list(spy.calls)
  del spy.calls[:]
  g.bucketing(grads, 2, rule, perm=list(range(n)), form="rows", **kwargs)
  assert spy.calls == default and [c[0] for c in default] == ["_validate", "mix_rows", rule]


# ---------------------------------------------------------------------------- #
# 7. ShardedAggregator.nnm(form="scalars") with the tests' oracle backend

N, F, D = 11, 2, 1000
RULES = (("krum", {}), ("brute", {}), ("geomed", {"iters": 4}), ("cclip", {"tau": 20.0}), ("average", {}),
         ("cclip", {"tau": 20.0, "start": True}))


def _pipeline64(rows, f, rule, args):
  """Distances, neighbours, mixing and the rule in float64 on the vectors."""
  from tests import center_cases as cc
  n = len(rows)
  words = nc.masks_reference(nc.sqdist64(rows), n, f)
  y = np.stack(mc.mixed_rows64(rows, words))
  if rule == "average":
    return y.mean(axis=0)
  if rule == "krum":
    _, order = mc.krum_scores64(nc.sqdist64(list(y)), n, f)
    return y[order[:n - f - 2]].mean(axis=0)
  if rule == "brute":
    import itertools
    sq = nc.sqdist64(list(y))
    best = min(itertools.combinations(range(n), n - f), key=lambda s: max(sq[a, b] for a in s for b in s))
    return y[list(best)].mean(axis=0)
  start = _start(rows) if args.get("start") else None
  v, _ = cc.vector_iteration(y, rule, args.get("tau", 1e-6), args.get("iters", 3), start=start)
  return v


def _start(rows):
  return (np.mean(np.stack(rows[:3]), axis=0) + 0.25).astype(np.float32)


def _close(got, want):
  return np.abs(got.astype(np.float64) - want).max() <= 64 * nc.U * max(1.0, np.abs(want).max())


def _count_reduces(agg):
  calls = []
  inner = agg._all_reduce

  def counted(tensor, op=None):
    calls.append(tuple(tensor.shape))
    return inner(tensor, op)
  agg._all_reduce = counted
  return calls


def _run_rules(agg, local, slice_of):
  res = {}
  for rule, args in RULES:
    kwargs = dict(args)
    if kwargs.get("start"):
      kwargs["start"] = slice_of(_start(nc.ladder_rows(N, D, 1.3, seed=1)))
    calls = _count_reduces(agg)
    out = agg.nnm(local, F, rule=rule, form="scalars", d_total=D, **kwargs)
    del agg._all_reduce
    key = rule + ("+start" if args.get("start") else "")
    res[key] = dict(out=out, reduces=list(calls), masks=agg.last_masks.clone(), weights=agg.last_weights.clone(),
                    selection=None if rule not in ("krum", "brute") else agg.last_selection[0][:agg.last_selection[1]].tolist())
  return res


def test_sharded_scalars_on_one_rank():
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from tests.sharded_backend import OracleBackend
  rows = nc.ladder_rows(N, D, 1.3, seed=1)
  local = [torch.from_numpy(r) for r in rows]
  agg = ShardedAggregator(backend=OracleBackend(), local_only=True)
  res = _run_rules(agg, local, torch.from_numpy)
  words = nc.masks_reference(nc.sqdist64(rows), N, F)
  for (rule, args), key in zip(RULES, res):
    r = res[key]
    assert r["out"].dtype == torch.float32 and _close(r["out"].numpy(), _pipeline64(rows, F, rule, args)), key
    assert nc.from_int64(r["masks"].tolist())[:N] == words
    total = float(r["weights"].sum())
    assert abs(total - 1.0) <= 1e-12, (key, total)
    # the rows form of the same aggregator computes the same thing, up to the float32 mixing it does and this does not
    other = agg.nnm(local, F, rule=rule, d_total=D, **{k: (torch.from_numpy(_start(rows)) if k == "start" else v)
                                                       for k, v in args.items()})
    assert _close(r["out"].numpy(), other.double().numpy()), key
  assert res["krum"]["selection"] is not None and len(res["krum"]["selection"]) == N - F - 2
  assert sorted(res["brute"]["selection"]) == res["brute"]["selection"] and len(res["brute"]["selection"]) == N - F
  with pytest.raises(ValueError) as err:
    agg.nnm(local, F, rule="trmean", form="scalars")
  assert all(name in str(err.value) for name in ("krum", "brute", "geomed", "cclip", "average"))
  with pytest.raises(ValueError):
    agg.nnm(local, F, rule="krum", form="columns")
  with pytest.raises(ValueError):
    agg.nnm(local, F, rule="cclip", form="scalars")          # tau is required: the rule's own error


def test_torch_legs_give_the_host_forms_bits(bm):
  from byzantinemomentum_amd.torch_legs import _mix_weights_torch, _mixed_sqdist_torch
  for n in (1, 7, 25, 64):
    sq = torch.from_numpy(np.ascontiguousarray(_matrix(n, seed=n)))
    for name, words in mc.mask_sets(n):
      masks = torch.tensor(nc.to_int64(list(words)), dtype=torch.int64)
      n_out = len(words)
      want = bm.gars.mixed_sqdist(sq, n, masks, n_out)
      assert mc.same_bits64(_mixed_sqdist_torch(sq, n, masks, n_out).numpy(), want.numpy()), (n, name)
      w = torch.from_numpy(np.random.default_rng(n).normal(size=64))
      assert mc.same_bits64(_mix_weights_torch(masks, n, n_out, weights=w).numpy(),
                            bm.gars.mix_weights(masks, n, n_out, weights=w).numpy()), (n, name)
      m = min(64, n_out + 1)
      sel = torch.from_numpy(np.random.default_rng(n).integers(0, n_out, size=64).astype(np.int32))
      assert mc.same_bits64(_mix_weights_torch(masks, n, n_out, selection=sel, m=m).numpy(),
                            bm.gars.mix_weights(masks, n, n_out, selection=sel, m=m).numpy()), (n, name)
  # what the host forms refuse, the legs refuse; what they poison, the legs poison
  with pytest.raises(ValueError):
    _mixed_sqdist_torch(torch.zeros(3, 3, dtype=torch.float64), 3, torch.tensor([8]), 1)
  bad = torch.tensor([0, -1], dtype=torch.int32)
  masks = torch.tensor([3, 6])
  assert mc.same_bits64(_mix_weights_torch(masks, 3, 2, selection=bad, m=2).numpy(),
                        bm.gars.mix_weights(masks, 3, 2, selection=bad, m=2).numpy())
  empty = torch.tensor([3, 0, 6])
  sq = torch.from_numpy(np.ascontiguousarray(_matrix(3, seed=3)))
  assert mc.same_bits64(_mixed_sqdist_torch(sq, 3, empty, 3).numpy(), bm.gars.mixed_sqdist(sq, 3, empty, 3).numpy())


def _free_port():
  with socket.socket() as s:
    s.bind(("127.0.0.1", 0))
    return s.getsockname()[1]


def _worker(rank, world, port, queue):
  os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
  dist.init_process_group("gloo", rank=rank, world_size=world)
  try:
    from byzantinemomentum_amd.sharded import ShardedAggregator, shard_bounds
    from tests.sharded_backend import OracleBackend
    rows = nc.ladder_rows(N, D, 1.3, seed=1)
    lo, hi = shard_bounds(D, world, rank)
    local = [torch.from_numpy(r[lo:hi].copy()) for r in rows]
    agg = ShardedAggregator(backend=OracleBackend())
    res = _run_rules(agg, local, lambda v: torch.from_numpy(v[lo:hi].copy()))
    for r in res.values():
      r["out"] = agg.all_gather_output(r["out"], D).numpy().copy()
      r["masks"], r["weights"] = r["masks"].numpy().copy(), r["weights"].numpy().copy()
    queue.put((rank, res))
    dist.barrier()
  finally:
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sharded_scalars_on_the_gloo_world_of_two():
  from byzantinemomentum_amd.sharded import ShardedAggregator
  from tests.sharded_backend import OracleBackend
  world = 2
  ctx = mp.get_context("spawn")
  queue = ctx.Queue()
  port = _free_port()
  procs = [ctx.Process(target=_worker, args=(r, world, port, queue)) for r in range(world)]
  for p in procs:
    p.start()
  results = dict(queue.get(timeout=240) for _ in range(world))
  for p in procs:
    p.join(timeout=60)
    assert p.exitcode == 0
  rows = nc.ladder_rows(N, D, 1.3, seed=1)
  one = _run_rules(ShardedAggregator(backend=OracleBackend(), local_only=True), [torch.from_numpy(r) for r in rows],
                   torch.from_numpy)
  for key, single in one.items():
    points = N + (1 if key.endswith("+start") else 0)
    assert single["reduces"] == [(points, points)]                     # (a no-op with one rank, entered once as well)
    for r in range(world):
      got = results[r][key]
      assert got["reduces"] == [(points, points)], (key, r, got["reduces"])        # exactly ONE all-reduce: D
      assert np.array_equal(got["masks"], single["masks"].numpy()), (key, r)
      assert got["selection"] == single["selection"], (key, r)
      # the all-reduced matrix is the sum of two partial sums: the weights move by its rounding, the output with them
      assert np.abs(got["weights"] - single["weights"].numpy()).max() <= 1e-9, (key, r)
      assert _close(got["out"], single["out"].double().numpy()), (key, r)
    assert np.array_equal(results[0][key]["weights"], results[1][key]["weights"]), key   # every rank: the same bits
    assert np.array_equal(results[0][key]["out"], results[1][key]["out"]), key
