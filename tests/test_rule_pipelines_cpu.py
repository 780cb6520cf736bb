"""The launches the scalar-stage rules of gars make, without a GPU: geomed, cclip, caf, dnc and form="scalars" of nnm /
bucketing with the launching functions of the module replaced by recorders on CPU tensors.  Pins the sequence of every
public call and the arguments that carry meaning (the row counts of mix_weights, the start's flag, point count and mask
word, the block of the matrix the neighbour masks are made of)."""

import pytest
import torch

N, F, D = 11, 2, 8
DISTANCES = ["pairwise_sqdist"]
KRUM = ["pairwise_sqdist", "nnm_masks", "mixed_sqdist", "rank_from_sqdist", "mix_weights", "weighted_sum"]


def _swap(seq, old, new):
  return [new if name == old else name for name in seq]


def _without(seq, name):
  return [other for other in seq if other != name]


NNM_SEQUENCES = {
  "krum": KRUM,
  "brute": _swap(KRUM, "rank_from_sqdist", "brute_select_device"),
  "geomed": _swap(KRUM, "rank_from_sqdist", "center_weights"),
  "cclip": _swap(KRUM, "rank_from_sqdist", "center_weights"),
  "average": ["pairwise_sqdist", "nnm_masks", "mix_weights", "weighted_sum"],
}
BUCKETING_SEQUENCES = {rule: _without(seq, "nnm_masks") for rule, seq in NNM_SEQUENCES.items()}
BUCKETING_SEQUENCES["average"] = ["mix_weights", "weighted_sum"]  # no distance pass


@pytest.fixture(scope="module")
def gars():
  import byzantinemomentum_amd
  return byzantinemomentum_amd.gars


class _Recorder:
  """Stand-ins for the launching functions of gars: they append (name, args, kwargs) and answer with CPU tensors of the
  shapes the real ones give.  `_validate` is stubbed and not recorded."""

  def __init__(self, monkeypatch, gars):
    self.calls = []

    def record(name, result):
      def fn(*args, **kwargs):
        self.calls.append((name, args, kwargs))
        return result(*args, **kwargs)
      return fn

    def square(points, d_total=None):  # every entry its own number: a block of it is recognised
      count = len(points)
      return torch.arange(count * count, dtype=torch.float64).reshape(count, count)

    def never(name):
      return lambda *args, **kwargs: pytest.fail(f"{name} on a scalars path")

    vector = lambda points, weights: torch.zeros(D)  # noqa: E731
    answers = {
      "pairwise_sqdist": square,
      "nnm_masks": lambda sq, n, f: torch.ones(64, dtype=torch.int64),
      "mixed_sqdist": lambda sq, n_in, masks, n_out: torch.zeros(n_out, n_out, dtype=torch.float64),
      "rank_from_sqdist": lambda *a: (torch.zeros(64, dtype=torch.int32), torch.zeros(64, dtype=torch.float64)),
      "brute_select_device": lambda *a: (torch.zeros(64, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)),
      "center_weights": lambda *a, **k: (torch.zeros(64, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)),
      "spectral_weights": lambda *a, **k: (torch.zeros(64, dtype=torch.float64), torch.zeros(4, dtype=torch.float64)),
      "mix_weights": lambda *a, **k: torch.zeros(64, dtype=torch.float64),
      "weighted_sum": vector,
      "mix_rows": never("mix_rows"),
      "colwise_mixed": never("colwise_mixed"),
    }
    monkeypatch.setattr(gars, "_validate", lambda g: (len(g), D, torch.device("cpu")))
    for name, answer in answers.items():
      monkeypatch.setattr(gars, name, record(name, answer))

  def names(self):
    return [call[0] for call in self.calls]

  def one(self, name):
    found = [call for call in self.calls if call[0] == name]
    assert len(found) == 1, (name, self.names())
    return found[0][1], found[0][2]

  def clear(self):
    del self.calls[:]


def _rows(n=N):
  return [torch.zeros(D) for _ in range(n)]


def _bound(fn_args, names):
  """Positional and keyword arguments as one dictionary, the positional ones named in order."""
  args, kwargs = fn_args
  return dict(zip(names, args), **kwargs)


CENTER_ARGS = ("sq", "n", "mode", "param", "iters", "tol", "has_start")
MIX_ARGS = ("masks", "n_in", "n_out", "weights", "selection", "m")


def test_center_rules(gars, monkeypatch):
  spy = _Recorder(monkeypatch, gars)
  want = ["pairwise_sqdist", "center_weights", "weighted_sum"]
  gars.geomed(_rows(), f=F, nu=1e-3, iters=5)
  assert spy.names() == want
  got = _bound(spy.one("center_weights"), CENTER_ARGS)
  assert (got["n"], got["mode"], got["param"], got["iters"], got.get("tol", 0.0), bool(got.get("has_start"))) == \
         (N, "geomed", 1e-3, 5, 0.0, False)
  assert len(spy.one("pairwise_sqdist")[0][0]) == N and len(spy.one("weighted_sum")[0][0]) == N
  spy.clear()
  gars.cclip(_rows(), tau=2.0)
  assert spy.names() == want
  got = _bound(spy.one("center_weights"), CENTER_ARGS)
  assert (got["n"], got["mode"], got["param"], got["iters"], bool(got.get("has_start"))) == (N, "cclip", 2.0, 3, False)
  spy.clear()
  start = torch.ones(D)
  gars.cclip(_rows(), tau=2.0, start=start)
  assert spy.names() == want
  got = _bound(spy.one("center_weights"), CENTER_ARGS)
  assert (got["n"], got["has_start"]) == (N, True) and tuple(got["sq"].shape) == (N + 1, N + 1)
  points = spy.one("weighted_sum")[0][0]
  assert len(points) == N + 1 and points[N] is start and spy.one("pairwise_sqdist")[0][0][N] is start


def test_spectral_rules(gars, monkeypatch):
  spy = _Recorder(monkeypatch, gars)
  want = ["pairwise_sqdist", "spectral_weights", "weighted_sum"]
  out = gars.caf(_rows(), F, power_iters=9)
  assert spy.names() == want
  args, kwargs = spy.one("spectral_weights")
  assert tuple(args[1:]) + tuple(kwargs.values()) == (N, "caf", F, 9)
  assert out.spectral_weights.shape == (64,) and out.spectral_info.shape == (4,)
  spy.clear()
  gars.dnc(_rows(), F, c=1.5)
  assert spy.names() == want
  args, kwargs = spy.one("spectral_weights")
  assert tuple(args[1:]) + tuple(kwargs.values()) == (N, "dnc", 3, 16)  # k = ceil(1.5 * 2)


@pytest.mark.parametrize("rule", sorted(NNM_SEQUENCES))
def test_nnm_scalars(gars, monkeypatch, rule):
  spy = _Recorder(monkeypatch, gars)
  extra = {"tau": 2.0} if rule == "cclip" else {}
  out = gars.nnm(_rows(), F, rule=rule, form="scalars", **extra)
  assert spy.names() == NNM_SEQUENCES[rule]
  sq = spy.one("nnm_masks")[0][0]
  assert tuple(sq.shape) == (N, N) and tuple(spy.one("nnm_masks")[0][1:]) == (N, F)
  mix = _bound(spy.one("mix_weights"), MIX_ARGS)
  assert (mix["n_in"], mix["n_out"]) == (N, N)
  if rule == "krum":
    assert mix["m"] == N - F - 2 and mix["selection"].dtype == torch.int32 and mix.get("weights") is None
    assert tuple(spy.one("rank_from_sqdist")[0][1:4]) == (N, F, N - F - 2)
    assert out.mix_selection[1] == N - F - 2
  elif rule == "brute":
    assert mix["m"] == N - F and mix.get("weights") is None
    assert tuple(spy.one("brute_select_device")[0][1:]) == (N, F)
    assert out.mix_selection[1] == N - F and out.brute_status is gars.last_brute_status
  elif rule == "average":
    assert mix.get("selection") is None and mix["weights"][:N].tolist() == [1.0 / N] * N
    assert out.mix_selection is None
  else:
    assert mix.get("selection") is None and mix.get("m") is None and out.mix_selection is None
    got = _bound(spy.one("center_weights"), CENTER_ARGS)
    assert (got["n"], got["mode"], bool(got.get("has_start"))) == (N, rule, False)
  if rule != "average":
    sq_read, n_in, masks, n_out = spy.one("mixed_sqdist")[0]
    assert (n_in, n_out) == (N, N) and sq_read is sq and masks is out.mix_masks and mix["masks"] is masks
  assert len(spy.one("weighted_sum")[0][0]) == N and out.mix_weights is spy.one("weighted_sum")[0][1]


def test_nnm_scalars_cclip_start_at_63_rows(gars, monkeypatch):
  """The start is point n of the distance pass and mixed row n, alone in its mask: at n = 63 that word's only bit is the
  sign bit.  The neighbour masks are made of the leading n x n block."""
  n, f = 63, 15
  spy = _Recorder(monkeypatch, gars)
  start = torch.ones(D)
  out = gars.nnm(_rows(n), f, rule="cclip", form="scalars", tau=2.0, start=start)
  assert spy.names() == NNM_SEQUENCES["cclip"]
  points = spy.one("pairwise_sqdist")[0][0]
  assert len(points) == n + 1 and points[n] is start
  whole = torch.arange((n + 1) * (n + 1), dtype=torch.float64).reshape(n + 1, n + 1)
  block, n_arg, f_arg = spy.one("nnm_masks")[0]
  assert (n_arg, f_arg) == (n, f) and block.is_contiguous() and torch.equal(block, whole[:n, :n])
  sq, n_in, masks, n_out = spy.one("mixed_sqdist")[0]
  assert torch.equal(sq, whole) and (n_in, n_out) == (n + 1, n + 1)
  assert masks.dtype == torch.int64 and masks.tolist() == [1] * n + [-(1 << 63)]
  got = _bound(spy.one("center_weights"), CENTER_ARGS)
  assert (got["n"], got["mode"], got["param"], got["iters"], got["has_start"]) == (n, "cclip", 2.0, 3, True)
  mix = _bound(spy.one("mix_weights"), MIX_ARGS)
  assert (mix["n_in"], mix["n_out"]) == (n + 1, n + 1) and mix["masks"] is masks and mix.get("selection") is None
  summed = spy.one("weighted_sum")[0][0]
  assert len(summed) == n + 1 and summed[n] is start
  assert out.mix_masks is masks and out.mix_masks.numel() == n + 1  # the words mixed_sqdist read


@pytest.mark.parametrize("rule", sorted(BUCKETING_SEQUENCES))
def test_bucketing_scalars(gars, monkeypatch, rule):
  s, buckets, f = 2, 6, 1
  spy = _Recorder(monkeypatch, gars)
  extra = {"average": {}, "geomed": {}, "cclip": {"tau": 2.0}}.get(rule, {"f": f})
  out = gars.bucketing(_rows(), s, rule, perm=list(range(N)), form="scalars", **extra)
  assert spy.names() == BUCKETING_SEQUENCES[rule]
  words = [3 << (2 * b) for b in range(5)] + [1 << 10]
  mix = _bound(spy.one("mix_weights"), MIX_ARGS)
  assert (mix["n_in"], mix["n_out"]) == (N, buckets) and mix["masks"].tolist() == words
  assert out.mix_masks.tolist() == words
  if rule == "krum":
    assert mix["m"] == buckets - f - 2 and tuple(spy.one("rank_from_sqdist")[0][1:4]) == (buckets, f, buckets - f - 2)
  elif rule == "brute":
    assert mix["m"] == buckets - f and tuple(spy.one("brute_select_device")[0][1:]) == (buckets, f)
  elif rule == "average":
    assert mix["weights"][:buckets].tolist() == [1.0 / buckets] * buckets
  else:
    got = _bound(spy.one("center_weights"), CENTER_ARGS)
    assert (got["n"], got["mode"], bool(got.get("has_start"))) == (buckets, rule, False)
  if rule != "average":
    sq, n_in, masks, n_out = spy.one("mixed_sqdist")[0]
    assert (n_in, n_out) == (N, buckets) and tuple(sq.shape) == (N, N) and masks.tolist() == words
  assert len(spy.one("weighted_sum")[0][0]) == N
