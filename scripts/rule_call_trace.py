"""Which library calls the scalar-stage rules make, and what they compute: the check that a change of their host side
(gars.py, sharded.py and what these share) left both alone.  The companion of step_call_trace.py, whose recorders it uses.

    python scripts/rule_call_trace.py [--tree DIR] [--out FILE] [--show NAME] [--backend oracle]

Uses the public functions of gars and the public methods of ShardedAggregator only, so the same file runs against any
checkout of this project (--tree, default: the one this file is in).  The loaded library handle is wrapped: every bm_*
call appends its name and its integer / float arguments to a list.  Every configuration runs once on seeded inputs at
d = 4 099 and prints two SHA-256 digests: of the call list, and of the results — the output vector and every published
attribute (gars: mix_masks, mix_weights, mix_selection, brute_status, spectral_weights, spectral_info of the result and
gars.last_brute_status; the aggregator: last_masks, last_weights, last_selection, last_center_info, last_spectral_info,
brute_status; of a selection the entries that count).  A configuration that is refused is recorded with the exception's
type.  Two checkouts agree when their tables are equal line by line (`diff`); --show prints one configuration's calls.

Matrix: the front ends gars and a local_only ShardedAggregator (which has no bucketing) x (n, f) in (11, 2), (25, 5),
(64, 15) x
  geomed, cclip, caf, dnc, brute unchecked and check=True,
  nnm x every rule of NNM_RULES x both forms,
  bucketing at s = 2 x every rule x both forms, the rule's f the largest Bulyan admits on the bucket means,
and at (63, 15) cclip with a start vector: alone, under nnm and under bucketing, both forms.
Row i is a draw of independent normal coordinates scaled by 1 + i / 10: the Brute searches prune on that and end at once.

--backend oracle: the same matrix on CPU tensors with tests/sharded_backend.OracleBackend (of --tree), no GPU.  What is
recorded is every method call on the backend and on the aggregator, `_all_reduce` with its tensor's shape included.  That
backend declares no capabilities: these are the plain-torch legs.  gars has no CPU path: each of its configurations is
recorded as refused, with the type of the first refusal.  The aggregator's Brute configurations at n = 64 are left out
in this mode: OracleBackend.brute_select walks every one of the C(64, 15) subsets."""
import argparse
import os
import sys

from step_call_trace import TracedLibrary, described, digest, record_methods

D = 4099
SHAPES = ((11, 2), (25, 5), (64, 15))
START_SHAPE = (63, 15)
GARS_PUBLISHED = ("mix_masks", "mix_weights", "mix_selection", "brute_status", "spectral_weights", "spectral_info")
AGGREGATOR_PUBLISHED = ("last_masks", "last_weights", "last_selection", "last_center_info", "last_spectral_info",
                        "brute_status")
ORACLE_BRUTE_ROWS = 25  # the C(25, 5) = 53 130 subsets are walked, the C(64, 15) are not


def rule_args(rule, f=None):
  """What `rule` needs beyond the rows when it runs under nnm (f=None: nnm hands its own f on) or bucketing."""
  args = {"tau": 20.0} if rule == "cclip" else {}
  takes_f = rule not in ("median", "average", "geomed", "cclip")
  return dict(args, f=f) if takes_f and f is not None else args


def configurations(rules, brute_rows):
  """(name, front-end method, positional arguments after the rows, keyword arguments, wants a start, n); Brute only on
  up to `brute_rows` rows."""
  for n, f in SHAPES:
    tag = f"n{n}f{f}"
    yield f"{tag}-geomed", "geomed", (), {}, False, n
    yield f"{tag}-cclip", "cclip", (), {"tau": 20.0}, False, n
    yield f"{tag}-caf", "caf", (f,), {}, False, n
    yield f"{tag}-dnc", "dnc", (f,), {}, False, n
    if n <= brute_rows:
      yield f"{tag}-brute", "brute", (f,), {}, False, n
      yield f"{tag}-brute-check", "brute", (f,), {"check": True}, False, n
    buckets = -(-n // 2)
    for rule in rules:
      for form in ("rows", "scalars"):
        if rule != "brute" or n <= brute_rows:
          yield f"{tag}-nnm-{rule}-{form}", "nnm", (f,), dict(rule_args(rule), rule=rule, form=form), False, n
        if rule != "brute" or buckets <= brute_rows:
          yield (f"{tag}-bucketing-{rule}-{form}", "bucketing", (2, rule),
                 dict(rule_args(rule, (buckets - 3) // 4), seed=7, form=form), False, n)
  n, f = START_SHAPE
  tag = f"n{n}f{f}"
  yield f"{tag}-cclip-start", "cclip", (), {"tau": 20.0}, True, n
  for form in ("rows", "scalars"):
    yield f"{tag}-nnm-cclip-start-{form}", "nnm", (f,), {"rule": "cclip", "tau": 20.0, "form": form}, True, n
    yield f"{tag}-bucketing-cclip-start-{form}", "bucketing", (2, "cclip"), {"tau": 20.0, "seed": 7, "form": form}, True, n


def content(torch, value):
  """A published value as the results digest reads it."""
  if isinstance(value, torch.Tensor):
    return (tuple(value.shape), str(value.dtype), value.detach().cpu().numpy().tobytes())
  if isinstance(value, tuple) and len(value) == 2 and isinstance(value[0], torch.Tensor):  # (selection, count)
    return (str(value[0].dtype), int(value[1]), value[0][:int(value[1])].cpu().numpy().tobytes())
  return described(torch, value)


def run(torch, front, holder, method, args, kwargs, start, n, device):
  gen = torch.Generator().manual_seed(1234 + n)
  rows = [torch.randn(D, generator=gen).mul_(1.0 + 0.1 * i).to(device) for i in range(n)]
  if start:
    kwargs = dict(kwargs, start=torch.randn(D, generator=gen).to(device))
  out = getattr(holder, method)(rows, *args, **kwargs)
  if front == "gars":
    published = [(name, content(torch, getattr(out, name, None))) for name in GARS_PUBLISHED]
    published.append(("last_brute_status", content(torch, holder.last_brute_status)))
  else:
    published = [(name, content(torch, getattr(holder, name, None))) for name in AGGREGATOR_PUBLISHED]
  return content(torch, out), published


def main():
  parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
  parser.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  parser.add_argument("--out", help="write the table here as well")
  parser.add_argument("--show", help="print the calls of the configuration of this name and stop")
  parser.add_argument("--backend", choices=("hip", "oracle"), default="hip")
  args = parser.parse_args()
  sys.path.insert(0, os.path.abspath(args.tree))
  import torch
  from byzantinemomentum_amd import _lib, gars
  from byzantinemomentum_amd.sharded import ShardedAggregator
  oracle = args.backend == "oracle"
  log = []
  if oracle:
    torch.set_num_threads(1)
    from tests.sharded_backend import OracleBackend
    device = torch.device("cpu")

    def aggregator():
      backend = record_methods(torch, OracleBackend(), "backend", log)
      return record_methods(torch, ShardedAggregator(backend=backend, local_only=True), "aggregator", log)
  else:
    _lib._lib = TracedLibrary(_lib.load(), _lib.SIGNATURES, log)
    device = torch.device("cuda:0")

    def aggregator():
      return ShardedAggregator(local_only=True)
  lines, reached = [], set()
  for front in ("gars", "aggregator"):
    brute_rows = ORACLE_BRUTE_ROWS if oracle and front == "aggregator" else _lib.MAX_ROWS
    for name, method, positional, kwargs, start, n in configurations(tuple(gars.NNM_RULES), brute_rows):
      name = f"{front}-{name}"
      if (args.show and name != args.show) or (front == "aggregator" and method == "bucketing"):
        continue
      holder = gars if front == "gars" else aggregator()
      gars.last_brute_status = None
      del log[:]
      try:
        results = run(torch, front, holder, method, positional, kwargs, start, n, device)
      except Exception as err:  # noqa: BLE001  (a refusal is a result: its type is compared)
        try:
          if not oracle:
            torch.cuda.synchronize()  # a refusal of the arguments leaves the device alone; a device error does not
        except RuntimeError:
          print(f"{name}: device error, stopping: {err}", flush=True)
          return 1
        results = f"refused: {type(err).__name__}: {err}"
      calls = list(log)
      if args.show:
        print("\n".join(repr(c) for c in calls))
        print(results if isinstance(results, str) else digest(results))
        return 0
      reached.update(".".join(c[:2]) if oracle else c[0] for c in calls)
      lines.append(f"{name} calls={digest(calls)} n_calls={len(calls)} results={digest(results)}"
                   + (f" REFUSED {results.split(': ')[1]}" if isinstance(results, str) else ""))
      print(lines[-1], flush=True)
  lines.append(f"# {len(lines)} configurations, {len(reached)} entry points reached: {' '.join(sorted(reached))}")
  print(lines[-1], flush=True)
  if args.out:
    with open(args.out, "w") as out:
      out.write("\n".join(lines) + "\n")
  return 0


if __name__ == "__main__":
  sys.exit(main())
