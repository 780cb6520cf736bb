"""Which library calls a step makes, and what it computes: the check that a change of the host mirror (step.py,
stats.py, the host code of bm_step_worker) left both alone.

    python scripts/step_call_trace.py [--tree DIR] [--out FILE] [--show NAME] [--backend oracle]

Uses the public constructor of AggregationStep and `_lib` only, so the same file runs against any checkout of this
project (--tree, default: the one this file is in).  The loaded library handle is wrapped: every bm_* call appends its
name and its integer / float arguments (pointers left out; the fields of bm_step_params included) to a list.  A matrix
of configurations runs three steps each on seeded inputs at d = 4 099, and each prints two SHA-256 digests: of the call
list, and of the results (defense vector, update_gradient(), the floats() dictionary, last_factor, last_search).
Two checkouts agree when their tables are equal line by line (`diff`); --show prints one configuration's calls.

Matrix: every rule x placement x clipping x ks in (h, h + 1) x (n, f) in (11, 2), (25, 5), (51, 12), with
  fixed factor:  f_real in (0, f); single_call off as well where it could be on (worker placement, the six rules of
                 bm_step_worker); gar_args {"m": n - f - 3} as well for krum / bulyan (the rules that take m)
  attack_evals 4: the three values of line_search with f_real = f, and f_real = 0 (no search runs) under "auto".
Brute runs at (11, 2) only: its subsets at n = 25 and 51 are not a step anybody waits for.  One process, one GPU; a
configuration whose arguments the library refuses, or whose floats() meets a zero norm (ZeroDivisionError), is recorded
as refused with the exception's type; after a device error nothing more is run.
Behind that matrix, the other attacks (names "...-<attack>-..."): little, anticge, nan, hidden with target_idx -1 and
"all", empire-strict (epsilon 2) x every rule x placement x clipping at (11, 2) and (25, 5), ks = h, f_real = f:
  fixed factor, little without the single call as well where it could be on;
  attack_evals 4 for the searchable ones under line_search "auto" and "host", hidden with attack_negative as well.

--backend oracle: the same matrix on CPU tensors with tests/sharded_backend.OracleBackend (of --tree), no GPU.  What is
recorded is every method call on the backend and on the ShardedAggregator the step holds: the name, the int / float /
str / bool / None arguments, shape and dtype of tensors and of lists of tensors.  That backend declares no
capabilities: this is the capability-less plan of every configuration; a configuration it cannot run is recorded as
refused.  The device forms are what the default mode covers."""
import argparse
import ctypes
import hashlib
import inspect
import itertools
import os
import sys

D = 4099
STEPS = 3
RULES = ("krum", "bulyan", "median", "trmean", "phocas", "meamed", "aksel", "brute", "average", "cge")
NUMBERS = (ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double)


def plain(value):
  value = getattr(value, "value", value)
  return value.hex() if isinstance(value, float) else value


class TracedLibrary:
  def __init__(self, lib, signatures, log):
    self._lib, self._signatures, self._log = lib, signatures, log

  def __getattr__(self, name):
    fn = getattr(self._lib, name)
    if not name.startswith("bm_") or name not in self._signatures:
      return fn
    kinds = self._signatures[name][1]

    def call(*args):
      entry = [name]
      for arg, kind in zip(args, kinds):
        if isinstance(getattr(arg, "_obj", None), ctypes.Structure):  # byref(bm_step_params)
          entry += [plain(getattr(arg._obj, field)) for field, _ in arg._obj._fields_]
        elif kind in NUMBERS:
          entry.append(plain(kind(getattr(arg, "value", arg))))
      self._log.append(tuple(entry))
      return fn(*args)
    self.__dict__[name] = call
    return call


def configurations():
  for (n, f), gar, placement, clip, extra in itertools.product(((11, 2), (25, 5), (51, 12)), RULES,
                                                               ("worker", "server", "update"), (None, 2.0), (0, 1)):
    if gar == "brute" and n != 11:
      continue
    base = dict(n=n, f=f, gar=gar, momentum_at=placement, gradient_clip=clip, extra=extra)
    for gar_args in ({}, {"m": n - f - 3}) if gar in ("krum", "bulyan") else ({},):
      for f_real in (0, f):
        for single_call in (True, False) if placement == "worker" and gar in RULES[:6] else (True,):
          yield dict(base, gar_args=gar_args, f_real=f_real, single_call=single_call, attack_evals=None, line_search="auto")
      for line_search, f_real in (("auto", f), ("host", f), ("generic", f), ("auto", 0)):
        yield dict(base, gar_args=gar_args, f_real=f_real, single_call=True, attack_evals=4, line_search=line_search)


def attack_configurations():
  attacks = (("little", {}), ("anticge", {}), ("nan", {}), ("hidden", {"attack_args": {"target_idx": -1}}),
             ("hidden-all", {"attack_args": {"target_idx": "all"}}), ("empire-strict", {"attack_factor": 2}))
  for (n, f), gar, placement, clip in itertools.product(((11, 2), (25, 5)), RULES, ("worker", "server", "update"),
                                                        (None, 2.0)):
    if gar == "brute" and n != 11:
      continue
    base = dict(n=n, f=f, gar=gar, momentum_at=placement, gradient_clip=clip, extra=0, gar_args={}, f_real=f)
    for label, more in attacks:
      attack = label.split("-all")[0]
      fixed = dict(base, label=label, more=dict(more, attack=attack), attack_evals=None, line_search="auto")
      yield dict(fixed, single_call=True)
      if attack == "little" and placement == "worker" and gar in RULES[:6]:
        yield dict(fixed, single_call=False)
      if attack in ("anticge", "nan"):
        continue
      for line_search in ("auto", "host"):
        for negative in (False, True) if attack == "hidden" else (False,):
          yield dict(fixed, single_call=True, attack_evals=4, line_search=line_search,
                     more=dict(more, attack=attack, attack_negative=negative))


def name_of(cfg):
  attack = f"-{cfg['label']}{'-neg' if cfg['more'].get('attack_negative') else ''}" if "label" in cfg else ""
  return (f"n{cfg['n']}f{cfg['f']}r{cfg['f_real']}-{cfg['gar']}{'-m' if cfg['gar_args'] else ''}-{cfg['momentum_at']}"
          f"-{'clip' if cfg['gradient_clip'] else 'noclip'}-ks+{cfg['extra']}{attack}-"
          + (f"evals4-{cfg['line_search']}" if cfg["attack_evals"] else ("call" if cfg["single_call"] else "sequence")))


def digest(items):
  return hashlib.sha256(repr(items).encode()).hexdigest()[:24]


def described(torch, value):
  """An argument as the oracle mode records it."""
  if isinstance(value, torch.Tensor):
    return ("tensor", tuple(value.shape), str(value.dtype))
  if isinstance(value, (list, tuple)) and value and all(isinstance(v, torch.Tensor) for v in value):
    return ("tensors", len(value), tuple(value[0].shape), str(value[0].dtype))
  if value is None or isinstance(value, (bool, int, str)):
    return value
  if isinstance(value, float):
    return value.hex()
  if isinstance(value, dict):
    return sorted((key, described(torch, val)) for key, val in value.items())
  return type(value).__name__


def record_methods(torch, obj, owner, log):
  """Every method of `obj` (its class's, the private ones too) appends (owner, name, arguments) to `log` when called."""
  for name, member in inspect.getmembers(type(obj)):
    if name.startswith("__") or not callable(member) or isinstance(member, type):
      continue

    def call(*args, _fn=getattr(obj, name), _name=name, **kwargs):
      log.append((owner, _name) + tuple(described(torch, a) for a in args)
                 + tuple((key, described(torch, val)) for key, val in sorted(kwargs.items())))
      return _fn(*args, **kwargs)
    setattr(obj, name, call)
  return obj


def run(cfg, torch, AggregationStep, log, aggregator=None):
  """(calls, results) of STEPS steps of one configuration."""
  device = torch.device("cpu" if aggregator else "cuda:0")
  n, f, f_real = cfg["n"], cfg["f"], cfg["f_real"]
  h = n - f_real
  more = dict(cfg.get("more", {}), **({"aggregator": aggregator()} if aggregator else {}))
  step = AggregationStep(n, f, f_real, gar=cfg["gar"], gar_args=cfg["gar_args"], momentum=0.9, dampening=0.9,
                         momentum_at=cfg["momentum_at"], **{"attack_factor": 1.1, **more}, nb_past=2,
                         gradient_clip=cfg["gradient_clip"],
                         single_call=cfg["single_call"], attack_evals=cfg["attack_evals"], line_search=cfg["line_search"])
  gen = torch.Generator().manual_seed(1234)
  origin = torch.randn(D, generator=gen).to(device)
  params = (origin + 0.01).contiguous()
  del log[:]
  results = []
  for _ in range(STEPS):
    sampled = [torch.randn(D, generator=gen).mul_(1.0 + 0.1 * i).to(device) for i in range(h + cfg["extra"])]
    defense = step.run(sampled, params, origin)
    floats = step.floats()
    search = step.last_search
    results.append((defense.cpu().numpy().tobytes(), step.update_gradient().cpu().numpy().tobytes(),
                    sorted((key, float(val).hex()) for key, val in floats.items()), float(step.last_factor).hex(),
                    None if search is None else [(float(x).hex(), float(y).hex()) for x, y in search]))
  return list(log), results


def main():
  parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
  parser.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
  parser.add_argument("--out", help="write the table here as well")
  parser.add_argument("--show", help="print the calls of the configuration of this name and stop")
  parser.add_argument("--backend", choices=("hip", "oracle"), default="hip")
  args = parser.parse_args()
  sys.path.insert(0, os.path.abspath(args.tree))
  import torch
  from byzantinemomentum_amd import _lib
  from byzantinemomentum_amd.step import AggregationStep
  log, aggregator = [], None
  if args.backend == "oracle":
    torch.set_num_threads(1)  # vectors of 4 099 numbers: threads only wait for one another (minutes against an hour)
    from byzantinemomentum_amd.sharded import ShardedAggregator
    from tests.sharded_backend import OracleBackend

    def aggregator():
      backend = record_methods(torch, OracleBackend(), "backend", log)
      return record_methods(torch, ShardedAggregator(backend=backend), "aggregator", log)
  else:
    _lib._lib = TracedLibrary(_lib.load(), _lib.SIGNATURES, log)
  lines, plans = [], set()
  for cfg in itertools.chain(configurations(), attack_configurations()):
    name = name_of(cfg)
    if args.show and name != args.show:
      continue
    try:
      calls, results = run(cfg, torch, AggregationStep, log, aggregator)
    except (Exception if aggregator else (ValueError, RuntimeError, ArithmeticError)) as err:
      try:
        if not aggregator:
          torch.cuda.synchronize()  # a refusal of the arguments leaves the device alone; a device error does not
      except RuntimeError:
        print(f"{name}: device error, stopping: {err}", flush=True)
        return 1
      calls, results = list(log), f"refused: {type(err).__name__}: {err}"
    if args.show:
      print("\n".join(repr(c) for c in calls))
      return 0
    plans.update(".".join(c[:2]) if aggregator else c[0] for c in calls)
    lines.append(f"{name} calls={digest(calls)} n_calls={len(calls)} results={digest(results)}"
                 + (f" REFUSED {results.split(': ')[1]}" if isinstance(results, str) else ""))
  lines.append(f"# {len(lines)} configurations, {len(plans)} entry points reached: {' '.join(sorted(plans))}")
  text = "\n".join(lines) + "\n"
  sys.stdout.write(text)
  if args.out:
    with open(args.out, "w") as out:
      out.write(text)
  return 0


if __name__ == "__main__":
  sys.exit(main())
