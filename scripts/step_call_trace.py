"""Which library calls a step makes, and what it computes: the check that a change of the host mirror (step.py,
stats.py, the host code of bm_step_worker) left both alone.

    python scripts/step_call_trace.py [--tree DIR] [--out FILE] [--show NAME]

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
configuration whose arguments the library refuses is recorded as refused; after a device error nothing more is run."""
import argparse
import ctypes
import hashlib
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


def name_of(cfg):
  return (f"n{cfg['n']}f{cfg['f']}r{cfg['f_real']}-{cfg['gar']}{'-m' if cfg['gar_args'] else ''}-{cfg['momentum_at']}"
          f"-{'clip' if cfg['gradient_clip'] else 'noclip'}-ks+{cfg['extra']}-"
          + (f"evals4-{cfg['line_search']}" if cfg["attack_evals"] else ("call" if cfg["single_call"] else "sequence")))


def digest(items):
  return hashlib.sha256(repr(items).encode()).hexdigest()[:24]


def run(cfg, torch, AggregationStep, log):
  """(calls, results) of STEPS steps of one configuration."""
  device = torch.device("cuda:0")
  n, f, f_real = cfg["n"], cfg["f"], cfg["f_real"]
  h = n - f_real
  step = AggregationStep(n, f, f_real, gar=cfg["gar"], gar_args=cfg["gar_args"], momentum=0.9, dampening=0.9,
                         momentum_at=cfg["momentum_at"], attack_factor=1.1, nb_past=2, gradient_clip=cfg["gradient_clip"],
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
  args = parser.parse_args()
  sys.path.insert(0, os.path.abspath(args.tree))
  import torch
  from byzantinemomentum_amd import _lib
  from byzantinemomentum_amd.step import AggregationStep
  log = []
  _lib._lib = TracedLibrary(_lib.load(), _lib.SIGNATURES, log)
  lines, plans = [], set()
  for cfg in configurations():
    name = name_of(cfg)
    if args.show and name != args.show:
      continue
    try:
      calls, results = run(cfg, torch, AggregationStep, log)
    except (ValueError, RuntimeError) as err:
      try:
        torch.cuda.synchronize()  # a refusal of the arguments leaves the device alone; a device error does not
      except RuntimeError:
        print(f"{name}: device error, stopping: {err}", flush=True)
        return 1
      calls, results = list(log), f"refused: {type(err).__name__}: {err}"
    if args.show:
      print("\n".join(repr(c) for c in calls))
      return 0
    plans.update(c[0] for c in calls)
    lines.append(f"{name} calls={digest(calls)} n_calls={len(calls)} results={digest(results)}"
                 + (" REFUSED" if isinstance(results, str) else ""))
  lines.append(f"# {len(lines)} configurations, {len(plans)} entry points reached: {' '.join(sorted(plans))}")
  text = "\n".join(lines) + "\n"
  sys.stdout.write(text)
  if args.out:
    with open(args.out, "w") as out:
      out.write(text)
  return 0


if __name__ == "__main__":
  sys.exit(main())
