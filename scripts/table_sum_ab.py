"""A/B of the row-table sums (bm_selected_mean, bm_anticge_sum, bm_weighted_sum) between two builds of the library on one
GPU: the same inputs through both, a sha256 of every output, then the two alternating in one process with HIP events
around each call and medians, as scripts/anticge_probe.py does.

    python scripts/table_sum_ab.py --parent PATH/TO/OLDER/libbm_gar.so [--rounds 20] [--out FILE]

The bar of the timing is the older build's own spread: a copy of it runs in the same alternation as a third library
(the three rotate through the places of a round), and a kernel counts as unchanged when the median of new / parent lies
inside the range the per-round ratios copy / parent span.  Both builds are loaded with ctypes side by side (their
symbols stay local to each handle)."""

import argparse
import ctypes
import hashlib
import math
import pathlib
import shutil
import statistics
import sys
import tempfile

import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from byzantinemomentum_amd import _lib, stats  # noqa: E402

D_C3, D_C5 = 11173962, 36489290


def open_library(path):
  lib = ctypes.CDLL(str(path))
  for name, (restype, argtypes) in _lib.SIGNATURES.items():
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = restype, argtypes
  assert lib.bm_abi_version() == _lib.ABI_VERSION, path
  return lib


def ptr(t):
  return ctypes.c_void_p(t.data_ptr())


def sha(t):
  torch.cuda.synchronize()
  return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def rows_at(n, d, offset, gen):
  """n rows of d floats, each `offset` floats behind a 256-byte boundary."""
  per = -(-(d + offset) // 64) * 64
  pool = torch.zeros(n * per, dtype=torch.float32, device="cuda:0")
  views = [pool[i * per + offset:i * per + offset + d] for i in range(n)]
  for i, v in enumerate(views):
    v.copy_((0.5 + i / n) * torch.randn(d, device="cuda:0", generator=gen))
  return views


def mean_call(lib, rows, idx, m):
  out = torch.empty_like(rows[0])
  stream = torch.cuda.current_stream().cuda_stream
  table = _lib.pointer_table(rows)

  def call():
    code = lib.bm_selected_mean(table, len(rows), ptr(idx), m, rows[0].numel(), ptr(out), stream)
    assert code == 0, code
    return [out]
  return call


def anticge_call(lib, rows, f_decl, row_sq):
  d = rows[0].numel()
  out = torch.empty_like(rows[0])
  order = torch.empty(_lib.MAX_ROWS, dtype=torch.int32, device="cuda:0")
  scal = torch.empty(2, dtype=torch.float64, device="cuda:0")
  ws = torch.empty(int(lib.bm_anticge_workspace_bytes(d)), dtype=torch.uint8, device="cuda:0")
  stream = torch.cuda.current_stream().cuda_stream
  table = _lib.pointer_table(rows)

  def call():
    code = lib.bm_anticge_sum(table, len(rows), d, f_decl, ptr(row_sq), ptr(out), ptr(order), ptr(scal), ptr(ws), stream)
    assert code == 0, code
    return [out, scal[:1]]
  return call


def wsum_call(lib, rows, weights):
  out = torch.empty_like(rows[0])
  w = torch.tensor(weights, dtype=torch.float64, device="cuda:0")
  stream = torch.cuda.current_stream().cuda_stream
  table = _lib.pointer_table(rows)

  def call():
    code = lib.bm_weighted_sum(table, len(rows), ptr(w), rows[0].numel(), ptr(out), stream)
    assert code == 0, code
    return [out]
  return call


def timed(fn):
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  fn()
  stop.record()
  stop.synchronize()
  return start.elapsed_time(stop) * 1e3  # microseconds


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--parent", required=True)
  ap.add_argument("--new", default=str(_lib.LIB_PATH))
  ap.add_argument("--rounds", type=int, default=20)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("table_sum_ab needs a GPU")
  lines = []

  def say(text):
    print(text, flush=True)
    lines.append(text)

  with tempfile.TemporaryDirectory() as tmp:
    copy = shutil.copy(args.parent, pathlib.Path(tmp) / "libbm_gar_parent_copy.so")
    libs = {"parent": open_library(args.parent), "new": open_library(args.new), "copy": open_library(copy)}
    gen = torch.Generator(device="cuda:0").manual_seed(11)
    equal = True

    def digests(tag, make):
      nonlocal equal
      got = {name: [sha(t) for t in make(lib)()] for name, lib in libs.items() if name != "copy"}
      same = got["parent"] == got["new"]
      equal &= same
      say(f"digest {tag}: parent {' '.join(got['parent'])} | new {' '.join(got['new'])} | {'equal' if same else 'DIFFERENT'}")

    def race(tag, make, nbytes):
      calls = {name: make(lib) for name, lib in libs.items()}
      for _ in range(3):
        for call in calls.values():
          call()
      torch.cuda.synchronize()
      t = {name: [] for name in calls}
      order = list(calls)
      for r in range(args.rounds):  # (the call behind a pause runs a few percent faster: every library takes every place)
        for name in order[r % 3:] + order[:r % 3]:
          t[name].append(timed(calls[name]))
      med = {name: statistics.median(v) for name, v in t.items()}
      new_ratio = statistics.median(n / p for n, p in zip(t["new"], t["parent"]))
      own = [c / p for c, p in zip(t["copy"], t["parent"])]
      verdict = "unchanged" if min(own) <= new_ratio <= max(own) else ("FASTER" if new_ratio < min(own) else "SLOWER")
      say(f"time {tag}: parent {med['parent']:.1f} us, new {med['new']:.1f} us, parent copy {med['copy']:.1f} us "
          f"({args.rounds} alternations); median new/parent {new_ratio:.4f}, parent copy/parent spans "
          f"[{min(own):.4f}, {max(own):.4f}] -> {verdict}; new: {nbytes / (med['new'] * 1e-6) / 1e12:.2f} TB/s")

    # --- the mean
    rows = rows_at(40, D_C3, 0, gen)
    for m in (7, 37):
      idx = torch.zeros(_lib.MAX_ROWS, dtype=torch.int32, device="cuda:0")
      idx[:m] = torch.randperm(40, device="cuda:0", generator=gen)[:m].int()
      digests(f"mean m={m} d={D_C3}", lambda lib: mean_call(lib, rows, idx, m))
      race(f"mean m={m} d={D_C3}", lambda lib: mean_call(lib, rows, idx, m), 4 * D_C3 * (m + 1))
    small = rows_at(11, 4099, 0, gen)
    idx = torch.tensor([3, 1, -1, 7] + [0] * 60, dtype=torch.int32, device="cuda:0")
    digests("mean m=4 d=4099, a negative index", lambda lib: mean_call(lib, small, idx, 4))
    # --- the weighted sum (the 40 rows above)
    stack = rows[:21] + [rows[20]] * 4
    weights = [0.01 + 0.005 * i for i in range(25)]
    digests(f"weighted sum 25 rows, five references to one, d={D_C3}", lambda lib: wsum_call(lib, stack, weights))
    digests("weighted sum, a NaN weight", lambda lib: wsum_call(lib, stack, weights[:9] + [math.nan] + weights[10:]))
    digests("weighted sum, every weight zero", lambda lib: wsum_call(lib, stack, [0.0] * 25))
    w21 = [(-1) ** i * (0.02 + 0.003 * i) for i in range(21)]
    race(f"weighted sum 21 distinct rows d={D_C3}", lambda lib: wsum_call(lib, rows[:21], w21), 4 * D_C3 * 22)
    # --- anticge
    sq = stats.row_sqnorms(rows[:39]).contiguous()
    race(f"anticge sum h=39 f_decl=12 d={D_C3}", lambda lib: anticge_call(lib, rows[:39], 12, sq), 4 * D_C3 * 28)
    for offset in (0, 2, 1):
      nine = rows_at(9, 4099, offset, gen)
      sq9 = stats.row_sqnorms(nine).contiguous()
      digests(f"anticge h=9 f_decl=2 d=4099 offset {offset}: S, scal[0]", lambda lib: anticge_call(lib, nine, 2, sq9))
    del rows, stack, small
    torch.cuda.empty_cache()
    rows = rows_at(20, D_C5, 0, gen)
    sq = stats.row_sqnorms(rows).contiguous()
    digests(f"anticge h=20 f_decl=5 d={D_C5}: S, scal[0]", lambda lib: anticge_call(lib, rows, 5, sq))
    race(f"anticge sum h=20 f_decl=5 d={D_C5}", lambda lib: anticge_call(lib, rows, 5, sq), 4 * D_C5 * 16)
    say("all digests equal" if equal else "DIGESTS DIFFER")
  if args.out:
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text("\n".join(lines) + "\n")
  return 0 if equal else 1


if __name__ == "__main__":
  sys.exit(main())
