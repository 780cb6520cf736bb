"""A/B of the `hidden` attack's vector on one GPU: (a) bm_attack_vector forming avg + factor * dir from the coordinate's
index (two streams: avg read, the vector written) against (b) the way the library had before it, bm_multi_fma3 on a
MATERIALISED 0 / 1 direction vector (three streams; forming the direction is not timed), alternating in one process, HIP
events around each call, medians.

    python scripts/attack_vector_probe.py [--lengths 36489290,11173962] [--rounds 20] [--out FILE]

Both write into the same preallocated output, so no allocation is timed.  The fraction of 8 TB/s is each form's own bytes
(8 d for the kernel, 12 d for the composition) over its median; "spread" is the range of the alternations."""

import argparse
import pathlib
import statistics
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from byzantinemomentum_amd import _lib, gars, stats  # noqa: E402

PEAK = 8e12
FACTOR = 1.5


def timed(fn, stream):
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record(stream)
  fn()
  stop.record(stream)
  stop.synchronize()
  return start.elapsed_time(stop) * 1e3  # microseconds


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--lengths", default="36489290,11173962")
  ap.add_argument("--rounds", type=int, default=20)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("attack_vector_probe needs a GPU")
  dev = torch.device("cuda", 0)
  stream = torch.cuda.current_stream(dev)
  lib = _lib.load()
  lines = []

  def say(text):
    print(text, flush=True)
    lines.append(text)

  say(f"attack_vector_probe: {torch.cuda.get_device_name(dev)}, {args.rounds} alternations, factor {FACTOR}")
  for d in (int(v) for v in args.lengths.split(",")):
    gen = torch.Generator(device=dev).manual_seed(11)
    avg = torch.randn(d, device=dev, generator=gen)
    out_a, out_b = torch.empty_like(avg), torch.empty_like(avg)
    for kind, target in (("shift_one", d - 1), ("shift_all", -1)):
      direction = torch.ones_like(avg) if kind == "shift_all" else torch.zeros_like(avg)
      if kind == "shift_one":
        direction[target] = 1

      def kernel():
        _lib.check(lib.bm_attack_vector(_lib.ATTACK_VECTOR_KINDS[kind], gars._ptr(avg), d, target, FACTOR, None,
                                        gars._ptr(out_a), None, gars._stream(dev)), "bm_attack_vector")

      def composition():
        stats.multi_fma3([out_b], [avg], [direction], 1.0, FACTOR)

      for _ in range(3):
        kernel()
        composition()
      torch.cuda.synchronize(dev)
      same = torch.equal(out_a, out_b)
      ta, tb = [], []
      for _ in range(args.rounds):
        ta.append(timed(kernel, stream))
        tb.append(timed(composition, stream))
      ma, mb = statistics.median(ta), statistics.median(tb)
      say(f"d={d} {kind}: kernel {ma:.1f} us ({8 * d / (ma * 1e-6) / PEAK:.2f} of 8 TB/s, spread {min(ta):.1f}..{max(ta):.1f})"
          f" | multi_fma3 on a direction vector {mb:.1f} us ({12 * d / (mb * 1e-6) / PEAK:.2f} of 8 TB/s, spread "
          f"{min(tb):.1f}..{max(tb):.1f}) | same bits: {same}")
  if args.out:
    pathlib.Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
