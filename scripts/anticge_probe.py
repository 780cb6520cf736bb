"""A/B of the `anticge` attack on one GPU: the chain of this library (bm_row_sqnorms -> bm_anticge_sum ->
bm_anticge_scale) against the same attack composed from the exports the library had before it
(bm_row_sqnorms -> bm_stable_argsort -> bm_selected_mean over the index table with the smallest row twice ->
bm_row_sqnorms of the mean -> bm_multi_scale), alternating in one process, HIP events, medians.

    python scripts/anticge_probe.py [--cases 20:5:36489290,39:12:11173962] [--rounds 20] [--out FILE]

The composition forms its factor with a few torch operations on device scalars (no host round trip either); its
selected mean is S / m, so the factor carries m.  Bytes the new chain needs: 4 d (h + maxpos + 4): h rows for the norms,
maxpos rows read and S written by the sum, S read and written by the scaling; the composition reads its result once
more for the norm.  The fraction of 8 TB/s is those bytes over the median."""

import argparse
import pathlib
import statistics
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from byzantinemomentum_amd import gars, stats  # noqa: E402

PEAK = 8e12


def timed(fn, stream):
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record(stream)
  out = fn()
  stop.record(stream)
  stop.synchronize()
  return start.elapsed_time(stop) * 1e3, out  # microseconds


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--cases", default="20:5:36489290,39:12:11173962")
  ap.add_argument("--rounds", type=int, default=20)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("anticge_probe needs a GPU")
  dev = torch.device("cuda", 0)
  stream = torch.cuda.current_stream(dev)
  lines = []

  def say(text):
    print(text, flush=True)
    lines.append(text)

  for case in args.cases.split(","):
    h, f_decl, d = (int(v) for v in case.split(":"))
    maxpos = h - f_decl
    gen = torch.Generator(device=dev).manual_seed(11)
    rows = [(0.5 + i / h) * torch.randn(d, device=dev, generator=gen) for i in range(h)]

    def new_chain():
      sq = stats.row_sqnorms(rows).contiguous()
      byz, _, scal = stats.anticge_sum(rows, f_decl, sq)
      return stats.anticge_scale(byz, scal)

    def composed():
      sq = stats.row_sqnorms(rows).contiguous()
      order = gars.stable_argsort(sq, h)
      table = torch.cat([order[:1], order[:maxpos]]).contiguous()
      mean = gars.selected_mean(rows, table, maxpos + 1)
      norm2 = stats.row_sqnorms([mean])
      byznorm = sq[order[maxpos].long()].sqrt().float().double()
      attnorm = (norm2[0].sqrt() * (maxpos + 1)).float().double()
      factor = (-torch.nextafter(byznorm, torch.zeros_like(byznorm)) / attnorm * (maxpos + 1)).float().reshape(1)
      stats.multi_scale([mean], factor)
      return mean

    for _ in range(3):
      a, b = new_chain(), composed()
    torch.cuda.synchronize()
    diff = float((a - b).abs().max() / a.abs().max())
    t_new, t_old = [], []
    for _ in range(args.rounds):
      t_new.append(timed(new_chain, stream)[0])
      t_old.append(timed(composed, stream)[0])
    # the legs of the new chain, each between its own events
    legs = {"row_sqnorms": [], "anticge_sum": [], "anticge_scale": []}
    for _ in range(max(args.rounds // 2, 3)):
      t, sq = timed(lambda: stats.row_sqnorms(rows).contiguous(), stream)
      legs["row_sqnorms"].append(t)
      t, (byz, _, scal) = timed(lambda: stats.anticge_sum(rows, f_decl, sq), stream)
      legs["anticge_sum"].append(t)
      legs["anticge_scale"].append(timed(lambda: stats.anticge_scale(byz, scal), stream)[0])
    old_legs = {"row_sqnorms": [], "selected_mean": [], "norm_of_result": [], "multi_scale": []}
    for _ in range(max(args.rounds // 2, 3)):
      t, sq = timed(lambda: stats.row_sqnorms(rows).contiguous(), stream)
      old_legs["row_sqnorms"].append(t)
      order = gars.stable_argsort(sq, h)
      table = torch.cat([order[:1], order[:maxpos]]).contiguous()
      t, mean = timed(lambda: gars.selected_mean(rows, table, maxpos + 1), stream)
      old_legs["selected_mean"].append(t)
      old_legs["norm_of_result"].append(timed(lambda: stats.row_sqnorms([mean]), stream)[0])
      one = torch.full((1,), 0.5, device=dev)
      old_legs["multi_scale"].append(timed(lambda: stats.multi_scale([mean], one), stream)[0])
    med_new, med_old = statistics.median(t_new), statistics.median(t_old)
    nbytes = 4 * d * (h + maxpos + 4)
    say(f"h={h} f_decl={f_decl} d={d}: new chain median {med_new:.1f} us (min {min(t_new):.1f}, max {max(t_new):.1f}), "
        f"composition median {med_old:.1f} us (min {min(t_old):.1f}, max {max(t_old):.1f}), {args.rounds} alternations; "
        f"new chain {nbytes / 1e9:.2f} GB -> {nbytes / (med_new * 1e-6) / PEAK:.3f} of 8 TB/s; "
        f"max|new - composed| / max|new| = {diff:.2e}")
    say("  new chain legs (median us): " + ", ".join(f"{k} {statistics.median(v):.1f}" for k, v in legs.items()))
    say("  composition legs (median us): " + ", ".join(f"{k} {statistics.median(v):.1f}" for k, v in old_legs.items()))
    del rows
    torch.cuda.empty_cache()
  if args.out:
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
  main()
