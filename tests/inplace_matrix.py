"""The small streaming kernels a step falls back to whenever its first pass does not fuse, and the scalar reductions
beside them: what a call launches, seeded inputs inside guard gaps, and expected values made of the inputs alone (a
helper module, not a conftest; the shape of tests/mix_matrix.py).

  multi_axpby_kernel<1,2,4>     reduce.hip    bm_multi_axpby                      y <- fma(b, x, fl32(a y))
  multi_fma3_kernel<1,2,4>      step.hip      bm_multi_fma3, bm_multi_fma3_bdev   out <- fma(b, q, fl32(a fl32(c p)))
  multi_scale_kernel<1,2,4>     step.hip      bm_multi_scale                      y <- fl32(y c), rows of c == 1 untouched
  anticge_scale_kernel<1,2,4>   anticge.hip   bm_anticge_scale                    v <- fl32(v m), untouched unless |S| > 0
  clip_factors_kernel           step.hip      bm_clip_factors
  row_sqnorms_kernel<1,2,4>     reduce.hip    bm_row_sqnorms
  sqdist2_kernel<1,2,4>         search_eval.hip  bm_sqdist2
  multi_dot_kernel<1,2,4>       reduce.hip    bm_multi_dot

Three parts:
  * a mirror of the launch sites: `launches(entry, byte offsets, d)` restates Alignment and
    for_body_and_tail(Tail::kOwnLaunch, ...) of launch_plan.h with each site's block and caps — per launch the width, the
    grid, the trips a lane takes and how many workgroups take a second one; `sqnorm_walk` / `sqdist_walk` the fp32 -> fp64
    folds of the two sums of squares.  It imports nothing from the package; tests/test_inplace_matrix_cpu.py holds it to
    the sources;
  * inputs: every vector of a case is cut from ONE flat allocation, at least GUARD floats of a sentinel bit pattern before
    and after each; ordinary rows whose scale differs by row with SPECIAL elements (KINDS) at the start, in the middle of
    the first wave and over the last columns, each kind in every lane position of a 16-byte group and in the tail;
  * references on the CPU: the fused step through first_pass_matrix.fma_emulated, the coordinates it flags as fp32
    midpoints and every coordinate whose result lies below the smallest normal evaluated exactly (fractions.Fraction,
    one rounding) — no coordinate is left out of a comparison; float64 sums for the reductions.
"""

import functools
import math
import os
import sys
from collections import namedtuple
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

F32 = np.float32

# ---------------------------------------------------------------------------------------------------------------------
# Mirror of the launch sites (launch_plan.h; reduce.hip, step.hip, anticge.hip, search_eval.hip, colwise_kernels.h)

AXPBY, FMA3, SCALE, ANTICGE, SQNORMS, SQDIST2, DOT = "axpby", "fma3", "scale", "anticge_scale", "row_sqnorms", "sqdist2", "multi_dot"
WRITERS = (AXPBY, FMA3, SCALE, ANTICGE)
REDUCTIONS = (SQNORMS, SQDIST2, DOT)

BM_MAX_ROWS = 64
MAX_VEC = 4                       # for_body_and_tail<4> at every site
TAIL_OWN_LAUNCH = True            # Tail::kOwnLaunch at every site

Site = namedtuple("Site", "kernel source block cap_body cap_tail")
SITES = {
  AXPBY: Site("multi_axpby_kernel", "reduce.hip", 256, 2048, 2048),            # kRedBlock, caps_of(2048)
  FMA3: Site("multi_fma3_kernel", "step.hip", 256, 2048, 2048),                # kStepBlock, caps_of(2048)
  SCALE: Site("multi_scale_kernel", "step.hip", 256, 2048, 2048),              # kStepBlock, caps_of(2048)
  ANTICGE: Site("anticge_scale_kernel", "anticge.hip", 256, 2048, 2048),       # kAcgScaleBlock, caps_of(kAcgScaleBlocks)
  SQNORMS: Site("row_sqnorms_kernel", "reduce.hip", 256, 128, 128),            # kRedBlock, caps_of(kNormBlocks)
  SQDIST2: Site("sqdist2_kernel", "search_eval.hip", 256, 2048, 2048),         # kColBlock, kEvalCaps
  DOT: Site("multi_dot_kernel", "reduce.hip", 256, 1024, 1024),                # kRedBlock, kDotCaps
}
K_NORM_LOADS = 2                  # row_sqnorms_kernel: two loads in flight per lane and iteration
K_FOLD_EVERY = 16                 # both sums of squares fold their fp32 chains into fp64 every 16 iterations
K_MAX_CORE, K_MAX_EXTRA = 4, 32
K_DOT_SLOTS = K_MAX_CORE * (K_MAX_CORE + 1) // 2 + K_MAX_EXTRA   # 42


def universe():
  """Every (kernel, width) instance of the seven families: 21."""
  return {(s.kernel, w) for s in SITES.values() for w in (1, 2, 4)}


def vec_of(byte_offsets):
  """Alignment::vec: the widest vector every pointer allows."""
  bits = 0
  for o in byte_offsets:
    bits |= int(o)
  return 4 if bits & 15 == 0 else (2 if bits & 7 == 0 else 1)


def stream_grid(work, block, cap):
  return min(max(-(-work // block), 1), cap)


# One launch: `count` vectors of `width` floats from coordinate `first`; trips: the most a lane loops; second: how many
# workgroups hold a lane that loops twice; alone: a VEC = 1 launch with no body before it (it takes the whole grid).
Launch = namedtuple("Launch", "width first count grid trips second alone")


def _launch(width, first, count, grid, block, alone):
  stride = grid * block
  second = -(-(count - stride) // block) if count > stride else 0
  return Launch(width, first, count, grid, -(-count // stride), min(second, grid), alone)


def for_body_and_tail(vec, d, block, cap_body, cap_tail):
  """for_body_and_tail<4>(Tail::kOwnLaunch, vec, d, block, Caps{cap_body, cap_tail}, ...): the launches in order."""
  assert TAIL_OWN_LAUNCH
  out = []
  vec = min(vec, MAX_VEC)
  if d // vec == 0:
    vec = 1
  nvec = d // vec
  body = 0
  if d > 0 and vec > 1:
    body = nvec * vec
    out.append(_launch(vec, 0, nvec, stream_grid(nvec, block, cap_body), block, False))
  if body < d:
    rest = d - body
    out.append(_launch(1, body, rest, stream_grid(rest, block, cap_tail) if body == 0 else 1, block, body == 0))
  return out


def launches(entry, byte_offsets, d):
  s = SITES[entry]
  return for_body_and_tail(vec_of(byte_offsets), d, s.block, s.cap_body, s.cap_tail)


def instances(entry, byte_offsets, d):
  return {(SITES[entry].kernel, l.width) for l in launches(entry, byte_offsets, d)}


def forms(entry, byte_offsets, d):
  """Which launch forms a call takes: "tail_alone" (pointers wider than d: the VEC = 1 launch with the whole grid),
  "scalar" (4-byte pointers: the same launch for the whole row), "body", "tail_behind_body", "second_trip"."""
  ls = launches(entry, byte_offsets, d)
  out = set()
  for l in ls:
    if l.alone:
      out.add("tail_alone" if vec_of(byte_offsets) > 1 else "scalar")
    elif l.width > 1:
      out.add("body")
    else:
      out.add("tail_behind_body")
    if l.trips >= 2:
      out.add("second_trip")
  return out


def second_trip_d(entry, width):
  """The shortest d at which one WHOLE workgroup of the capped grid takes a second trip and the widest tail follows
  (width 1 has no tail launch: three lanes of a second workgroup loop as well)."""
  s = SITES[entry]
  return width * (s.cap_body * s.block + s.block) + (width - 1 if width > 1 else 3)


Walk = namedtuple("Walk", "iterations folds remainder_after_fold plain_remainder")


def sqnorm_walk(count, grid, block=256):
  """row_sqnorms_kernel over `count` vectors: the most two-load iterations a lane runs, how many lanes fold (16
  iterations or more), how many of those then take the single-load remainder, how many lanes take it without a fold."""
  stride = grid * block
  lanes = np.arange(min(stride, max(count, 1)), dtype=np.int64)
  # iteration i runs while lane + (2 i + 1) stride < count
  iters = np.maximum((count - lanes - stride + 2 * stride - 1) // (2 * stride), 0)
  iters = np.where(lanes + stride < count, iters, 0)
  rem = lanes + 2 * iters * stride < count
  fold = iters >= K_FOLD_EVERY
  return Walk(int(iters.max()) if iters.size else 0, int(fold.sum()), int((fold & rem).sum()), int((~fold & rem).sum()))


def sqdist_walk(count, grid, block=256):
  """sqdist2_kernel over `count` vectors: (the most iterations a lane runs, how many lanes fold)."""
  stride = grid * block
  lanes = np.arange(min(stride, max(count, 1)), dtype=np.int64)
  iters = np.maximum(-(-(count - lanes) // stride), 0)
  return int(iters.max()) if iters.size else 0, int((iters >= K_FOLD_EVERY).sum())


def sqnorm_areas(byte_offsets, d):
  """(nbody, ntail): the partials per row bm_row_sqnorms leaves in its body area (VEC > 1) and in its tail area."""
  nbody = ntail = 0
  for l in launches(SQNORMS, byte_offsets, d):
    if l.width == 1:
      ntail = l.grid
    else:
      nbody = l.grid
  return nbody, ntail


def sqnorm_fold_d(width):
  """A length at which every lane of row_sqnorms_kernel passes the fold, most then take the single-load remainder and
  five do not (35 strides and 5 vectors), with the widest tail behind it."""
  s = SITES[SQNORMS]
  stride = s.cap_body * s.block
  return width * ((K_NORM_LOADS * K_FOLD_EVERY + 3) * stride + 5) + (width - 1)


def sqdist_fold_d():
  """The shortest length at which a lane of sqdist2_kernel reaches its fold: 4-byte rows, lane 0 alone."""
  s = SITES[SQDIST2]
  return (K_FOLD_EVERY - 1) * s.cap_tail * s.block + 1


def dot_slot(a, b):
  """The slot of Gram entry (a, b), a <= b, in multi_dot_kernel's accumulators: the upper triangle of a 4 x 4 matrix."""
  slot = 0
  for i in range(K_MAX_CORE):
    for j in range(i, K_MAX_CORE):
      if (i, j) == (a, b):
        return slot
      slot += 1
  raise ValueError((a, b))


# ---------------------------------------------------------------------------------------------------------------------
# Layout: every vector of a case inside one flat allocation, guard gaps around each

GUARD = 32                               # floats, at least, before and after every vector
SENTINEL = np.uint32(0xCAFEF00D)         # a finite negative float: a kernel that reads it shows up in the outputs too
OFFSETS = (0, 4, 8, "mixed")


def row_offsets(offset, count, start=0):
  """Byte offset behind a 16-byte boundary of each of `count` vectors: the same for all, or for "mixed" 4, 0, 12, 8, ..."""
  if offset == "mixed":
    return [(4 + 12 * (start + i)) % 16 for i in range(count)]
  return [int(offset)] * count


def layout(specs):
  """specs: [(length, byte offset)] -> (floats of the allocation, start of every vector)."""
  pos, starts = 0, []
  for d, off in specs:
    pos += GUARD
    pos = -(-pos // 4) * 4 + off // 4
    starts.append(pos)
    pos += d
  pos += GUARD
  return -(-pos // 4) * 4, starts


class Flat:
  """The host image of one case: `bits` (uint32) full of the sentinel with the vectors written in."""

  def __init__(self, vectors, offsets):
    self.total, self.starts = layout([(len(v), o) for v, o in zip(vectors, offsets)])
    self.lengths = [len(v) for v in vectors]
    self.offsets = list(offsets)
    self.bits = np.full(self.total, SENTINEL, dtype=np.uint32)
    for v, s in zip(vectors, self.starts):
      self.bits[s:s + len(v)] = np.asarray(v, dtype=F32).view(np.uint32)

  def expected(self, outputs):
    """(bits after the call, mask of the elements where a NaN matches any NaN): outputs = {vector index: (values,
    exact)} — `exact` rows must keep their bits whatever they hold."""
    want = self.bits.copy()
    loose = np.zeros(self.total, dtype=bool)
    for i, (vals, exact) in outputs.items():
      s = self.starts[i]
      want[s:s + self.lengths[i]] = np.asarray(vals, dtype=F32).view(np.uint32)
      if not exact:
        loose[s:s + self.lengths[i]] = True
    return want, loose

  def where(self, index):
    """(vector index or None for a guard gap, position in it) of a flat index."""
    for i, (s, n) in enumerate(zip(self.starts, self.lengths)):
      if s <= index < s + n:
        return i, index - s
    return None, index


def first_mismatch(got_bits, want_bits, loose):
  """The first flat index where the bits differ (inside `loose` a NaN matches any NaN), or None."""
  bad = got_bits != want_bits
  if bad.any():
    both_nan = np.isnan(got_bits.view(F32)) & np.isnan(want_bits.view(F32))
    bad &= ~(loose & both_nan)
  hit = np.flatnonzero(bad)
  return int(hit[0]) if hit.size else None


# ---------------------------------------------------------------------------------------------------------------------
# Values

KINDS = ("nan_x", "nan_y", "inf", "inf_minus_inf", "zeros", "subnormal_in", "subnormal_out", "huge")
#  nan_x          NaN in x (the fma's multiplicand) only          nan_y   NaN in y (the operand scaled by a) only
#  inf            x = +inf or -inf (by column parity), y ordinary
#  inf_minus_inf  b x = +-inf against a y = -+inf: NaN out of two infinities inside the fma
#  zeros          +-0 in both operands, the four sign pairs by column
#  subnormal_in   both operands a few units of 2^-149
#  subnormal_out  normal operands about 2^-125: a result below 2^-126 at |a|, |b| < 1
#  huge           |x| in [3.2e38, 3.39e38], |y| in [2.3e38, 2.5e38], signs such that b x takes from a y: at a = 1.5 fl32(a y)
#                 is infinite although the exact sum is an fp32 number
NK = len(KINDS)
END = 36                                 # the last END columns: column d - 1 - j holds slot j % 9, slot 8 ordinary
STARTS = (0, 128)                        # sites: kind k, repeat r at site + 16 k + 5 r (lane positions 0 .. 3)


def kind_map(k, d):
  """int8 k x d: the kind of every element, -1 = ordinary.  The kind of a special column rotates with the row, so that
  from 8 rows on every special column — the trailing ones included — holds every kind."""
  out = np.full((k, d), -1, dtype=np.int8)
  rows = np.arange(k)
  for s in STARTS:
    for kind in range(NK):
      for r in range(4):
        c = s + 16 * kind + 5 * r
        if c < d:
          out[:, c] = (kind + rows) % NK
  for j in range(min(d, END)):
    c = d - 1 - j
    out[:, c] = (j % 9 + rows) % NK if j % 9 < NK else -1
  return out


@functools.lru_cache(maxsize=4)
def values(k, d, flip=False):
  """(x, y, kinds): two k x d float32 arrays — x the fma's multiplicand (axpby's x, fma3's q), y the operand scaled first
  (axpby's y, fma3's p) — ordinary rows of scale 1 + row with the special elements written over them.  flip: the
  coefficients a and b have opposite signs (inf_minus_inf and huge then take equal signs)."""
  rng = np.random.default_rng(104729 * k + d % 1000003 + (1 if flip else 0))
  scale = (1.0 + np.arange(k, dtype=F32))[:, None]
  x = rng.standard_normal(size=(k, d), dtype=F32) * scale
  y = rng.standard_normal(size=(k, d), dtype=F32) * scale
  kinds = kind_map(k, d)
  rr, cc = np.nonzero(kinds >= 0)
  opposite = F32(1.0) if flip else F32(-1.0)
  for r, c in zip(rr.tolist(), cc.tolist()):
    kind = KINDS[kinds[r, c]]
    if kind == "nan_x":
      x[r, c] = math.nan
    elif kind == "nan_y":
      y[r, c] = math.nan
    elif kind == "inf":
      x[r, c] = math.inf if c % 2 == 0 else -math.inf
    elif kind == "inf_minus_inf":
      x[r, c] = math.inf
      y[r, c] = opposite * F32(math.inf)
    elif kind == "zeros":
      x[r, c] = -0.0 if c & 1 else 0.0
      y[r, c] = -0.0 if c & 2 else 0.0
    elif kind == "subnormal_in":
      x[r, c] = F32(rng.integers(1, 4096) * 2.0 ** -149) * (1 if c & 1 else -1)
      y[r, c] = F32(rng.integers(1, 4096) * 2.0 ** -149)
    elif kind == "subnormal_out":
      x[r, c] *= F32(2.0 ** -125) / scale[r, 0]
      y[r, c] *= F32(2.0 ** -125) / scale[r, 0]
    else:
      x[r, c] = F32(rng.uniform(3.2e38, 3.39e38))
      y[r, c] = opposite * F32(rng.uniform(2.3e38, 2.5e38))
  for a in (x, y, kinds):
    a.setflags(write=False)
  return x, y, kinds


@functools.lru_cache(maxsize=4)
def finite_values(k, d, seed=0):
  """k x d float32 for the reductions: ordinary rows of scale 1 + row, zeros and subnormals among them (no sum may
  overflow or hold a NaN: the non-finite rows are a case of their own)."""
  rng = np.random.default_rng(15485863 * (seed + 1) + 104729 * k + d % 1000003)
  v = rng.standard_normal(size=(k, d), dtype=F32) * (1.0 + np.arange(k, dtype=F32))[:, None]
  kinds = kind_map(k, d)
  v[kinds == KINDS.index("zeros")] = -0.0
  v[kinds == KINDS.index("subnormal_in")] = F32(2.0 ** -60)      # (tiny, its square still an fp32 number)
  v.setflags(write=False)
  return v


COEFS = ((0.9, 0.1), (1.5, -0.3), (-0.99, 0.01))       # (a, b): a momentum pair, |a| > 1 with a negative b, a negative a
NESTEROV = (1.0, -0.0495)                             # a = 1, b = -mu lr


def factors_for(k, seed=0):
  """float32[64] clipping factors in (0.3, 1), every third one exactly 1."""
  rng = np.random.default_rng(7 + seed)
  f = rng.uniform(0.3, 1.0, size=BM_MAX_ROWS).astype(F32)
  f[::3] = 1.0
  return f


# ---------------------------------------------------------------------------------------------------------------------
# References

MIN_NORMAL = 2.0 ** -126
_TWO128 = Fraction(2) ** 128


def round_f32(v):
  """A Fraction rounded once to float32, ties to even, subnormals and overflow included; returned as a Python float."""
  if v == 0:
    return 0.0
  mag = abs(v)
  e = max(mag.numerator.bit_length() - mag.denominator.bit_length(), -126)
  while mag >= Fraction(2) ** (e + 1):
    e += 1
  while e > -126 and mag < Fraction(2) ** e:
    e -= 1
  q = Fraction(2) ** (e - 23)
  n = mag / q
  lo = n.numerator // n.denominator
  rem = n - lo
  if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and lo % 2):
    lo += 1
  out = lo * q
  if out >= _TWO128:
    return math.copysign(math.inf, v)
  return math.copysign(float(out), v)


def fma_exact(b, x, t):
  """fma(b, x, t) of three finite float32 numbers, exactly: one rounding of b x + t (a zero result takes IEEE's sign)."""
  s = Fraction(float(b)) * Fraction(float(x)) + Fraction(float(t))
  if s == 0:
    prod_negative = math.copysign(1.0, float(b)) * math.copysign(1.0, float(x)) < 0
    return -0.0 if prod_negative and math.copysign(1.0, float(t)) < 0 else 0.0
  return round_f32(s)


Counts = namedtuple("Counts", "midpoints subnormal total")


def fma3_reference(p, q, a, b, factors=None):
  """(out, Counts): out = fl32(b q + fl32(a x)), x = fl32(c_row p) with factors, else p — float32 arrays of one shape
  (rows first).  first_pass_matrix.fma_emulated gives the value and flags the fp32 midpoints of its float64 sum; those
  and every coordinate whose result is not above the smallest normal are evaluated exactly."""
  import torch
  from tests import first_pass_matrix as FP
  p, q = np.ascontiguousarray(p, dtype=F32), np.ascontiguousarray(q, dtype=F32)
  a32, b32 = F32(a), F32(b)
  with np.errstate(all="ignore"):
    x = p if factors is None else p * np.asarray(factors, dtype=F32)[:p.shape[0], None]
    ref, mid = FP.fma_emulated(float(b32), torch.tensor(q), float(a32), torch.tensor(x))
    out = ref.numpy().copy()
    mid = mid.numpy()
    t = x * a32                                               # fl32(a x): what fma_emulated adds
    # (a float64 sum of exactly zero IS the exact sum, its sign IEEE's already: everything else this small is redone)
    small = (np.isfinite(out) & (np.abs(out) <= F32(MIN_NORMAL)) & np.isfinite(q) & np.isfinite(t)
             & (q.astype(np.float64) * float(b32) + t.astype(np.float64) != 0))
  todo = mid | small
  for idx in zip(*np.nonzero(todo)):
    out[idx] = fma_exact(b32, q[idx], t[idx])
  return out, Counts(int(mid.sum()), int(small.sum()), out.size)


def fma3_all_exact(p, q, a, b, factors=None):
  """The same in exact arithmetic on every coordinate whose operands are finite (the others through float64, where no
  rounding is involved): what fma3_reference is held to on the CPU."""
  a32, b32 = F32(a), F32(b)
  with np.errstate(all="ignore"):
    x = p if factors is None else p * np.asarray(factors, dtype=F32)[:p.shape[0], None]
    t = x * a32
    out = (q.astype(np.float64) * float(b32) + t.astype(np.float64)).astype(F32)
  ok = np.isfinite(q) & np.isfinite(t)
  for idx in zip(*np.nonzero(ok)):
    out[idx] = fma_exact(b32, q[idx], t[idx])
  return out


def axpby_reference(y, x, a, b):
  """y <- fl32(b x + fl32(a y)): the fused step with out = p = y, q = x, no factors."""
  return fma3_reference(y, x, a, b)


def scale_reference(y, factors):
  """(fl32(y c_row), rows that must keep their bits: c == 1)."""
  c = np.asarray(factors, dtype=F32)[:y.shape[0]]
  with np.errstate(all="ignore"):
    out = y * c[:, None]
  same = c == F32(1.0)
  out[same] = y[same]
  return out, same


def anticge_multiplier(scal):
  """anticge_multiplier of anticge.hip from scal = (|S|^2, |g|^2) in float64: the fp32 multiplier, or None when the
  vector is left as it is (|S| not > 0)."""
  with np.errstate(all="ignore"):
    att = F32(np.sqrt(np.float64(scal[0])))
    if not att > 0:
      return None
    byz = F32(np.sqrt(np.float64(scal[1])))
    norm = np.float64(byz) if np.isfinite(byz) else np.float64(np.inf)
    return F32(-np.nextafter(norm, np.float64(0.0)) / np.float64(att))


def clip_factors_reference(sq, clip):
  """float32(clip / sqrt(sq)) in float64 where sqrt(sq) > clip, else 1 (a NaN compares false: 1)."""
  sq = np.asarray(sq, dtype=np.float64)
  c = np.float64(F32(clip))
  with np.errstate(all="ignore"):
    norm = np.sqrt(sq)
    return np.where(norm > c, (c / norm).astype(F32), F32(1.0)).astype(F32)


# Numpy twins of five plausible defects, for tests/test_inplace_matrix_cpu.py: the case lists must tell each from the
# reference on their own inputs.

def twin_unfused(p, q, a, b, factors=None):
  """a y + b x with the product rounded: no fusion."""
  with np.errstate(all="ignore"):
    x = p if factors is None else p * np.asarray(factors, dtype=F32)[:p.shape[0], None]
    return x * F32(a) + q * F32(b)


def _fma_with_addend(q, b, t):
  """fl32(b q + t) for a given fp32 addend (through the reference's own path: a = 1, p = t)."""
  return fma3_reference(t, q, 1.0, b)[0]


def twin_factor_after_a(p, q, a, b, factors):
  """fl32(fl32(a p) c) in the place of fl32(a fl32(c p))."""
  with np.errstate(all="ignore"):
    t = (p * F32(a)) * np.asarray(factors, dtype=F32)[:p.shape[0], None]
  return _fma_with_addend(q, b, t)


def twin_b_rounded_twice(b64):
  """The device factor rounded to float32 twice: toward zero first (the double cut to its high part), then to nearest,
  which no longer moves it — one ulp off wherever float32(b) lies above |b|."""
  b = F32(b64)
  if abs(float(b)) > abs(float(b64)):
    b = np.nextafter(b, F32(0.0))
  return b


def twin_tail_at_body_width(flat_bits, start, d, width, new_tail_bits):
  """A tail of d % width columns stored as one whole vector: the width - d % width elements behind the row are written."""
  out = flat_bits.copy()
  body = d // width * width
  if body < d:
    out[start + body:start + body + width] = new_tail_bits
  return out


def twin_scale_all_rows(y, factors):
  """Rows of factor 1 multiplied like the others (a signalling NaN comes back quiet)."""
  c = np.asarray(factors, dtype=F32)[:y.shape[0]]
  with np.errstate(all="ignore"):
    out = y * c[:, None]
  snan = np.isnan(y) & ((y.view(np.uint32) & np.uint32(0x00400000)) == 0)
  bits = out.view(np.uint32).copy()
  bits[snan] = y.view(np.uint32)[snan] | np.uint32(0x00400000)    # what an IEEE multiply by 1 returns
  return bits.view(F32)


# ---------------------------------------------------------------------------------------------------------------------
# The case lists

D_SHORT = (1, 2, 3, 4, 5, 6, 7, 255, 256, 259, 1027, 4100, 4103)   # (6: a 2-column tail behind a body; 4103: a tail behind several workgroups)
K_SHORT = (1, 2, 20, 63, 64)

# A writer case.  offs: (byte offset of the outputs, of the inputs) — a number, or "mixed"; form (fma3): "inplace" (out is
# p), "fresh", "shared_q", "nesterov"; bdev: b in device memory; pscale: clipping factors given; special: what the scale
# and anticge cases vary.
WCase = namedtuple("WCase", "group entry k d out_off in_off form coef bdev pscale special")


def _w(group, entry, k, d, out_off, in_off=None, form="inplace", coef=0, bdev=False, pscale=False, special=None):
  return WCase(group, entry, k, d, out_off, out_off if in_off is None else in_off, form, coef, bdev, pscale, special)


def writer_cases(group, entry, k=None):
  out = []
  if group == "short":
    if entry == ANTICGE:
      for d in D_SHORT:
        for off in (0, 4, 8, 12):
          out.append(_w(group, entry, 1, d, off, special="ordinary"))
      return out
    for kk in (K_SHORT if k is None else (k,)):
      for i, d in enumerate(D_SHORT):
        for off in OFFSETS:
          out.append(_w(group, entry, kk, d, off, coef=i % len(COEFS), special="arbitrary" if i % 2 else "pow2"))
  elif group == "forced":           # only the outputs off, and only the inputs off (the writers with inputs of their own)
    for d in (7, 1027):
      for off in (4, 8):
        if entry == AXPBY:
          out += [_w(group, entry, 20, d, off, 0), _w(group, entry, 20, d, 0, off)]
        elif entry == FMA3:
          out += [_w(group, entry, 20, d, off, 0, form="fresh"), _w(group, entry, 20, d, 0, off, form="fresh")]
  elif group == "second_trip":
    for width, off in ((1, 4), (2, 8), (4, 0)):
      out.append(_w(group, entry, 1 if entry == ANTICGE else 2, second_trip_d(entry, width), off,
                    form="fresh" if entry == FMA3 else "inplace", coef=1, special="ordinary" if entry == ANTICGE else "arbitrary"))
  elif group == "fma3_forms":
    assert entry == FMA3
    for bdev in (False, True):
      for pscale in (False, True):
        for form in ("inplace", "fresh", "shared_q", "nesterov"):
          for d, off in ((1027, 0), (259, 4), (1027, 8), (3, 0)):
            out.append(_w(group, entry, 1 if form == "nesterov" else 20, d, off, form=form,
                          coef=-1 if form == "nesterov" else (1 if pscale else 0), bdev=bdev, pscale=pscale))
  elif group == "scale_special":
    assert entry == SCALE
    for d, off in ((1027, 0), (259, 4), (1027, 8), (3, 0), (1027, "mixed")):
      for special in ("pow2", "arbitrary", "one_on_snan", "zero"):
        out.append(_w(group, entry, 20, d, off, special=special))
  elif group == "anticge_special":
    assert entry == ANTICGE
    for d, off in ((1027, 0), (259, 4), (1027, 8), (3, 0)):
      for special in ("ordinary", "zero_norm", "nan_norm", "inf_byz"):
        out.append(_w(group, entry, 1, d, off, special=special))
  else:
    raise ValueError(group)
  return out


WRITER_GROUPS = {AXPBY: ("short", "forced", "second_trip"), FMA3: ("short", "forced", "second_trip", "fma3_forms"),
                 SCALE: ("short", "second_trip", "scale_special"), ANTICGE: ("short", "second_trip", "anticge_special")}


def all_writer_cases():
  return [c for e in WRITERS for g in WRITER_GROUPS[e] for c in writer_cases(g, e)]


def coef_of(case):
  return NESTEROV if case.coef < 0 else COEFS[case.coef]


def scale_factors(case):
  """float32[64] factors of a bm_multi_scale case."""
  rng = np.random.default_rng(31 + case.d)
  if case.special == "pow2":
    f = (2.0 ** rng.integers(-3, 4, size=BM_MAX_ROWS)).astype(F32)
  else:
    f = rng.uniform(0.2, 1.8, size=BM_MAX_ROWS).astype(F32)
  f[1::4] = 1.0                                      # untouched rows among the others (k = 1: row 0 is scaled)
  if case.special == "one_on_snan":
    f[0] = 1.0
  if case.special == "zero":
    f[0] = 0.0
  return f


SNAN_BITS = (0x7F800001, 0xFF812345, 0x7FBFFFFF, 0x80000000)   # three signalling NaNs and -0


def scale_input(case):
  """The k x d input of a bm_multi_scale case: the y of values(); "one_on_snan" fills row 0 with signalling-NaN bit
  patterns and -0, which a multiply by 1 would not return as they are."""
  y = values(case.k, case.d)[1].copy()
  if case.special == "one_on_snan":
    y.view(np.uint32)[0] = np.resize(np.array(SNAN_BITS, dtype=np.uint32), case.d)
  return y


def anticge_input(case):
  """(vector, scal): the y row of values() — every kind of special element in it — and the two float64 scalars."""
  v = values(8, case.d)[1][3].copy()
  fin = v[np.isfinite(v) & (np.abs(v) < 1e30)].astype(np.float64)
  s2 = float((fin * fin).sum()) or 1.0
  scal = {"ordinary": (s2, 7.25 * s2), "zero_norm": (0.0, 7.25), "nan_norm": (math.nan, 7.25),
          "inf_byz": (s2, math.inf)}[case.special]
  return v, scal


def writer_offsets(case):
  """(byte offsets of the output vectors, of the input vectors that are not outputs)."""
  k = case.k
  if case.entry in (SCALE, ANTICGE):
    return row_offsets(case.out_off, k), []
  if case.entry == AXPBY:
    return row_offsets(case.out_off, k), row_offsets(case.in_off, k, start=k)
  nq = 1 if case.form == "shared_q" else k
  if case.form == "fresh":
    return row_offsets(case.out_off, k), row_offsets(case.in_off, k + nq, start=k)
  return row_offsets(case.out_off, k), row_offsets(case.in_off, nq, start=k)


def writer_pointers(case):
  outs, ins = writer_offsets(case)
  return outs + ins


def writer_launches(case):
  return launches(case.entry, writer_pointers(case), case.d)


Prepared = namedtuple("Prepared", "flat outputs counts roles args")


@functools.lru_cache(maxsize=2)
def _fma_expected(entry, k, d, coef, bdev, pscale, form):
  """The expected rows of an axpby / fma3 case: the same whatever the offsets."""
  a, b = NESTEROV if coef < 0 else COEFS[coef]
  x, y, _ = values(k, d, a * b < 0)
  q = np.broadcast_to(x[0], x.shape) if form == "shared_q" else x
  factors = factors_for(k) if pscale else None
  b_used = F32(np.float64(b)) if bdev else F32(b)
  return fma3_reference(y, q, a, b_used, factors)


def prepare(case):
  """The host image of a writer case, the expected outputs {vector index: (values, exact)}, the Counts of exactly
  resolved coordinates, the roles (name -> vector indices) and the scalar arguments."""
  k, d = case.k, case.d
  outs_off, ins_off = writer_offsets(case)
  if case.entry == SCALE:
    y = scale_input(case)
    f = scale_factors(case)
    want, same = scale_reference(y, f)
    flat = Flat(list(y), outs_off)
    return Prepared(flat, {i: (want[i], bool(same[i])) for i in range(k)}, Counts(0, 0, y.size), {"y": list(range(k))},
                    {"factors": f})
  if case.entry == ANTICGE:
    v, scal = anticge_input(case)
    m = anticge_multiplier(scal)
    with np.errstate(all="ignore"):
      want = v if m is None else v * m
    flat = Flat([v], outs_off)
    return Prepared(flat, {0: (want, m is None)}, Counts(0, 0, v.size), {"y": [0]}, {"scal": scal, "multiplier": m})
  a, b = coef_of(case)
  x, y, _ = values(k, d, a * b < 0)
  want, counts = _fma_expected(case.entry, k, d, case.coef, case.bdev, case.pscale, case.form)
  qs = [x[0]] if case.form == "shared_q" else list(x)
  if case.entry == AXPBY or case.form != "fresh":
    vectors = list(y) + qs
    roles = {"out": list(range(k)), "p": list(range(k)), "q": [k] * k if case.form == "shared_q" else list(range(k, 2 * k))}
  else:
    vectors = [np.zeros(d, dtype=F32)] * k + list(y) + qs
    roles = {"out": list(range(k)), "p": list(range(k, 2 * k)),
             "q": [2 * k] * k if case.form == "shared_q" else list(range(2 * k, 3 * k))}
  flat = Flat(vectors, outs_off + ins_off)
  return Prepared(flat, {i: (want[i], False) for i in range(k)}, counts, roles,
                  {"a": a, "b": b, "factors": factors_for(k) if case.pscale else None})


# Reduction cases
RCase = namedtuple("RCase", "group entry k d offs nc ne special")
SQDIST_OFFS = ((0, 0), (4, 4), (8, 8), (0, 4), (8, 0))
DOT_NE = (0, 1, 31, 32)


def reduction_cases(entry, group=None):
  out = []
  if entry == SQNORMS:
    for k in K_SHORT:
      for d in D_SHORT:
        for off in OFFSETS:
          out.append(RCase("short", entry, k, d, off, 0, 0, None))
    out.append(RCase("fold", entry, 2, sqnorm_fold_d(1), 4, 0, 0, None))
    out.append(RCase("fold", entry, 2, sqnorm_fold_d(4), 0, 0, 0, None))
    for d, off in ((1027, 0), (4103, 0), (1027, 4), (4100, 8)):
      out.append(RCase("areas", entry, 64, d, off, 0, 0, None))
    for off in (0, 4):
      out.append(RCase("nonfinite", entry, 5, 1027, off, 0, 0, "nonfinite"))
  elif entry == SQDIST2:
    for d in D_SHORT:
      for offs in SQDIST_OFFS:
        out.append(RCase("short", entry, 2, d, offs, 0, 0, None))
    out.append(RCase("fold", entry, 2, sqdist_fold_d(), (4, 4), 0, 0, "hot_lane"))
    for d, offs in ((1027, (0, 0)), (259, (4, 4))):
      out.append(RCase("equal", entry, 2, d, offs, 0, 0, "equal"))
    out.append(RCase("empty", entry, 2, 0, (0, 0), 0, 0, None))
  elif entry == DOT:
    for nc in range(1, K_MAX_CORE + 1):
      for ne in DOT_NE:
        for d in (3, 1027):
          for off in OFFSETS:
            out.append(RCase("short", entry, nc + ne, d, off, nc, ne, None))
  else:
    raise ValueError(entry)
  return [c for c in out if group is None or c.group == group]


def all_reduction_cases():
  return [c for e in REDUCTIONS for c in reduction_cases(e)]


def reduction_offsets(case):
  if case.entry == SQDIST2:
    return list(case.offs)
  return row_offsets(case.offs, case.k)


def reduction_launches(case):
  return launches(case.entry, reduction_offsets(case), case.d)


def reduction_input(case):
  """The k x d float32 rows of a reduction case."""
  v = finite_values(case.k, case.d).copy() if case.d else np.zeros((case.k, 0), dtype=F32)
  if case.special == "nonfinite":
    v[1, 5] = math.nan
    v[3, case.d - 2] = math.inf
  elif case.special == "equal":
    v[1] = v[0]
  elif case.special == "hot_lane":
    # the columns lane 0 of workgroup 0 walks (0, stride, 2 stride, ...) carry the weight of the sum: the one lane that
    # folds decides the result
    stride = SITES[SQDIST2].cap_tail * SITES[SQDIST2].block
    v[0, ::stride] += F32(4000.0)
  return v


BAR_SQ = 1e-6                     # relative, sums of squares: test_sums_of_squares_and_axpby_at_every_width
BAR_DOT = 1e-6                    # of |a| |b|, dots: the same test


def reduction_reference(case, v):
  """float64: row_sqnorms -> k sums; sqdist2 -> one; multi_dot -> (nc x nc Gram, ne extras, norms of the k rows)."""
  v64 = v.astype(np.float64)
  with np.errstate(all="ignore"):
    if case.entry == SQNORMS:
      return (v64 * v64).sum(axis=1)
    if case.entry == SQDIST2:
      return float(((v64[0] - v64[1]) ** 2).sum())
    core, extra = v64[:case.nc], v64[case.nc:]
    return core @ core.T, extra @ core[0] if case.ne else np.zeros(0), np.sqrt((v64 * v64).sum(axis=1))


# ---------------------------------------------------------------------------------------------------------------------
# Running a case on the GPU

DEV = "cuda:0"


def _bm():
  import byzantinemomentum_amd
  byzantinemomentum_amd._lib.load()
  return byzantinemomentum_amd


def upload(flat):
  """(the device allocation, the views of its vectors)."""
  import torch
  dev = torch.from_numpy(flat.bits.view(np.int32)).to(DEV).view(torch.float32)
  assert dev.data_ptr() % 256 == 0
  views = [dev[s:s + n] for s, n in zip(flat.starts, flat.lengths)]
  for v, o in zip(views, flat.offsets):
    assert v.data_ptr() % 16 == o
  return dev, views


def download(dev):
  import torch
  return dev.view(torch.int32).cpu().numpy().view(np.uint32)


def run_writer(case, prepared=None, entry_point=None):
  """Runs a writer case; returns (the bits of the whole allocation after the call, Prepared).  Through the package's
  wrappers, or through the C entry points where a wrapper refuses the count (more than 64 tensors in one validated
  list) or `entry_point` is "c"."""
  import ctypes
  import torch
  bm = _bm()
  lib = bm._lib.load()
  pre = prepare(case) if prepared is None else prepared
  dev, views = upload(pre.flat)
  table = bm._lib.pointer_table
  if case.entry == SCALE:
    bm.stats.multi_scale([views[i] for i in pre.roles["y"]], torch.from_numpy(pre.args["factors"]).to(DEV))
  elif case.entry == ANTICGE:
    bm.stats.anticge_scale(views[0], torch.tensor(pre.args["scal"], dtype=torch.float64, device=DEV))
  else:
    outs, ps, qs = ([views[i] for i in pre.roles[r]] for r in ("out", "p", "q"))
    a, b = pre.args["a"], pre.args["b"]
    factors = None if pre.args["factors"] is None else torch.from_numpy(pre.args["factors"]).to(DEV)
    bdev = torch.tensor([b], dtype=torch.float64, device=DEV) if case.bdev else None
    direct = case.k + 1 > bm._lib.MAX_ROWS or entry_point == "c"
    if case.entry == AXPBY:
      if direct:
        rc = lib.bm_multi_axpby(table(outs), table(qs), case.k, case.d, ctypes.c_float(a), ctypes.c_float(b), None)
        assert rc == 0, (case, rc)
      else:
        bm.stats.multi_axpby(outs, qs, a, b)
    elif direct:
      scale = None if factors is None else ctypes.c_void_p(factors.data_ptr())
      if case.bdev:
        rc = lib.bm_multi_fma3_bdev(table(outs), table(ps), table(qs), case.k, case.d, ctypes.c_float(a),
                                    ctypes.c_void_p(bdev.data_ptr()), scale, None)
      else:
        rc = lib.bm_multi_fma3(table(outs), table(ps), table(qs), case.k, case.d, ctypes.c_float(a), ctypes.c_float(b),
                               scale, None)
      assert rc == 0, (case, rc)
    else:
      bm.stats.multi_fma3(outs, ps, qs, a, bdev if case.bdev else b, factors)
  torch.cuda.synchronize()
  return download(dev), pre


def check_writer(case, got_bits, pre):
  """None, or a description of the first element that is not what it must be: an output (bit for bit, a NaN matching any
  NaN), an input or a guard gap (the very bits)."""
  want, loose = pre.flat.expected(pre.outputs)
  at = first_mismatch(got_bits, want, loose)
  if at is None:
    return None
  vec, pos = pre.flat.where(at)
  what = "guard gap" if vec is None else ("output" if vec in pre.outputs else "input")
  return dict(case=case._asdict(), what=what, vector=vec, position=pos, got=hex(int(got_bits[at])), want=hex(int(want[at])),
              launches=[tuple(l) for l in writer_launches(case)])



def with_device_multiplier(case, got_bits, pre):
  """bm_anticge_scale with a finite multiplier: (Prepared whose expected vector is fl32(v m) of the multiplier the DEVICE
  used, that multiplier, the float64 one -sqrt(scal[1]) / sqrt(scal[0])) — the multiplier read off the ordinary elements
  with anticge_reference.multiplier_of (None when no fp32 number explains them).  Other cases: (pre, None, None)."""
  m = pre.args.get("multiplier")
  if case.entry != ANTICGE or m is None or not np.isfinite(m):
    return pre, None, None
  import torch
  from tests import anticge_reference as AR
  s = pre.flat.starts[0]
  v, after = pre.flat.bits[s:s + case.d].view(F32), got_bits[s:s + case.d].view(F32)
  plain = np.isfinite(v) & (np.abs(v) > 1e-3) & (np.abs(v) < 1e3)
  if not plain.any():
    return pre, None, None
  m_dev = AR.multiplier_of(torch.tensor(after[plain]), torch.tensor(v[plain]))
  want64 = -math.sqrt(pre.args["scal"][1]) / math.sqrt(pre.args["scal"][0])
  if m_dev is None:
    return pre, None, want64
  with np.errstate(all="ignore"):
    return pre._replace(outputs={0: (v * F32(m_dev), False)}), m_dev, want64


def run_reduction(case, v=None):
  """The float64 results of a reduction case as numpy: k sums, one sum, or the 64 doubles of bm_multi_dot's `out`
  pre-filled with a sentinel.  Returns (result, bits of the allocation after the call, Flat)."""
  import ctypes
  import torch
  bm = _bm()
  lib = bm._lib.load()
  v = reduction_input(case) if v is None else v
  flat = Flat(list(v), reduction_offsets(case))
  dev, views = upload(flat)
  if case.entry == SQNORMS:
    res = bm.stats.row_sqnorms(views).cpu().numpy()
  elif case.entry == SQDIST2:
    res = bm.stats.sqdist2(views[0], views[1]).cpu().numpy()
  else:
    out = torch.full((64,), -12345.5, dtype=torch.float64, device=DEV)
    ws = bm.gars._workspace(torch.device(DEV), bm._lib.WS_DOT, 1, case.d, "ws_dot")
    core, extra = views[:case.nc], views[case.nc:]
    rc = lib.bm_multi_dot(bm._lib.pointer_table(core), case.nc, bm._lib.pointer_table(extra) if extra else None, case.ne,
                          case.d, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), None)
    assert rc == 0, (case, rc)
    res = out.cpu().numpy()
  torch.cuda.synchronize()
  return res, download(dev), flat


def check_reduction(case, res, v):
  """(worst error in units of the bar, list of misses)."""
  want = reduction_reference(case, v)
  worst, misses = 0.0, []

  def hold(name, got, ref, scale, bar):
    nonlocal worst
    if not math.isfinite(ref):
      if not (math.isnan(got) if math.isnan(ref) else got == ref):
        misses.append((name, got, ref))
      return
    err = abs(got - ref) / (bar * scale) if scale > 0 else (0.0 if got == ref else math.inf)
    worst = max(worst, err)
    if not err <= 1.0:
      misses.append((name, got, ref, err))

  if case.entry == SQNORMS:
    assert res.shape == (case.k,)
    for i in range(case.k):
      hold(f"row {i}", float(res[i]), float(want[i]), float(want[i]), BAR_SQ)
  elif case.entry == SQDIST2:
    hold("sqdist2", float(res[0]), want, want, BAR_SQ)
  else:
    gram, extras, norms = want
    nc, ne = case.nc, case.ne
    for i in range(nc):
      for j in range(nc):
        hold(f"gram {i} {j}", float(res[i * nc + j]), float(gram[i, j]), float(norms[i] * norms[j]), BAR_DOT)
        if res[i * nc + j] != res[j * nc + i]:
          misses.append(("transpose", i, j))
    for e in range(ne):
      hold(f"extra {e}", float(res[nc * nc + e]), float(extras[e]), float(norms[0] * norms[nc + e]), BAR_DOT)
    if not (res[nc * nc + ne:] == -12345.5).all():
      misses.append(("written beyond nc^2 + ne", res[nc * nc + ne:].tolist()[:4]))
  return worst, misses
