// minmax_core.h — the closed form of the Min-Max / Min-Sum factor (include/bm_gar.h, bm_minmax_factor) from the h x h
// squared distances and the BM_PERTURB_SLOTS scalars of bm_perturb_stats.  One definition, compiled for the host form
// (minmax.cpp) and the device form (minmax.hip); the whole library is built with -ffp-contract=off and both sides
// round sqrt and the quotient correctly, so the two give the same bits (tests/test_gpu_minmax.py).
//
// Order of every fp64 sum: PLAIN INDEX ORDER.  minmax_row adds row i of D over j = 0 .. h-1; minmax_finish adds the
// rows' sums, the a_i and the b_i over i = 0 .. h-1.  A row is one lane's work on the device, the finish one lane's:
// h <= 64 terms, a few microseconds, and nothing to keep in step between two forms.
#pragma once
#include <math.h>

#include "bm_common.h"

namespace bm {

constexpr int kMinmaxOut = 6;  // { gamma, bound, binding row, P, N, degenerate }
constexpr int kPerturbP = BM_MAX_ROWS, kPerturbN = BM_MAX_ROWS + 1;  // the slots of |p|^2 and |avg|^2

__host__ __device__ inline bool minmax_args_ok(int h, int mode) {
  return h >= 2 && h <= BM_MAX_ROWS && (mode == BM_MINMAX || mode == BM_MINSUM);
}

__host__ __device__ inline bool minmax_finite(double v) { return v - v == 0.0; }

// Row i of D (row length ld): its sum over j in index order, and its largest entry right of the diagonal (-inf on the
// last row, NaN when it holds one).
__host__ __device__ inline void minmax_row(const double* D, int ld, int h, int i, double* rowsum, double* rowmax) {
  double s = 0.0, m = -INFINITY;
  for (int j = 0; j < h; ++j) {
    const double v = D[i * ld + j];
    s = s + v;
    if (j > i) m = (v != v || m != m) ? NAN : (v > m ? v : m);
  }
  *rowsum = s;
  *rowmax = m;
}

// The rest, sequential: scal = { b_0 .. b_{h-1}, ..., P, N }.
__host__ __device__ inline void minmax_finish(const double* rowsum, const double* rowmax, const double* scal, int h,
                                              int mode, double* out) {
  const double hh = (double)h;
  const double P = scal[kPerturbP], N = scal[kPerturbN];
  double total = 0.0;
  for (int i = 0; i < h; ++i) total = total + rowsum[i];
  const double shift = total / (2.0 * hh * hh);
  bool ok = P > 0.0 && minmax_finite(P);
  double gamma = 0.0, bound, binding = -1.0;
  if (mode == BM_MINMAX) {
    bound = rowmax[0];
    for (int i = 1; i < h - 1; ++i) {
      const double m = rowmax[i];
      bound = (m != m || bound != bound) ? NAN : (m > bound ? m : bound);
    }
    ok = ok && minmax_finite(bound);
    double best = INFINITY;
    int arg = -1;
    for (int i = 0; i < h && ok; ++i) {
      double a = rowsum[i] / hh - shift;
      if (a <= 0.0) a = 0.0;
      const double b = scal[i];
      const double disc = b * b + P * (bound - a);
      if (!minmax_finite(a) || !minmax_finite(b) || !(disc >= 0.0)) {
        ok = false;
        break;
      }
      const double g = (-b + sqrt(disc)) / P;
      if (g < best) {  // strict: ties go to the lower index
        best = g;
        arg = i;
      }
    }
    ok = ok && arg >= 0 && minmax_finite(best);
    if (ok) {
      gamma = best;
      binding = (double)arg;
    }
  } else {
    bound = rowsum[0];
    double A = 0.0, B = 0.0;
    for (int i = 0; i < h; ++i) {
      const double s = rowsum[i];
      bound = (s != s || bound != bound) ? NAN : (s > bound ? s : bound);
      double a = s / hh - shift;
      if (a <= 0.0) a = 0.0;
      A = A + a;
      B = B + scal[i];
    }
    const double disc = B * B + hh * P * (bound - A);
    ok = ok && minmax_finite(bound) && minmax_finite(A) && minmax_finite(B) && disc >= 0.0;
    if (ok) {
      const double g = (-B + sqrt(disc)) / (hh * P);
      ok = minmax_finite(g);
      if (ok) gamma = g;
    }
  }
  out[0] = gamma;
  out[1] = bound;
  out[2] = binding;
  out[3] = P;
  out[4] = N;
  out[5] = ok ? 0.0 : 1.0;
}

}  // namespace bm
