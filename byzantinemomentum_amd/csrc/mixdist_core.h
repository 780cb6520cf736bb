// mixdist_core.h — the squared distances BETWEEN mixed rows, and the weights of the ORIGINAL rows behind a weighted sum
// of mixed rows, from scalars alone; shared by the host forms (mixdist.cpp: bm_mixed_sqdist, bm_mix_weights) and the
// device forms (mixdist.hip).
//
// A mixed row is y_a = (1 / c_a) sum_{i in mask_a} x_i, so with w = W_a - W_b (W_a = mask_a / c_a)
//     |y_a - y_b|^2 = -1/2 w' D w = P_ab / (c_a c_b) - 1/2 P_aa / c_a^2 - 1/2 P_bb / c_b^2,
//     P_ab = sum_{i in mask_a} Q_ib,   Q_ib = sum_{j in mask_b, j != i} D_ij,
// D the squared distances of the original rows: no mixed row has to exist for a rule that reads distances only.
//
// ONE definition for both sides, and the library is built with -ffp-contract=off: mixdist_q() and mixdist_p() are
// sequential fp64 sums in ascending index order from +0, mixdist_entry() is the closing expression, evaluated left to
// right.  The host walks every (i, b) and (a, b); the device gives each lane a few of them.  Same bits.
#pragma once
#include "bm_common.h"

namespace bm {

__host__ __device__ inline int mixdist_popcount(uint64_t m) {
  int c = 0;
  for (; m; m &= m - 1) ++c;
  return c;
}

__host__ __device__ inline bool mixdist_finite(double x) { return x - x == 0.0; }

// Q_ib: D (leading dimension ld) is read at (min(i, j), max(i, j)), j in mask_b ascending, j != i; the diagonal and
// every j outside the mask are not read.
__host__ __device__ inline double mixdist_q(const double* D, int ld, int n_in, int i, uint64_t mask_b) {
  double s = 0.0;
  for (int j = 0; j < n_in; ++j)
    if (j != i && ((mask_b >> j) & 1)) s = s + (i < j ? D[i * ld + j] : D[j * ld + i]);
  return s;
}

// P_ab: Q (leading dimension ld, Q[i * ld + b]) over i in mask_a ascending.
__host__ __device__ inline double mixdist_p(const double* Q, int ld, int n_in, uint64_t mask_a, int b) {
  double s = 0.0;
  for (int i = 0; i < n_in; ++i)
    if ((mask_a >> i) & 1) s = s + Q[i * ld + b];
  return s;
}

// Which row of a pair walks the outer sum: the one with the smaller mask WORD (the lower index when they are equal, and
// then the pair takes no arithmetic).  P_xy and P_yx are the same sum in two orders and differ in their last bits; with
// the order taken from the masks and not from the indices, an entry is a function of the two masks alone — rows with
// equal masks get bitwise-equal rows of the output, which the exact-tie handling of the rules relies on.
__host__ __device__ inline bool mixdist_first(uint64_t mask_a, uint64_t mask_b) { return mask_a <= mask_b; }

// out_xy for x != y, x the row mixdist_first names.  An empty mask: NaN (bm_mix_rows writes a NaN row there).  Equal masks: +0 by this test, not by
// arithmetic — such a pair reads no distance.  A non-finite distance read for the pair makes one of the three sums
// non-finite: NaN, and the clamp (a comparison that a NaN fails) leaves a NaN alone.
__host__ __device__ inline double mixdist_entry(double p_ab, double p_aa, double p_bb, uint64_t mask_a, uint64_t mask_b) {
  if (mask_a == 0 || mask_b == 0) return __builtin_nan("");
  if (mask_a == mask_b) return 0.0;
  if (!mixdist_finite(p_ab) || !mixdist_finite(p_aa) || !mixdist_finite(p_bb)) return __builtin_nan("");
  const double ca = (double)mixdist_popcount(mask_a), cb = (double)mixdist_popcount(mask_b);
  const double v = p_ab / (ca * cb) - 0.5 * p_aa / (ca * ca) - 0.5 * p_bb / (cb * cb);
  return v <= 0.0 ? 0.0 : v;  // (-0 and every negative value to +0; a NaN fails the comparison and stays)
}

// "no bit at or above n_in"
__host__ __device__ inline bool mixdist_mask_ok(uint64_t m, int n_in) { return n_in >= 64 || (m >> n_in) == 0; }

inline bool mixdist_args_ok(int n_in, int n_out) {
  return n_in >= 1 && n_in <= BM_MAX_ROWS && n_out >= 1 && n_out <= BM_MAX_ROWS;
}

// ---------------------------------------------------------------------------
// Weights of the original rows.  The weight of mixed row r is w_mixed[r], or, from an index table, 1 / m per entry of
// sel[0 .. m) that names r (added one entry at a time from +0, in table order).
__host__ __device__ inline double mixw_from_sel(const int32_t* sel, int m, int r) {
  const double each = 1.0 / (double)m;
  double w = 0.0;
  for (int t = 0; t < m; ++t)
    if (sel[t] == r) w = w + each;
  return w;
}

// An entry of the table outside 0 .. n_out-1 (bm_brute_select_device leaves -1 after a search that gave up) poisons the
// result, as bm_selected_mean answers it with NaN.
__host__ __device__ inline bool mixw_sel_ok(const int32_t* sel, int m, int n_out) {
  bool ok = true;
  for (int t = 0; t < m; ++t) ok = ok && sel[t] >= 0 && sel[t] < n_out;
  return ok;
}

// A mixed row that counts (weight != 0, a NaN included) but has an empty mask is a NaN row: it poisons the result too.
__host__ __device__ inline bool mixw_rows_ok(const double* w, const uint64_t* masks, int n_out) {
  bool ok = true;
  for (int r = 0; r < n_out; ++r) ok = ok && (w[r] == 0.0 || masks[r] != 0);
  return ok;
}

// w_out[j] = sum over r ascending, w_r != 0 and bit j of mask_r set, of w_r / c_r.
__host__ __device__ inline double mixw_entry(const double* w, const uint64_t* masks, int n_out, int j) {
  double s = 0.0;
  for (int r = 0; r < n_out; ++r)
    if (w[r] != 0.0 && ((masks[r] >> j) & 1)) s = s + w[r] / (double)mixdist_popcount(masks[r]);
  return s;
}

inline bool mixw_args_ok(int n_in, int n_out, const void* w_mixed, const void* sel, int m) {
  if (!mixdist_args_ok(n_in, n_out)) return false;
  if ((w_mixed == nullptr) == (sel == nullptr)) return false;
  return sel == nullptr || (m >= 1 && m <= BM_MAX_ROWS);
}

}  // namespace bm
