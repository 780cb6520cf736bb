// center_core.h — the geometric median (smoothed Weiszfeld) and centered clipping iterated ON SCALARS, shared by the
// host form (center.cpp, bm_center_weights) and the device form (center.hip, bm_center_weights_device).
//
// Every iterate of both rules is an affine combination v = sum_j c_j p_j (sum c = 1) of the points p_0 .. p_{N-1} (the n
// rows and, for centered clipping, the start vector as point n), so with D the N x N squared distances of the points
//     |p_i - v|^2 = sum_j c_j D_ij - 1/2 sum_jk c_j c_k D_jk = t_i - q / 2,    t_i = sum_j c_j D_ij,  q = sum_i c_i t_i
// and an iteration is O(N^2) flops on the weights instead of two passes over n d-sized rows (the scalar form of the
// factor search, search_core.h, used the same way).
//
// ONE definition for both sides: center_run() is written as phases over the points; a phase handles the points
// par.begin() .. par.end() - 1 (the host: all 64, one after the other; the device: lane i handles point i), phases are
// separated by par.sync(), and a sum over the points is par.sum() of 64 slots in the butterfly order of search_core.h
// (slot[i] + slot[i ^ 1], then ^ 2, ... ^ 32), which a wave follows with all its lanes at once.  The sums over j inside
// a point (center_row_dot) run in index order.  The library is built with -ffp-contract=off, so what is written here is
// what both sides compute: the device form is tested bit for bit against the host form.
#pragma once
#include "bm_common.h"

namespace bm {

// The state of the iteration: on the host's stack, in LDS on the device.
struct CenterState {
  double c[BM_MAX_ROWS];     // the weights of the iterate (sum 1; 0 beyond N and on unusable points)
  double e[BM_MAX_ROWS];     // the change of c in the current iteration
  double t[BM_MAX_ROWS];     // t_i, then the per-row value of the step (w_i or s_i)
  double slot[BM_MAX_ROWS];  // the terms of a sum over the points
  int usable[BM_MAX_ROWS];
};

__host__ __device__ inline bool center_finite(double v) { return __builtin_fabs(v) < __builtin_inf(); }

// sum_j w_j D_ij over j < N in index order; terms with w_j == 0 are skipped (their D_ij may be NaN: an unusable point)
// (In groups of eight whose loads leave together, at clamped indices, a term beyond N adding 0.0: one dependent LDS
//  read per term made an iteration at 25 points 4.4 us instead of 3.5, profiles/center_timings.txt.  The additions stay one chain.)
__host__ __device__ inline double center_row_dot(const double* w, const double* drow, int N) {
  double s = 0.0;
  for (int j0 = 0; j0 < N; j0 += 8) {
    double wj[8], dj[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int j = j0 + q < N ? j0 + q : N - 1;
      wj[q] = w[j];
      dj[q] = drow[j];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) s += (j0 + q < N && wj[q] != 0.0) ? wj[q] * dj[q] : 0.0;
  }
  return s;
}

// |p_i - v| from t_i and q: sqrt(max(0, t_i - q / 2)), a non-finite square counts as +inf (krum.py:46-47)
__host__ __device__ inline double center_radius(double t_i, double q) {
  const double r2 = t_i - 0.5 * q;
  if (!center_finite(r2)) return __builtin_inf();
  return sqrt(r2 < 0.0 ? 0.0 : r2);
}

// D: the N x N squared distances, row i at D + i * ld.  info: { iterations run, move^2 of the last one, usable rows }
// (written by every caller of the phase that holds point 0).  On return st.c holds the N weights, then zeros.
template <class Par>
__host__ __device__ inline void center_run(const double* D, int ld, int n, int has_start, int mode, double param,
                                           int iters, double tol, CenterState& st, double* info, Par& par) {
  const int N = n + (has_start ? 1 : 0);
  const double kNaN = __builtin_nan("");
  // usable points: D_ij non-finite for at least one and at least half of the other points -> never any weight (the
  // copies of the `nan` attack, whether or not the distance pass gave aliased NaN rows a finite mutual distance)
  for (int i = par.begin(); i < par.end(); ++i) {
    int bad = 0;
#pragma unroll 8
    for (int j = 0; j < N; ++j) bad += (i < N && j != i && !center_finite(D[i * ld + j])) ? 1 : 0;
    const bool ok = i < N && !(bad > 0 && 2 * bad >= N - 1);
    st.usable[i] = ok ? 1 : 0;
    st.slot[i] = (ok && i < n) ? 1.0 : 0.0;
  }
  const double U = par.sum(st.slot);  // the usable ROWS (an exact small integer)
  if (!(U > 0.0)) {
    for (int i = par.begin(); i < par.end(); ++i) {
      st.c[i] = i < N ? kNaN : 0.0;
      if (i == 0) {
        info[0] = 0.0;
        info[1] = kNaN;
        info[2] = 0.0;
      }
    }
    par.sync();
    return;
  }
  // start: the start vector when it is given and usable, else uniform over the usable rows
  const bool from_start = has_start && st.usable[n] != 0;
  for (int i = par.begin(); i < par.end(); ++i) {
    const bool row = i < n && st.usable[i] != 0;
    st.c[i] = from_start ? (i == n ? 1.0 : 0.0) : (row ? 1.0 / U : 0.0);
  }
  par.sync();
  int done = 0;
  double move2 = 0.0;
  for (int it = 0; it < iters; ++it) {
    for (int i = par.begin(); i < par.end(); ++i) {
      const double ti = i < N ? center_row_dot(st.c, D + i * ld, N) : 0.0;
      const double ci = st.c[i];
      st.t[i] = ti;
      st.slot[i] = (i < N && ci != 0.0) ? ci * ti : 0.0;
    }
    const double q = par.sum(st.slot);
    for (int i = par.begin(); i < par.end(); ++i) {
      const bool row = i < n && st.usable[i] != 0;
      const double r = center_radius(st.t[i], q);
      double w = 0.0;
      if (row) w = mode == BM_CENTER_GEOMED ? 1.0 / (r > param ? r : param) : (r <= param ? 1.0 : param / r);
      st.t[i] = w;
      st.slot[i] = w;
    }
    const double W = par.sum(st.slot);
    for (int i = par.begin(); i < par.end(); ++i) {
      const double old = st.c[i];
      double next = 0.0;
      if (i < N) {
        if (mode == BM_CENTER_GEOMED) {
          next = st.t[i] / W;
        } else {
          next = old * (1.0 - W / U);
          next = next + st.t[i] / U;
        }
      }
      st.e[i] = next - old;
      st.c[i] = next;
    }
    par.sync();
    // the squared length of the step, |sum_j e_j p_j|^2 = -1/2 sum_jk e_j e_k D_jk (sum e = 0)
    for (int i = par.begin(); i < par.end(); ++i) {
      const double ui = i < N ? center_row_dot(st.e, D + i * ld, N) : 0.0;
      const double ei = st.e[i];
      st.slot[i] = (i < N && ei != 0.0) ? ei * ui : 0.0;
    }
    move2 = -0.5 * par.sum(st.slot);
    move2 = move2 <= 0.0 ? 0.0 : move2;  // (max(0, .): a -0 becomes +0, a NaN stays)
    done = it + 1;
    if (tol > 0.0 && sqrt(move2) <= tol) break;
  }
  for (int i = par.begin(); i < par.end(); ++i)
    if (i == 0) {
      info[0] = (double)done;
      info[1] = move2;
      info[2] = U;
    }
  par.sync();
}

// Arguments both entry points refuse before doing anything.
inline bool center_args_ok(int n, int has_start, int mode, double param, int iters, double tol) {
  if (has_start != 0 && has_start != 1) return false;
  if (n < 1 || n + has_start > BM_MAX_ROWS) return false;
  if (mode != BM_CENTER_GEOMED && mode != BM_CENTER_CCLIP) return false;
  if (!(param > 0.0) || !center_finite(param)) return false;
  if (iters < 1 || iters > 64) return false;
  if (!(tol >= 0.0) || !center_finite(tol)) return false;
  return true;
}

}  // namespace bm
