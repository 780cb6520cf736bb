// spectral_core.h — the spectral filtering rules CAF (covariance-bound agnostic filter) and DnC (spectral outlier
// removal) evaluated ON SCALARS, shared by the host form (spectral.cpp, bm_spectral_weights) and the device form
// (spectral.hip, bm_spectral_weights_device).
//
// With weights c >= 0 on the rows (C = sum c), mu = sum c_i x_i / C and y_i = x_i - mu, every quantity of the rules is a
// function of the n x n squared distances D:  r_i = sum_k c_k D_ik / C,  s = sum_i c_i r_i / C,
//     <y_i, y_j> = K_ij = -1/2 (D_ij - r_i - r_j + s),      |y_i|^2 = r_i - s / 2,
// and a direction v = sum_i z_i y_i is carried as its coefficients z:  <y_i, v> = (K z)_i
//     = -1/2 (sum_j D_ij z_j - r_i Z - sum_j r_j z_j + s Z),  Z = sum z:  one row-dot on D per row and two sums, K is
// never formed.  A power step of the weighted covariance is z <- c o (K z) / C, rescaled (the scale of v is immaterial
// until the end); after the steps q = K z gives |v|^2 = z . q, the projections g_i = q_i / sqrt(z . q), the variance
// along v, lambda = sum c_i q_i^2 / (C z . q), and tau_i / tau_max = q_i^2 / max q^2.  An evaluation costs T + 2 row-dot
// sweeps, whatever d is.
//
// ONE definition for both sides, written as center_core.h is: phases over the rows par.begin() .. par.end() - 1
// separated by par.sync(); sums and maxima over the rows through par.sum() / par.sum2() / par.max() of 64 slots (sums in
// the butterfly order of search_core.h); the row-dots of a sweep through par.dots(), which adds the terms of a row in
// LANES interleaved chains (chain l: the terms j = l, l + LANES, ... in index order; spectral_partial_dot) and the
// chains in index order — the device gives each chain a lane.  LANES = 1 is center_row_dot.  The library is built with
// -ffp-contract=off: the device form is tested bit for bit against the host form.
#pragma once
#include "bm_common.h"
#include "center_core.h"

namespace bm {

// Lanes per row-dot (chains per row): 256 threads, four waves.  BM_SPECTRAL_LANES = 1 selects the one-chain form on
// both sides (an A/B knob: profiles/spectral_timings.txt).
constexpr int kSpectralLanes = 4;

// The state of a run: on the host's stack, in LDS on the device (one copy per wave: every wave computes every row).
struct SpectralState {
  double c[BM_MAX_ROWS];     // the weights of the round (0 on unusable rows and beyond n)
  double sc[BM_MAX_ROWS];    // sqrt(c)
  double z[BM_MAX_ROWS];     // the coefficients of the direction
  double r[BM_MAX_ROWS];     // r_i
  double q[BM_MAX_ROWS];     // (K z)_i, then tau_i
  double w[BM_MAX_ROWS];     // the start keys, then the raw coefficients of a power step
  double best[BM_MAX_ROWS];  // the weights that are returned (sum 1)
  double slot[BM_MAX_ROWS];  // the terms of a sum over the rows
  double slot2[BM_MAX_ROWS];
  int usable[BM_MAX_ROWS];
};

// Chain `l` of `lanes` of sum_j w_j D_ij: the terms j = l, l + lanes, ... < N in index order; terms with w_j == 0 are
// skipped (their D_ij may be NaN: an unusable row).  Loads in groups of eight at clamped indices, as center_row_dot.
template <int LANES>
__host__ __device__ inline double spectral_partial_dot(const double* w, const double* drow, int N, int l) {
  if (LANES == 1) return center_row_dot(w, drow, N);
  double s = 0.0;
  for (int j0 = l; j0 < N; j0 += 8 * LANES) {
    double wj[8], dj[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int j = j0 + q * LANES < N ? j0 + q * LANES : N - 1;
      wj[q] = w[j];
      dj[q] = drow[j];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) s += (j0 + q * LANES < N && wj[q] != 0.0) ? wj[q] * dj[q] : 0.0;
  }
  return s;
}

// One evaluation E(c) of st.c (C = sum c > 0).  Returns false when it is degenerate (no row off the weighted mean, or a
// direction of no length); else st.q holds tau_i = q_i^2 on the rows of weight (0 elsewhere; a NaN counts as +inf) and
// lambda the variance along the direction.
template <class Par>
__host__ __device__ inline bool spectral_evaluate(const double* D, int ld, int n, int T, double C, SpectralState& st,
                                                  double& lambda, Par& par) {
  par.sync();
  par.dots(st.c, D, ld, n, st.r);
  for (int i = par.begin(); i < par.end(); ++i) {
    const double ci = st.c[i];
    const bool live = i < n && ci != 0.0;
    const double ri = live ? st.r[i] / C : 0.0;
    st.r[i] = ri;
    st.sc[i] = live ? sqrt(ci) : 0.0;
    st.slot[i] = live ? ci * ri : 0.0;
  }
  const double s = par.sum(st.slot) / C;
  // the start: the row farthest from the weighted mean, by c_i |y_i|^2 (the uniform vector is in K's null space)
  for (int i = par.begin(); i < par.end(); ++i) {
    const double key = st.c[i] != 0.0 ? st.c[i] * (st.r[i] - 0.5 * s) : 0.0;
    st.w[i] = key > 0.0 ? key : 0.0;  // (a NaN key counts 0)
    st.slot[i] = st.w[i];
  }
  const double top = par.max(st.slot);
  if (!(top > 0.0)) return false;
  for (int i = par.begin(); i < par.end(); ++i) st.slot[i] = (i < n && st.w[i] == top) ? -(double)i : -(double)BM_MAX_ROWS;
  const int first = (int)(-par.max(st.slot));  // ties to the lowest index
  for (int i = par.begin(); i < par.end(); ++i) st.z[i] = i == first ? st.sc[i] : 0.0;
  for (int t = 0;; ++t) {
    par.sync();
    par.dots(st.z, D, ld, n, st.q);
    for (int i = par.begin(); i < par.end(); ++i) {
      const double zi = st.z[i];
      st.slot[i] = zi;
      st.slot2[i] = zi != 0.0 ? st.r[i] * zi : 0.0;
    }
    double Z, R;
    par.sum2(st.slot, st.slot2, Z, R);
    const double sZ = s * Z;
    for (int i = par.begin(); i < par.end(); ++i) {
      double kz = 0.0;
      if (st.c[i] != 0.0) {
        kz = st.q[i] - st.r[i] * Z;
        kz = kz - R;
        kz = kz + sZ;
        kz = -0.5 * kz;
      }
      st.q[i] = kz;
    }
    if (t == T) break;
    for (int i = par.begin(); i < par.end(); ++i) {
      const double wi = st.c[i] != 0.0 ? st.sc[i] * st.q[i] / C : 0.0;
      st.w[i] = wi;
      st.slot[i] = wi * wi;
    }
    const double norm2 = par.sum(st.slot);
    if (!(norm2 > 0.0) || !center_finite(norm2)) break;  // no further step: st.q is K z of the direction that stays
    const double norm = sqrt(norm2);
    for (int i = par.begin(); i < par.end(); ++i) st.z[i] = st.sc[i] * (st.w[i] / norm);
  }
  for (int i = par.begin(); i < par.end(); ++i) {
    const double zi = st.z[i], qi = st.q[i];
    st.slot[i] = zi != 0.0 ? zi * qi : 0.0;
    st.slot2[i] = st.c[i] != 0.0 ? st.c[i] * (qi * qi) : 0.0;
  }
  double zq, cq2;
  par.sum2(st.slot, st.slot2, zq, cq2);
  if (!(zq > 0.0)) return false;
  lambda = cq2 / (C * zq);
  for (int i = par.begin(); i < par.end(); ++i) {
    const double t2 = st.q[i] * st.q[i];
    st.q[i] = st.c[i] != 0.0 ? (t2 == t2 ? t2 : __builtin_inf()) : 0.0;
  }
  return true;
}

// D: the n x n squared distances, row i at D + i * ld.  info: { rounds evaluated, best lambda, usable rows, the round
// whose weights are kept (-1: none) }, written by the caller that holds row 0 and par.writes().  On return st.best
// holds the n weights, then zeros.
template <class Par>
__host__ __device__ inline void spectral_run(const double* D, int ld, int n, int mode, int count, int T,
                                             SpectralState& st, double* info, Par& par) {
  const double kNaN = __builtin_nan(""), kInf = __builtin_inf();
  // usable rows: center_core.h's predicate
  for (int i = par.begin(); i < par.end(); ++i) {
    int bad = 0;
#pragma unroll 8
    for (int j = 0; j < n; ++j) bad += (i < n && j != i && !center_finite(D[i * ld + j])) ? 1 : 0;
    const bool ok = i < n && !(bad > 0 && 2 * bad >= n - 1);
    st.usable[i] = ok ? 1 : 0;
    st.slot[i] = ok ? 1.0 : 0.0;
  }
  const double U = par.sum(st.slot);  // (an exact small integer)
  double best_lambda = kInf;
  int kept = -1, rounds = 0;
  if (!(U > 0.0)) {
    for (int i = par.begin(); i < par.end(); ++i) st.best[i] = i < n ? kNaN : 0.0;
  } else {
    for (int i = par.begin(); i < par.end(); ++i) {
      st.c[i] = st.usable[i] ? 1.0 : 0.0;
      st.best[i] = st.usable[i] ? 1.0 / U : 0.0;
    }
    if (mode == BM_SPECTRAL_CAF) {
      const double floor_mass = (double)(n - 2 * count);  // of the original n: unusable rows are mass already filtered
      for (int round = 0; round < n; ++round) {
        par.sync();
        for (int i = par.begin(); i < par.end(); ++i) st.slot[i] = st.c[i];
        const double C = par.sum(st.slot);
        if (!(C > floor_mass)) break;
        double lambda = 0.0;
        if (!spectral_evaluate(D, ld, n, T, C, st, lambda, par)) break;
        rounds = round + 1;
        if (lambda < best_lambda) {
          best_lambda = lambda;
          kept = round;
          for (int i = par.begin(); i < par.end(); ++i) st.best[i] = st.c[i] / C;
        }
        for (int i = par.begin(); i < par.end(); ++i) st.slot[i] = st.q[i];
        const double tmax = par.max(st.slot);
        if (!(tmax > 0.0)) break;
        // the soft filter: the row of largest tau gets exactly 0
        for (int i = par.begin(); i < par.end(); ++i) {
          const double ti = st.q[i];
          const double ratio = ti == tmax ? 1.0 : ti / tmax;
          st.c[i] = st.c[i] != 0.0 ? st.c[i] * (1.0 - ratio) : 0.0;
        }
      }
    } else {
      double lambda = 0.0;
      if (spectral_evaluate(D, ld, n, T, U, st, lambda, par)) {
        best_lambda = lambda;
        kept = 0;
        rounds = 1;
      } else {
        for (int i = par.begin(); i < par.end(); ++i) st.q[i] = 0.0;  // degenerate: every tau is 0
      }
      par.sync();
      // remove the usable rows of largest tau, the higher index first among equals
      const int drop = count - (n - (int)U) > 0 ? count - (n - (int)U) : 0;
      for (int i = par.begin(); i < par.end(); ++i) {
        const double ti = st.q[i];
        int before = 0;
        for (int j = 0; j < n; ++j) {
          const double tj = st.q[j];
          before += (st.usable[j] != 0 && (tj > ti || (tj == ti && j > i))) ? 1 : 0;
        }
        st.best[i] = (st.usable[i] != 0 && before >= drop) ? 1.0 / (U - (double)drop) : 0.0;
      }
    }
  }
  for (int i = par.begin(); i < par.end(); ++i)
    if (i == 0 && par.writes()) {
      info[0] = (double)rounds;
      info[1] = best_lambda;
      info[2] = U > 0.0 ? U : 0.0;
      info[3] = (double)kept;
    }
  par.sync();
}

constexpr int kSpectralMaxPowerIters = 256;

// Arguments both entry points refuse before doing anything.
inline bool spectral_args_ok(int n, int mode, int count, int power_iters) {
  if (n < 1 || n > BM_MAX_ROWS) return false;
  if (power_iters < 1 || power_iters > kSpectralMaxPowerIters) return false;
  if (mode == BM_SPECTRAL_CAF) return count >= 0 && 2 * count < n;
  if (mode == BM_SPECTRAL_DNC) return count >= 0 && count < n;
  return false;
}

}  // namespace bm
