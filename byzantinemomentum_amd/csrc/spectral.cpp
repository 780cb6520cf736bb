// spectral.cpp — bm_spectral_weights: the weights of CAF / DnC from an n x n matrix of squared distances ON THE HOST
// (pure host code: no kernel, no HIP call).  The evaluation is spectral_core.h's, the one the device form
// (spectral.hip) runs: the two are compared bit for bit.
#include <cmath>
#include <cstdint>

#include "search_core.h"  // butterfly_order_sum: the order of the sums over the rows
#include "spectral_core.h"

namespace {

// The host walks the 64 rows of a phase one after the other; nothing to wait for between phases.  A row-dot is the
// LANES chains of the device's lanes, one after the other, added in index order.
template <int LANES>
struct HostPar {
  int begin() const { return 0; }
  int end() const { return BM_MAX_ROWS; }
  bool writes() const { return true; }
  void sync() const {}
  double sum(const double (&slots)[BM_MAX_ROWS]) const { return bm::butterfly_order_sum(slots); }
  void sum2(const double (&a)[BM_MAX_ROWS], const double (&b)[BM_MAX_ROWS], double& sa, double& sb) const {
    sa = bm::butterfly_order_sum(a);
    sb = bm::butterfly_order_sum(b);
  }
  double max(const double (&slots)[BM_MAX_ROWS]) const {
    double m = slots[0];
    for (int i = 1; i < BM_MAX_ROWS; ++i) m = slots[i] > m ? slots[i] : m;
    return m;
  }
  void dots(const double* w, const double* D, int ld, int N, double* out) const {
    for (int i = 0; i < BM_MAX_ROWS; ++i) {
      double s = 0.0;
      if (i < N) {
        s = bm::spectral_partial_dot<LANES>(w, D + i * ld, N, 0);
        for (int l = 1; l < LANES; ++l) s = s + bm::spectral_partial_dot<LANES>(w, D + i * ld, N, l);
      }
      out[i] = s;
    }
  }
};

template <int LANES>
void run(const double* sq, int n, int mode, int count, int power_iters, double* weights_out, double* info_out) {
  bm::SpectralState st;
  HostPar<LANES> par;
  bm::spectral_run(sq, n, n, mode, count, power_iters, st, info_out, par);
  for (int i = 0; i < BM_MAX_ROWS; ++i) weights_out[i] = st.best[i];
}

}  // namespace

extern "C" int bm_spectral_weights(const double* sq_host, int n, int mode, int count, int power_iters,
                                   double* weights_out, double* info_out) {
  using namespace bm;
  if (sq_host == nullptr || weights_out == nullptr || info_out == nullptr ||
      !spectral_args_ok(n, mode, count, power_iters))
    return BM_EINVAL;
  if (tuning().spectral_lanes == 1)
    run<1>(sq_host, n, mode, count, power_iters, weights_out, info_out);
  else
    run<kSpectralLanes>(sq_host, n, mode, count, power_iters, weights_out, info_out);
  return 0;
}
