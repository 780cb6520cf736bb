// center.cpp — bm_center_weights: the weights of the geometric median / centered clipping from an N x N matrix of
// squared distances ON THE HOST (pure host code: no kernel, no HIP call).  The iteration is center_core.h's, the one the
// device form (center.hip) runs: the two are compared bit for bit.
#include <cmath>
#include <cstdint>

#include "center_core.h"
#include "search_core.h"  // butterfly_order_sum: the order of the sums over the points

namespace {

// The host walks the 64 points of a phase one after the other; nothing to wait for between phases.
struct HostPar {
  int begin() const { return 0; }
  int end() const { return BM_MAX_ROWS; }
  void sync() const {}
  double sum(const double (&slots)[BM_MAX_ROWS]) const { return bm::butterfly_order_sum(slots); }
};

}  // namespace

extern "C" int bm_center_weights(const double* sq_host, int n, int has_start, int mode, double param, int iters,
                                 double tol, double* weights_out, double* info_out) {
  using namespace bm;
  if (sq_host == nullptr || weights_out == nullptr || info_out == nullptr ||
      !center_args_ok(n, has_start, mode, param, iters, tol))
    return BM_EINVAL;
  CenterState st;
  HostPar par;
  center_run(sq_host, n + has_start, n, has_start, mode, param, iters, tol, st, info_out, par);
  for (int i = 0; i < BM_MAX_ROWS; ++i) weights_out[i] = st.c[i];
  return 0;
}
