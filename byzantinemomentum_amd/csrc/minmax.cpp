// minmax.cpp — bm_minmax_factor: the closed-form factor of the Min-Max / Min-Sum attacks from an h x h matrix of
// squared distances and the scalars of bm_perturb_stats ON THE HOST (pure host code: no kernel, no HIP call).  The
// evaluation is minmax_core.h's, the one the device form (minmax.hip) runs: the two are compared bit for bit.
#include "minmax_core.h"

extern "C" int bm_minmax_factor(const double* sq_host, const double* scal_host, int h, int mode, double* out_host) {
  using namespace bm;
  if (sq_host == nullptr || scal_host == nullptr || out_host == nullptr || !minmax_args_ok(h, mode)) return BM_EINVAL;
  double rowsum[BM_MAX_ROWS], rowmax[BM_MAX_ROWS];
  for (int i = 0; i < h; ++i) minmax_row(sq_host, h, h, i, &rowsum[i], &rowmax[i]);
  minmax_finish(rowsum, rowmax, scal_host, h, mode, out_host);
  return 0;
}
