// mixdist.cpp — bm_mixed_sqdist and bm_mix_weights ON THE HOST (pure host code: no kernel, no HIP call): the squared
// distances between mixed rows from the distances of the original rows, and the weights of the original rows behind a
// weighted sum or a selection of mixed rows.  The arithmetic is mixdist_core.h's, the one the device forms (mixdist.hip)
// evaluate: the two are compared bit for bit.
#include <cstdint>

#include "mixdist_core.h"

extern "C" int bm_mixed_sqdist(const double* sq_host, int n_in, const uint64_t* masks_host, int n_out, double* out_host) {
  using namespace bm;
  if (sq_host == nullptr || masks_host == nullptr || out_host == nullptr || !mixdist_args_ok(n_in, n_out)) return BM_EINVAL;
  for (int a = 0; a < n_out; ++a)
    if (!mixdist_mask_ok(masks_host[a], n_in)) return BM_EINVAL;
  double Q[BM_MAX_ROWS * BM_MAX_ROWS];  // Q[i * n_out + b]
  double diag[BM_MAX_ROWS];
  for (int i = 0; i < n_in; ++i)
    for (int b = 0; b < n_out; ++b) Q[i * n_out + b] = mixdist_q(sq_host, n_in, n_in, i, masks_host[b]);
  for (int a = 0; a < n_out; ++a) diag[a] = mixdist_p(Q, n_out, n_in, masks_host[a], a);
  for (int a = 0; a < n_out; ++a) {
    out_host[a * n_out + a] = masks_host[a] == 0 ? __builtin_nan("") : 0.0;
    for (int b = a + 1; b < n_out; ++b) {
      const int x = mixdist_first(masks_host[a], masks_host[b]) ? a : b, y = a + b - x;
      const double v = mixdist_entry(mixdist_p(Q, n_out, n_in, masks_host[x], y), diag[x], diag[y], masks_host[x], masks_host[y]);
      out_host[a * n_out + b] = v;
      out_host[b * n_out + a] = v;
    }
  }
  return 0;
}

extern "C" int bm_mix_weights(const uint64_t* masks_host, int n_in, int n_out, const double* w_mixed, const int32_t* sel, int m,
                              double* w_out_host) {
  using namespace bm;
  if (masks_host == nullptr || w_out_host == nullptr || !mixw_args_ok(n_in, n_out, w_mixed, sel, m)) return BM_EINVAL;
  for (int r = 0; r < n_out; ++r)
    if (!mixdist_mask_ok(masks_host[r], n_in)) return BM_EINVAL;
  double w[BM_MAX_ROWS];
  bool ok = true;
  if (sel != nullptr) {
    ok = mixw_sel_ok(sel, m, n_out);
    for (int r = 0; r < n_out; ++r) w[r] = ok ? mixw_from_sel(sel, m, r) : 0.0;
  } else {
    for (int r = 0; r < n_out; ++r) w[r] = w_mixed[r];
  }
  ok = ok && mixw_rows_ok(w, masks_host, n_out);
  for (int j = 0; j < BM_MAX_ROWS; ++j)
    w_out_host[j] = j >= n_in ? 0.0 : ok ? mixw_entry(w, masks_host, n_out, j) : __builtin_nan("");
  return 0;
}
