// nnm.cpp — bm_nnm_masks: the neighbour masks of nearest-neighbour mixing from an n x n matrix of squared distances ON
// THE HOST (pure host code: no kernel, no HIP call).  The membership rule is nnm_core.h's, the one the device form
// (nnm.hip) evaluates: the two are compared bit for bit.
#include <cstdint>

#include "nnm_core.h"

extern "C" int bm_nnm_masks(const double* sq_host, int n, int f, uint64_t* masks_host) {
  using namespace bm;
  if (sq_host == nullptr || masks_host == nullptr || !nnm_args_ok(n, f)) return BM_EINVAL;
  for (int i = 0; i < BM_MAX_ROWS; ++i) {
    uint64_t m = 0;
    if (i < n)
      for (int j = 0; j < n; ++j) m |= nnm_member(sq_host + (int64_t)i * n, n, n - f, i, j) ? (uint64_t)1 << j : 0;
    masks_host[i] = m;
  }
  return 0;
}
