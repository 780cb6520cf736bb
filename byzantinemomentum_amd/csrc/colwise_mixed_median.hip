// colwise_mixed_median.hip — instances of one rule on mixed rows (contract: colwise_mixed.hip, launch logic: colwise_mixed_dispatch.h).
#include "colwise_mixed_dispatch.h"

namespace bm {
int colwise_mixed_median(const float* const* rows, int n, const uint64_t* masks, int64_t d, int f, float* out,
                         hipStream_t stream) {
  return colwise_mixed_dispatch<BM_OP_MEDIAN, 1, kMixedMaxRows>(rows, n, masks, d, f, out, stream);
}
}  // namespace bm
