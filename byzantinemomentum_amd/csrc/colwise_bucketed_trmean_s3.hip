// colwise_bucketed_trmean_s3.hip — instances of one rule on the means of buckets of 3 (contract: colwise_bucketed.hip, launch logic: colwise_bucketed_dispatch.h).
#include "colwise_bucketed_dispatch.h"

namespace bm {
int colwise_bucketed_trmean_s3(const float* const* rows, int n, const uint64_t* masks, int n_out, int64_t d, int f, float* out,
                               hipStream_t stream) {
  return colwise_bucketed_dispatch<BM_OP_TRMEAN, 3, 2, bucketed_max_rows(3)>(rows, n, masks, n_out, d, f, out, stream);
}
}  // namespace bm
