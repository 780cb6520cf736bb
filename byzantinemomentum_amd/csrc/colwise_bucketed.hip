// colwise_bucketed.hip — bm_colwise_bucketed: bucketing (or any mixing into n_out < n rows) fused into the coordinate-wise
// median and trimmed mean.  The column is loaded once, the n_out mixed values y_r = mean of the rows in mask_r
// (mix_kernels.h: the sequential fp32 sum of bm_mix_rows, bit for bit) are formed in registers and column_rule
// (colwise_kernels.h) runs on them: 4 d (n + 1) bytes where bm_mix_rows + bm_colwise move 4 d (n + 2 n_out + 1).  Same
// bits as bm_colwise on the rows bm_mix_rows writes (tests/test_gpu_bucketed.py).
#include "colwise_bucketed_dispatch.h"  // bucketed_max_rows, bucketed_n_out (no instance is made here)

namespace bm {
// one translation unit per rule and bucket size (colwise_bucketed_<rule>_s<S>.hip, launch logic in
// colwise_bucketed_dispatch.h); each answers BM_EINVAL for an n_out that is not its own ceil(n / S)
using BucketedRule = int(const float* const* rows, int n, const uint64_t* masks, int n_out, int64_t d, int f, float* out,
                         hipStream_t stream);
BucketedRule colwise_bucketed_median_s2, colwise_bucketed_median_s3, colwise_bucketed_trmean_s2, colwise_bucketed_trmean_s3;
}  // namespace bm

extern "C" int bm_colwise_bucketed_supported(int op, int n, int n_out) {
  using namespace bm;
  if (op != BM_OP_MEDIAN && op != BM_OP_TRMEAN) return 0;
  if (n < 2) return 0;
  for (int s = 2; s <= 3; ++s)
    if (n <= bucketed_max_rows(s) && n_out == bucketed_n_out(n, s)) return 1;
  return 0;
}

extern "C" int bm_colwise_bucketed(int op, const float* const* rows, int n, const uint64_t* masks_dev, int n_out,
                                   int64_t d, int f, float* out, void* stream) {
  using namespace bm;
  if (rows == nullptr || masks_dev == nullptr || (out == nullptr && d > 0) || n < 1 || n > BM_MAX_ROWS || n_out < 1 ||
      n_out > n || d < 0)
    return BM_EINVAL;
  if (op != BM_OP_MEDIAN && op != BM_OP_TRMEAN) return BM_EINVAL;
  if (op == BM_OP_TRMEAN && (f < 0 || n_out < 2 * f + 1)) return BM_EINVAL;
  if (!bm_colwise_bucketed_supported(op, n, n_out)) return BM_EINVAL;
  if (d == 0) return 0;
  for (int i = 0; i < n; ++i)
    if (rows[i] == nullptr) return BM_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // (n = 2, 4: both bucket sizes give one count, the instance is s = 2's)
  const bool two = n <= bucketed_max_rows(2) && n_out == bucketed_n_out(n, 2);
  if (op == BM_OP_MEDIAN) return (two ? colwise_bucketed_median_s2 : colwise_bucketed_median_s3)(rows, n, masks_dev, n_out, d, 0, out, s);
  return (two ? colwise_bucketed_trmean_s2 : colwise_bucketed_trmean_s3)(rows, n, masks_dev, n_out, d, f, out, s);
}
