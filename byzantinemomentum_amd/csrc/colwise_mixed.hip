// colwise_mixed.hip — bm_colwise_mixed: nearest-neighbour mixing fused into the coordinate-wise median and trimmed
// mean.  The column is loaded once, the n mixed values y_r = mean of the rows in mask_r (mix_kernels.h: the sequential
// fp32 sum of bm_mix_rows, bit for bit) are formed in registers and column_rule (colwise_kernels.h) runs on them: the
// stack is read once and d floats are written, 4 d (n + 1) bytes, as for the plain rules.  Same bits as bm_colwise on
// the rows bm_mix_rows writes (tests/test_gpu_nnm.py).
#include "colwise_mixed_dispatch.h"  // kMixedMaxRows (no instance is made here)

namespace bm {
// one translation unit per rule (colwise_mixed_<rule>.hip, launch logic in colwise_mixed_dispatch.h)
using MixedRule = int(const float* const* rows, int n, const uint64_t* masks, int64_t d, int f, float* out,
                      hipStream_t stream);
MixedRule colwise_mixed_median, colwise_mixed_trmean;
}  // namespace bm

extern "C" int bm_colwise_mixed_max_rows(void) { return bm::kMixedMaxRows; }

extern "C" int bm_colwise_mixed(int op, const float* const* rows, int n, const uint64_t* masks_dev, int64_t d, int f,
                                float* out, void* stream) {
  using namespace bm;
  if (rows == nullptr || masks_dev == nullptr || (out == nullptr && d > 0) || n < 1 || n > kMixedMaxRows || d < 0)
    return BM_EINVAL;
  if (op != BM_OP_MEDIAN && op != BM_OP_TRMEAN) return BM_EINVAL;
  if (op == BM_OP_TRMEAN && (f < 0 || n < 2 * f + 1)) return BM_EINVAL;
  if (d == 0) return 0;
  for (int i = 0; i < n; ++i)
    if (rows[i] == nullptr) return BM_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (op == BM_OP_MEDIAN) return colwise_mixed_median(rows, n, masks_dev, d, 0, out, s);
  return colwise_mixed_trmean(rows, n, masks_dev, d, f, out, s);
}
