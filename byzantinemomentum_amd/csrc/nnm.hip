// nnm.hip — bm_nnm_masks_device: the neighbour masks of nearest-neighbour mixing from the n x n squared distances where
// bm_pairwise_sqdist left them, in ONE workgroup, so that
//     distances -> masks -> bm_mix_rows / bm_colwise_mixed
// are launches on one stream with no copy and no synchronisation between them (a HIP graph records them).  The
// membership rule is nnm_core.h's, the one the host form (nnm.cpp) walks: same masks, bit for bit.
#include "bm_common.h"
#include "nnm_core.h"

namespace bm {

constexpr int kNnmParts = 4;                          // lanes per row: lane (i, q) answers for j = q, q + 4, ...
constexpr int kNnmBlock = BM_MAX_ROWS * kNnmParts;    // 256: the four lanes of a row are neighbours in one wave
constexpr int kNnmLd = BM_MAX_ROWS + 1;               // odd row length: the lanes of a wave walk 16 rows without a bank conflict

__global__ __launch_bounds__(kNnmBlock) void nnm_masks_kernel(const double* __restrict__ sq, int n, int k,
                                                              uint64_t* __restrict__ masks) {
  __shared__ double D[BM_MAX_ROWS * kNnmLd];
  const int tid = threadIdx.x;
  for (int p = tid; p < n * n; p += kNnmBlock) {
    const int i = p / n, j = p - i * n;
    D[i * kNnmLd + j] = sq[p];
  }
  __syncthreads();
  const int i = tid / kNnmParts, q = tid % kNnmParts;
  uint64_t m = 0;
  if (i < n)
    for (int j = q; j < n; j += kNnmParts) m |= nnm_member(D + i * kNnmLd, n, k, i, j) ? (uint64_t)1 << j : 0;
  // OR over the four lanes of the row (neighbours: xor 1, 2 stay inside the group)
  m |= __shfl_xor(m, 1, 64);
  m |= __shfl_xor(m, 2, 64);
  if (q == 0) masks[i] = m;  // BM_MAX_ROWS masks: zeros beyond n
}

}  // namespace bm

extern "C" int bm_nnm_masks_device(const double* sq_dev, int n, int f, uint64_t* masks_dev, void* stream) {
  using namespace bm;
  if (sq_dev == nullptr || masks_dev == nullptr || !nnm_args_ok(n, f)) return BM_EINVAL;
  hipLaunchKernelGGL(nnm_masks_kernel, dim3(1), dim3(kNnmBlock), 0, static_cast<hipStream_t>(stream), sq_dev, n, n - f,
                     masks_dev);
  BM_LAUNCH_CHECK();
  return 0;
}
