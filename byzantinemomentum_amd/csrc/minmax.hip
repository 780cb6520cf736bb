// minmax.hip — bm_minmax_factor_device: the closed-form factor of the Min-Max / Min-Sum attacks from the h x h squared
// distances where bm_pairwise_sqdist left them and the scalars where bm_perturb_stats left them, in ONE workgroup, so that
//     distances, perturbation scalars -> factor -> bm_multi_fma3_bdev
// are launches on one stream with no copy and no synchronisation between them.  The evaluation is minmax_core.h's, the
// one the host form (minmax.cpp) runs: same bits.  Lane i adds row i of D (in LDS); lane 0 runs the sequential rest.
#include "minmax_core.h"

namespace bm {

constexpr int kMinmaxLd = BM_MAX_ROWS + 1;  // odd row length: lane i walking row i meets no bank conflict

__global__ __launch_bounds__(64) void minmax_factor_kernel(const double* __restrict__ sq, const double* __restrict__ scal,
                                                           int h, int mode, double* __restrict__ out) {
  __shared__ double D[BM_MAX_ROWS * kMinmaxLd];
  __shared__ double rowsum[BM_MAX_ROWS], rowmax[BM_MAX_ROWS];
  const int lane = threadIdx.x;
  for (int p = lane; p < h * h; p += 64) {
    const int i = p / h, j = p - i * h;
    D[i * kMinmaxLd + j] = sq[p];
  }
  __syncthreads();
  if (lane < h) minmax_row(D, kMinmaxLd, h, lane, &rowsum[lane], &rowmax[lane]);
  __syncthreads();
  if (lane == 0) minmax_finish(rowsum, rowmax, scal, h, mode, out);
}

}  // namespace bm

extern "C" int bm_minmax_factor_device(const double* sq_dev, const double* scal_dev, int h, int mode, double* out_dev,
                                       void* stream) {
  using namespace bm;
  if (sq_dev == nullptr || scal_dev == nullptr || out_dev == nullptr || !minmax_args_ok(h, mode)) return BM_EINVAL;
  hipLaunchKernelGGL(minmax_factor_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), sq_dev, scal_dev, h,
                     mode, out_dev);
  BM_LAUNCH_CHECK();
  return 0;
}
